"""The pose granule of a resident session, {lo32, tag, hi32, tag} (glim_amd/csrc/pose_granule.hpp), on the host, no GPU.

The host stores a pose value into the session's device memory as two aligned 8-byte halves, each with the request's tag; a block takes a granule
only when both tags agree.  tests/pose_granule_check.cpp packs 100 000 seeded values and reads them back the way a block loads them: every
granule round-trips, and a granule with one half written under another tag (the neighbouring request, a cleared granule, the exit tag) is rejected."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
GRANULES = 100000


def test_pose_granule_round_trips_and_rejects_a_foreign_half(tmp_path):
    exe = str(tmp_path / "pose_granule_check")
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "glim_amd", "csrc"),
                           os.path.join(ROOT, "tests", "pose_granule_check.cpp"), "-o", exe], timeout=600)
    out = subprocess.run([exe, str(GRANULES)], capture_output=True, text=True, timeout=120, check=True).stdout
    r = dict(line.split() for line in out.splitlines())
    assert int(r["granules"]) == GRANULES, r
    assert r["round_trip_failures"] == "0", r
    assert r["foreign_halves_accepted"] == "0", r
