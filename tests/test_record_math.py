"""The record math of a VGICP linearisation (glim_amd/csrc/device_math.hpp "record math") on the host, no GPU.

A small synchronous linearisation returns RAW records (the summed accumulators) and the host applies the R^T B R rotation and the slot mapping
(finish_raw_record: rotate_part + compact_from_rot); every other form rotates on the device, one rotate_element per slot.  All forms have to give
the same bits, so the shared code must not be contracted into fused multiply-adds by the HOST compiler either.  tests/record_math_check.cpp is
compiled twice with the library's compiler, host side only -- -O0 and -O3 -march=native (an FMA-capable target) -- and hashes both forms over
100 000 seeded random records plus the special ones (zeros, -0.0, a record whose finaliser lost a row: NaN everywhere).  The hashes must agree
within a build (rotate_element == rotate_part) and across the builds (no contraction), and the NaN count must reach compact slot 0, where
records_lost() looks for it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
RECORDS = 100000


def _run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", *flags, "-I", os.path.join(ROOT, "glim_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "record_math_check.cpp"), "-o", exe], timeout=600)
    out = subprocess.run([exe, str(RECORDS)], capture_output=True, text=True, timeout=120, check=True).stdout
    return dict(line.split() for line in out.splitlines())


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    d = tmp_path_factory.mktemp("record_math")
    return {"O0": _run(d, "check_O0", ["-O0"]), "O3_native": _run(d, "check_O3", ["-O3", "-Xarch_host", "-march=native"])}


def test_host_finish_and_device_form_agree_within_each_build(builds):
    for name, r in builds.items():
        assert int(r["records"]) >= RECORDS + 3, (name, r)
        assert r["mismatching_values"] == "0", (name, r)
        assert r["hash_finish"] == r["hash_element"], (name, r)


def test_no_contraction_across_optimisation_levels(builds):
    assert builds["O0"]["hash_finish"] == builds["O3_native"]["hash_finish"], builds
    assert builds["O0"]["hash_element"] == builds["O3_native"]["hash_element"], builds


def test_nan_count_reaches_compact_slot_0(builds):
    for name, r in builds.items():
        assert r["nan_count_in_slot0"] == "1", (name, r)
