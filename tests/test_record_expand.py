"""The expansion of a compact record into the caller's dense blocks (glim_amd/csrc/record_expand.hpp) on the host, no GPU.

A binary factor's target blocks are H_tt = Ad^T H_ss Ad, H_ts = -Ad^T H_ss and b_t = -Ad^T b_s with Ad = Adjoint(delta^-1), whose upper right
3x3 block is structurally zero.  The expansion leaves the terms of that block out of its sums and takes the adjoint from the caller, who computes
it while the device works.  For finite records that must not change one bit: tests/record_expand_check.cpp keeps the earlier form (full six-term
sums) as a copy and runs both over 100 000 seeded finite records, unary and binary.  It is compiled twice with the library's compiler, host side
only -- -O0 and -O3 -march=native (an FMA-capable target); the hashes must agree within a build (old == new) and across the builds (no
contraction)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
RECORDS = 100000


def _run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", *flags, "-I", os.path.join(ROOT, "glim_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "record_expand_check.cpp"), "-o", exe], timeout=600)
    out = subprocess.run([exe, str(RECORDS)], capture_output=True, text=True, timeout=120, check=True).stdout
    return dict(line.split() for line in out.splitlines())


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    d = tmp_path_factory.mktemp("record_expand")
    return {"O0": _run(d, "check_O0", ["-O0"]), "O3_native": _run(d, "check_O3", ["-O3", "-Xarch_host", "-march=native"])}


def test_old_and_new_expansion_agree_within_each_build(builds):
    for name, r in builds.items():
        assert int(r["records"]) >= RECORDS, (name, r)
        assert r["mismatching_values"] == "0", (name, r)
        assert r["hash_old"] == r["hash_new"], (name, r)


def test_no_contraction_across_optimisation_levels(builds):
    assert builds["O0"]["hash_old"] == builds["O3_native"]["hash_old"], builds
    assert builds["O0"]["hash_new"] == builds["O3_native"]["hash_new"], builds
