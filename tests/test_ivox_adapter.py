"""Builds tests/cpp/test_ivox_adapter.cpp (the device iVox mirror of include/glim_amd/gtsam_points_compat.hpp and the factors over it in
adapters/gtsam/glim_amd_gtsam.hpp) against the stand-in GTSAM / Eigen / gtsam_points headers of tests/cpp/mock/ and runs it on the GPU box: the
HessianFactor blocks equal the C records of the same evaluations over the same map."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_ivox_adapter.cpp")


def _build(tmp_path):
    from glim_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exe = str(tmp_path / "test_ivox_adapter")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "mock"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "adapters", "gtsam"), SRC, "-o", exe, "-L" + os.path.join(ROOT, "glim_amd"), "-lglim_amd",
           "-Wl,-rpath," + os.path.join(ROOT, "glim_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(cmd)
    return exe


def test_ivox_adapter_compiles_against_the_stand_in_headers(tmp_path):
    _build(tmp_path)


@pytest.mark.gpu
def test_ivox_adapter_blocks_equal_the_c_record_on_gpu(tmp_path):
    exe = _build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "test_ivox_adapter OK" in out.stdout
