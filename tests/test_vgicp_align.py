"""VGICP fine registration (include/glim_amd.h "VGICP fine registration"), the part that needs no device: the ABI surface, the default parameters
and the argument errors that are answered before any HIP call.  The step rule itself is tests/cpp/test_lm_step.cpp's (tests/test_gicp_align.py)."""
import ctypes as C
import subprocess

import numpy as np

import lm_restatement as lmr
from align_cases import build_cpp, check_symbols

NEW_STABLE = ["glim_amd_vgicp_align_default_params", "glim_amd_vgicp_align_batch"]
NEW_DIAG = ["glim_amd_debug_vgicp_align_trace"]
INVALID = -1


def test_new_symbols_are_declared_once_and_listed():
    mirror = check_symbols(NEW_STABLE, NEW_DIAG, "vgicp_align.hpp")
    assert "glim_amd_vgicp_align_batch" in mirror
    assert '#include "gicp_align.hpp"' in mirror  # LMParams, AlignResult and, through it, the wrappers of gtsam_points_compat.hpp
    from glim_amd import api

    for n in ("vgicp_align_batch", "vgicp_align_debug_trace"):
        assert callable(getattr(api, n))
    assert callable(api.IntegratedVGICPFactorGPU.align)


def test_default_params_are_the_gicp_defaults():
    from glim_amd import _lib

    p, q = _lib.LMParams(), _lib.LMParams()
    assert _lib.lib().glim_amd_vgicp_align_default_params(C.byref(p)) == 0
    assert {k: getattr(p, k) for k, _ in _lib.LMParams._fields_} == lmr.DEFAULTS
    assert _lib.lib().glim_amd_gicp_align_default_params(C.byref(q)) == 0
    assert bytes(p) == bytes(q)
    assert _lib.lib().glim_amd_vgicp_align_default_params(None) == INVALID


def test_argument_errors_without_a_device():
    from glim_amd import _lib, api

    L = _lib.lib()
    out = (_lib.AlignResult * 2)()
    trace = (_lib.AlignTraceEntry * 64)()
    null2 = (C.c_void_p * 2)(None, None)
    T = np.tile(np.eye(4)[:3].reshape(-1), 2)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    fn = L.glim_amd_vgicp_align_batch
    assert fn(null2, null2, dp(T), 0, 0, None, out) == 0  # an empty batch
    assert fn(None, None, None, 0, 0, None, None) == 0
    assert fn(null2, null2, dp(T), 0, -1, None, out) == INVALID
    assert fn(null2, null2, dp(T), 0, 2, None, out) == INVALID  # null handles
    assert fn(None, null2, dp(T), 0, 2, None, out) == INVALID
    assert fn(null2, None, dp(T), 0, 2, None, out) == INVALID
    assert fn(null2, null2, None, 0, 2, None, out) == INVALID
    assert fn(null2, null2, dp(T), 0, 2, None, None) == INVALID
    for flags in (api.FACTOR_BINARY, api.FACTOR_BINARY | api.FACTOR_SURFACE_VALIDATION, 4):
        assert fn(null2, null2, dp(T), flags, 2, None, out) == INVALID
    for field, value in (("lambda_factor", 1.0), ("lambda_initial", float("nan")), ("lambda_initial", -1.0), ("error_scale", 0.0), ("max_iterations", -1),
                         ("max_trials", -1), ("max_trials", 4097), ("max_iterations", 4097), ("lambda_upper_bound", float("inf"))):
        bad = _lib.LMParams()
        L.glim_amd_vgicp_align_default_params(C.byref(bad))
        setattr(bad, field, value)
        assert fn(null2, null2, dp(T), 0, 2, C.byref(bad), out) == INVALID, field
    tr = L.glim_amd_debug_vgicp_align_trace
    assert tr(null2, null2, dp(T), 0, 2, None, out, trace) == INVALID
    assert tr(null2, null2, dp(T), 0, -1, None, out, trace) == INVALID
    assert tr(null2, null2, dp(T), api.FACTOR_BINARY, 2, None, out, trace) == INVALID
    assert tr(null2, null2, dp(T), 0, 2, None, out, None) == INVALID
    assert tr(null2, null2, dp(T), 0, 0, None, out, None) == 0
    assert api.vgicp_align_batch([], [], []) == []


def test_cpp_mirror_compiles_links_and_answers_without_a_device(tmp_path):
    """include/glim_amd/vgicp_align.hpp over the wrappers of gtsam_points_compat.hpp: compiled, linked, and run without a case (the defaults and
    an empty batch: no device call)"""
    out = subprocess.run([build_cpp(tmp_path, "vgicp_align")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "test_vgicp_align OK (no case given: nothing run)" in out.stdout, out.stdout + out.stderr
