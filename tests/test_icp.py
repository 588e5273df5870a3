"""The ICP factors and the ICP fine registration (include/glim_amd.h "ICP factors", "ICP fine registration"), the part that needs no device: the
NumPy restatement (tests/icp_restatement.py) pinned against the oracle's GICP factor with M = I, its gradient, the two special cases that pin the
elementwise reading of point-to-plane, the ABI surface and the C++ mirrors."""
import ctypes as C
import os
import subprocess

import numpy as np

import icp_restatement as icpr
import lm_restatement as lmr
from align_cases import ROOT, build_cpp, check_symbols

NEW_STABLE = ["glim_amd_icp_linearize", "glim_amd_icp_error", "glim_amd_icp_align_default_params", "glim_amd_icp_align_batch"]
NEW_DIAG = ["glim_amd_debug_icp_align_trace"]
PERTURBATION = [0.01, -0.02, 0.005, 0.05, 0.02, -0.01]


def build_drop_in(tmp_path):
    """tests/cpp/test_icp_drop_in.cpp over the drop-in include tree and the stand-in third-party headers, as tests/test_glim_module.py builds
    its programs (the stand-ins are not warning-clean: -w)"""
    exe = str(tmp_path / "test_icp_drop_in")
    inc = [os.path.join(ROOT, "adapters", "gtsam_points_hip"), os.path.join(ROOT, "adapters", "gtsam"), os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "glim_standin")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-w"] + ["-I" + d for d in inc] + [os.path.join(ROOT, "tests", "cpp", "test_icp_drop_in.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "glim_amd"), "-lglim_amd", "-Wl,-rpath," + os.path.join(ROOT, "glim_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-L/opt/rocm/lib", "-lamdhip64"])
    return exe


def test_point_to_point_restatement_is_the_oracle_gicp_factor_with_identity_metric(orc, small_pair):
    """target covariances I and source covariances 0 make M = (C_B + R C_A R^T)^-1 = I: the oracle's GICP factor is then point-to-point ICP"""
    t, s = small_pair["target"], small_pair["source"]
    tp, sp = np.asarray(t["points"], dtype=np.float64), np.asarray(s["points"], dtype=np.float64)
    eye, zero = np.tile(np.eye(3), (len(tp), 1, 1)), np.zeros((len(sp), 3, 3))
    T = small_pair["delta"] @ orc.se3_exp(PERTURBATION)
    for max_d in (1.0, 0.3):
        ref = orc.gicp_linearize(tp, eye, sp, zero, T, max_d, want_corr=True)
        got = icpr.icp_linearize(tp, sp, T, max_d)
        np.testing.assert_array_equal(got["corr"], ref["corr"])
        assert got["num_inliers"] == ref["num_inliers"] > 1000
        np.testing.assert_allclose(got["H_ss"], ref["H_ss"], rtol=1e-9, atol=1e-9 * np.abs(ref["H_ss"]).max())
        np.testing.assert_allclose(got["b_s"], ref["b_s"], rtol=1e-9, atol=1e-9 * np.abs(ref["b_s"]).max())
        np.testing.assert_allclose(got["error"], ref["error"], rtol=1e-10)


def test_finite_difference_gradient_of_both_metrics(orc, small_pair):
    """d/dxi of the error with the correspondences frozen == 2 b_s (the error carries no 1/2)"""
    t, s = small_pair["target"], small_pair["source"]
    tp, sp = np.asarray(t["points"], dtype=np.float64), np.asarray(s["points"], dtype=np.float64)[::7]
    T = small_pair["delta"] @ orc.se3_exp([0.004, -0.003, 0.002, 0.02, 0.01, -0.01])
    for normals in (None, t["normals"]):
        L = icpr.icp_linearize(tp, sp, T, 0.7, normals=normals)
        assert L["num_inliers"] > 100
        cost = lambda Tp: icpr.icp_linearize(tp, sp, Tp, 0.7, normals=normals, corr=L["corr"])["error"]
        g, eps = np.zeros(6), 1e-6
        for k in range(6):
            d = np.zeros(6)
            d[k] = eps
            g[k] = (cost(T @ orc.se3_exp(d)) - cost(T @ orc.se3_exp(-d))) / (2 * eps)
        np.testing.assert_allclose(g, 2.0 * L["b_s"], rtol=1e-5, atol=1e-6 * np.abs(L["b_s"]).max())


def test_point_to_plane_special_cases(orc, small_pair):
    t, s = small_pair["target"], small_pair["source"]
    tp, sp = np.asarray(t["points"], dtype=np.float64), np.asarray(s["points"], dtype=np.float64)
    T = small_pair["delta"] @ orc.se3_exp(PERTURBATION)
    q = icpr.transform(sp, T)
    point = icpr.icp_linearize(tp, sp, T, 1.0, q=q)
    # every normal (0, 0, 1): only r_z counts, and no x / y translation is observed
    up = icpr.icp_linearize(tp, sp, T, 1.0, normals=np.tile([0.0, 0.0, 1.0], (len(tp), 1)), q=q)
    ok = point["corr"] >= 0
    rz = (tp[point["corr"][ok]] - q[ok])[:, 2]
    np.testing.assert_array_equal(up["corr"], point["corr"])
    np.testing.assert_allclose(up["error"], np.sum(rz * rz), rtol=1e-12)
    Rt = T[:3, :3].T  # the translation columns are -R: "x / y translation of the target frame" is v = R^T e_x, R^T e_y in the source tangent
    for axis in (0, 1):
        v = np.concatenate([np.zeros(3), Rt[:, axis]])
        assert np.abs(up["H_ss"] @ v).max() <= 1e-12 * np.abs(up["H_ss"]).max() and abs(up["b_s"] @ v) <= 1e-12 * np.abs(up["b_s"]).max()
    # every normal (1, 1, 1): the elementwise weights are all 1 -- exactly the point-to-point record (n n^T would not give it)
    ones = icpr.icp_linearize(tp, sp, T, 1.0, normals=np.ones((len(tp), 3)), q=q)
    for k in ("H_ss", "b_s", "error", "num_inliers", "corr"):
        assert np.array_equal(ones[k], point[k]), k


def test_symbols_and_cpp_mirrors(tmp_path):
    """the new entry points are declared once, listed and resolved; icp_align.hpp knows nothing of the diagnostic header; programs over the C++
    mirror and over the drop-in header compile, link and run their no-device part"""
    from glim_amd import _lib, api

    mirror = check_symbols(NEW_STABLE, NEW_DIAG, "icp_align.hpp")
    for name in ("glim_amd_icp_linearize", "glim_amd_icp_error", "glim_amd_icp_align_batch", "glim_amd_icp_align_default_params"):
        assert name in mirror
    assert api.ICP_POINT_TO_PLANE == 0x4 and not api.ICP_POINT_TO_PLANE & (api.FACTOR_BINARY | api.FACTOR_SURFACE_VALIDATION)
    L = _lib.lib()
    p = _lib.LMParams()
    assert L.glim_amd_icp_align_default_params(C.byref(p)) == 0 and L.glim_amd_icp_align_default_params(None) == -1
    want = dict(lmr.DEFAULTS, max_iterations=200)
    assert {k: getattr(p, k) for k, _ in _lib.LMParams._fields_} == want
    q = api.icp_align_params()
    assert {k: getattr(q, k) for k in want} == want and q.resolved_max_trials() == 400
    # refusals that need no device
    out, trace = (_lib.AlignResult * 2)(), (_lib.AlignTraceEntry * 8)()
    null2 = (C.c_void_p * 2)(None, None)
    T, d = np.tile(np.eye(4)[:3].reshape(-1), 2), np.array([1.0, 1.0])
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    fn = L.glim_amd_icp_align_batch
    assert fn(null2, null2, dp(T), dp(d), 0, 0, None, out) == 0 and fn(None, None, None, None, api.ICP_POINT_TO_PLANE, 0, None, None) == 0
    assert fn(null2, null2, dp(T), dp(d), 0, -1, None, out) == -1
    assert fn(null2, null2, dp(T), dp(d), 0, 2, None, out) == -1  # null handles
    assert fn(null2, null2, dp(T), dp(d), api.FACTOR_BINARY, 0, None, out) == -1 and fn(null2, null2, dp(T), dp(d), 0x8, 0, None, out) == -1
    assert fn(null2, null2, dp(T), dp(np.array([1.0, np.nan])), 0, 2, None, out) == -1
    bad = _lib.LMParams()
    L.glim_amd_icp_align_default_params(C.byref(bad))
    bad.max_trials = 5000
    assert fn(null2, null2, dp(T), dp(d), 0, 2, C.byref(bad), out) == -1
    tr = L.glim_amd_debug_icp_align_trace
    assert tr(null2, null2, dp(T), dp(d), 0, 0, None, out, None, 0) == 0 and tr(null2, null2, dp(T), dp(d), 0, 2, None, out, None, 0) == -1
    assert tr(null2, null2, dp(T), dp(d), 0, 0, None, out, trace, -1) == -1 and tr(null2, null2, dp(T), dp(d), 0x1, 0, None, out, trace, 0) == -1
    Lin = _lib.Linearized6()
    assert L.glim_amd_icp_linearize(None, None, dp(T), 1.0, 0, C.byref(Lin)) == -1 and L.glim_amd_icp_linearize(None, None, dp(T), 1.0, 0x2, C.byref(Lin)) == -1
    for exe, tag in ((build_cpp(tmp_path, "icp_align"), "test_icp_align OK"), (build_drop_in(tmp_path), "test_icp_drop_in OK")):
        res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0 and tag in res.stdout, res.stdout + res.stderr
