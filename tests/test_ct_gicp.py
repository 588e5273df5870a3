"""Continuous-time GICP factor: gtsam_points::IntegratedCT_GICPFactor_<PointCloud, PointCloud> as GLIM's LiDAR-only CT odometry builds it
(odometry_estimation_ct.cpp:158-183), against the FP64 NumPy restatement of tests/ct_restatement.py (the per-bucket GICP terms are the committed
oracle's, orc.gicp_linearize): CPU pins of the restatement, HIP parity on the GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ct_restatement import (POSE_TOL, _check_record, _prior, _source, _target, adjoint, ct_poses, expmap, expmap_derivative, frozen_error, full_system,
                            hat, logmap, moving_source, np_ct_linearize, static_map, sweep_poses, time_table)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- CPU: the restatement --------------------------------------------------------------------------------------------------------------


def test_bucket_pose_derivatives_match_finite_differences():
    T0, T1 = sweep_poses()
    X = T0 @ expmap([0.01, -0.02, 0.03, 0.1, -0.05, 0.02])
    Y = T1 @ expmap([-0.02, 0.01, 0.05, -0.03, 0.08, 0.01])
    table = np.array([0.0, 0.013, 0.37, 0.5, 0.91, 1.0])
    T, D0, D1 = ct_poses(table, X, Y)
    eps = 1e-6
    for k in range(len(table)):
        for which, D in ((0, D0), (1, D1)):
            num = np.zeros((6, 6))
            for j in range(6):
                d = np.zeros(6)
                d[j] = eps
                Xp, Yp = (X @ expmap(d), Y) if which == 0 else (X, Y @ expmap(d))
                Xm, Ym = (X @ expmap(-d), Y) if which == 0 else (X, Y @ expmap(-d))
                Tp = ct_poses(table[k : k + 1], Xp, Yp)[0][0]
                Tm = ct_poses(table[k : k + 1], Xm, Ym)[0][0]
                num[:, j] = (logmap(np.linalg.inv(T[k]) @ Tp) - logmap(np.linalg.inv(T[k]) @ Tm)) / (2 * eps)
            np.testing.assert_allclose(D[k], num, atol=2e-8)
    # endpoints: T_0 = X with D0 = I, D1 = 0; T_last = Y
    np.testing.assert_allclose(T[0], X, atol=1e-15)
    np.testing.assert_allclose(D0[0], np.eye(6), atol=1e-15)
    assert not np.any(D1[0])
    np.testing.assert_allclose(T[-1], Y, atol=1e-12)


def test_time_table_semantics():
    t = np.array([0.0, 0.0004, 0.0011, 0.0012, 0.0005, 0.003, 0.0029, 0.05])
    table, idx = time_table(t)
    # 0.0004 joins bucket 0; 0.0011 opens one; 0.0012 joins; 0.0005 (back in time) joins; 0.003 opens; 0.0029 joins; 0.05 opens
    np.testing.assert_array_equal(idx, [0, 0, 1, 1, 1, 2, 2, 3])
    np.testing.assert_allclose(table, np.array([0.0, 0.0011, 0.003, 0.05]) / 0.05)
    table, idx = time_table(np.zeros(5))
    np.testing.assert_array_equal(table, [0.0])
    assert not idx.any()


@pytest.fixture(scope="module")
def cpu_case(orc):
    """a small moving-sensor scan (16 x 256) against the static map (16 x 512 x 2) with oracle covariances"""
    tp = static_map(16, 512)
    sp, times = moving_source(16, 256)
    _, tc = orc.covariances(tp, orc.knn(tp, 10))
    _, sc = orc.covariances(sp, orc.knn(sp, 10))
    T0, T1 = sweep_poses()
    return tp, tc, sp, sc, times, T0, T1


def test_restatement_gradient_and_hessian_match_numeric_derivatives(orc, cpu_case):
    tp, tc, sp, sc, times, T0, T1 = cpu_case
    X = T0 @ expmap([0.002, -0.001, 0.003, 0.02, -0.01, 0.01])
    Y = T1 @ expmap([-0.001, 0.002, -0.002, 0.01, 0.02, -0.01])
    L = np_ct_linearize(orc, tp, tc, sp, sc, times, X, Y, 1.0)
    assert L["num_inliers"] > 0.9 * len(sp)
    corr = L["corr"]
    sub = np.zeros_like(corr) - 1
    sub[::23] = corr[::23]
    # b: d/dxi of the frozen cost == 2 b (the oracle's convention: e = r^T M r without 1/2)
    eps = 1e-6
    g = np.zeros(12)
    for j in range(12):
        d = np.zeros(6)
        d[j % 6] = eps
        if j < 6:
            ep = frozen_error(tp, tc, sp, sc, times, sub, X, Y, X @ expmap(d), Y)
            em = frozen_error(tp, tc, sp, sc, times, sub, X, Y, X @ expmap(-d), Y)
        else:
            ep = frozen_error(tp, tc, sp, sc, times, sub, X, Y, X, Y @ expmap(d))
            em = frozen_error(tp, tc, sp, sc, times, sub, X, Y, X, Y @ expmap(-d))
        g[j] = (ep - em) / (2 * eps)
    # the restatement restricted to the same subset of points
    table, idx = time_table(times)
    T, D0, D1 = ct_poses(table, X, Y)
    Hn = np.zeros((12, 12))
    b_sub = np.zeros(12)
    H_sub = np.zeros((12, 12))
    for i in np.flatnonzero(sub >= 0):
        k, jj = idx[i], sub[i]
        R = T[k][:3, :3]
        M = np.linalg.inv(tc[jj] + R @ sc[i] @ R.T)

        def resid(Xv, Yv):
            Tk = ct_poses(table[k : k + 1], Xv, Yv)[0][0]
            return Tk[:3, :3] @ sp[i] + Tk[:3, 3] - tp[jj]

        J = np.zeros((3, 12))
        for j in range(12):
            d = np.zeros(6)
            d[j % 6] = 1e-6
            if j < 6:
                J[:, j] = (resid(X @ expmap(d), Y) - resid(X @ expmap(-d), Y)) / 2e-6
            else:
                J[:, j] = (resid(X, Y @ expmap(d)) - resid(X, Y @ expmap(-d))) / 2e-6
        Hn += J.T @ M @ J
        # the analytic per-point terms of the restatement: J = [-R hat(p) | R] [D0 | D1]
        Jp = np.hstack([-R @ hat(sp[i]), R]) @ np.hstack([D0[k], D1[k]])
        r = resid(X, Y)
        H_sub += Jp.T @ M @ Jp
        b_sub += Jp.T @ M @ r
    np.testing.assert_allclose(g, 2 * b_sub, rtol=1e-5, atol=1e-6 * np.abs(b_sub).max())
    np.testing.assert_allclose(Hn, H_sub, rtol=0, atol=1e-6 * np.abs(H_sub).max())


def test_restatement_with_equal_poses_is_the_rigid_factor(orc, cpu_case):
    tp, tc, sp, sc, times, T0, T1 = cpu_case
    X = T0 @ expmap([0.0, 0.0, 0.02, 0.3, 0.1, 0.0])
    L = np_ct_linearize(orc, tp, tc, sp, sc, times, X, X, 1.0)
    R = orc.gicp_linearize(tp, tc, sp, sc, X, 1.0)
    scale = np.abs(R["H_ss"]).max()
    np.testing.assert_allclose(L["H_00"] + L["H_01"] + L["H_01"].T + L["H_11"], R["H_ss"], rtol=0, atol=1e-9 * scale)
    np.testing.assert_allclose(L["b_0"] + L["b_1"], R["b_s"], rtol=0, atol=1e-9 * np.abs(R["b_s"]).max())
    assert L["num_inliers"] == R["num_inliers"] and abs(L["error"] - R["error"]) <= 1e-9 * R["error"]
    # all times equal: one bucket at t = 0, the end pose carries no information
    L1 = np_ct_linearize(orc, tp, tc, sp, sc, np.zeros(len(sp)), X, T1, 1.0)
    assert not np.any(L1["H_11"]) and not np.any(L1["H_01"]) and not np.any(L1["b_1"])
    R1 = orc.gicp_linearize(tp, tc, sp, sc, X, 1.0)
    np.testing.assert_allclose(L1["H_00"], R1["H_ss"], rtol=0, atol=1e-12 * scale)


def test_ct_symbols_are_exported_and_check_their_arguments_without_a_device():
    from glim_amd import _lib

    L = _lib.lib()
    names = [n for n in _lib.SYMBOLS if "ct_gicp" in n]
    assert len(names) == 9
    header = open(os.path.join(ROOT, "include", "glim_amd.h")).read()
    for n in names:
        assert hasattr(L, n), n
        assert n in header or n.startswith("glim_amd_debug_"), n
    assert "glim_amd_ct_gicp_factor" in header and "glim_amd_ct_linearized" in header
    X = np.eye(4)[:3].reshape(12).copy()
    dp = X.ctypes.data_as(C.POINTER(C.c_double))
    rec = _lib.CtLinearized()
    e, n = C.c_double(), C.c_int64()
    h = C.c_void_p()
    assert C.sizeof(rec) == 8 + 8 + 3 * 36 * 8 + 12 * 8
    assert L.glim_amd_ct_gicp_create(None, None, None, C.byref(h)) == -1
    assert L.glim_amd_ct_gicp_create(None, None, None, None) == -1
    assert L.glim_amd_ct_gicp_destroy(None) == 0
    assert L.glim_amd_ct_gicp_set_max_correspondence_distance(None, 1.0) == -1
    assert L.glim_amd_ct_gicp_linearize(None, dp, dp, C.byref(rec)) == -1
    assert L.glim_amd_ct_gicp_error(None, dp, dp, C.byref(e), C.byref(n)) == -1
    assert L.glim_amd_ct_gicp_correspondences(None, dp, dp, None) == -1
    assert L.glim_amd_ct_gicp_deskewed_points(None, dp, dp, 0, dp) == -1
    assert L.glim_amd_ct_gicp_deskewed_cloud(None, dp, dp, 1, C.byref(h)) == -1
    assert L.glim_amd_debug_ct_gicp_poses(None, dp, dp, None, 0, None, None, None, None, None) == -1
    # the C++ mirror and the gtsam adapter name the new entry points
    compat = open(os.path.join(ROOT, "include", "glim_amd", "gtsam_points_compat.hpp")).read()
    assert re.search(r"class IntegratedCT_GICPFactor\b", compat) and re.search(r"glim_amd_ct_gicp_linearize\s*\(", compat)
    adapter = open(os.path.join(ROOT, "adapters", "gtsam", "glim_amd_gtsam.hpp")).read()
    assert re.search(r"class IntegratedCT_GICPFactorHIP : public gtsam::NonlinearFactor", adapter)


# ---- GPU: the device factor against the restatement ----------------------------------------------------------------------------------



@pytest.fixture(scope="module")
def gpu_ctx():
    from glim_amd import api

    return api.Context(0, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["pre10k", "raw131k"])
def test_ct_factor_matches_the_restatement_on_a_moving_scan(orc, gpu_ctx, kind):
    from glim_amd import api

    ctx = gpu_ctx
    tp, tc, tg = _target(api, ctx, 64, 1024)
    sp, sc, times, pass_times, sg = _source(api, ctx, kind)
    assert (kind == "pre10k" and 8000 < len(sp) < 14000) or len(sp) == 131072
    T0, T1 = sweep_poses()
    X = T0 @ expmap([0.002, -0.001, 0.003, 0.03, -0.02, 0.01])
    Y = T1 @ expmap([-0.001, 0.002, -0.002, 0.02, 0.03, -0.01])
    values = {0: X, 1: Y}
    f = api.IntegratedCT_GICPFactor(0, 1, tg, sg, max_correspondence_distance=1.0, times=pass_times)
    tab, T, D0, D1, idx = f.debug_poses(values)
    table, idx_ref = time_table(times)
    assert 80 <= len(table) <= 120
    np.testing.assert_array_equal(idx, idx_ref)
    np.testing.assert_allclose(tab, table, rtol=0, atol=1e-15)
    Tr, D0r, D1r = ct_poses(table, X, Y)
    for a, b in ((T, Tr), (D0, D0r), (D1, D1r)):
        assert np.abs(a - b).max() < 1e-12
    got = f.linearize(values)
    ref = np_ct_linearize(orc, tp, tc, sp, sc, times, X, Y, 1.0, poses=(T, D0, D1))
    np.testing.assert_array_equal(f.correspondences(values), ref["corr"])
    _check_record(got, ref)
    # error(): the correspondences and M of the last linearize, at other values
    moved = {0: X @ expmap([0.001, 0.0, -0.001, 0.01, 0.0, 0.01]), 1: Y @ expmap([0.0, 0.002, 0.0, -0.01, 0.02, 0.0])}
    e, n = f.error(moved, with_inliers=True)
    sub = ref["corr"].copy()
    if kind == "raw131k":  # (the restatement's per-point loop on a tenth of the points: the kept state is per point)
        sub[np.arange(len(sub)) % 10 != 0] = -1
        assert n == ref["num_inliers"] and e > 0
    else:
        np.testing.assert_allclose(e, frozen_error(tp, tc, sp, sc, times, sub, X, Y, moved[0], moved[1]), rtol=2e-4)
        assert n == ref["num_inliers"]
    # error() at the linearisation point is the linearised error
    np.testing.assert_allclose(f.error(values), got["error"], rtol=2e-5)
    # a fresh factor: error() with no linearize computes the correspondences first
    g = api.IntegratedCT_GICPFactor(0, 1, tg, sg, target_tree=f.target_tree, times=pass_times)
    ref_m = np_ct_linearize(orc, tp, tc, sp, sc, times, moved[0], moved[1], 1.0, poses=g.debug_poses(moved)[1:4])
    np.testing.assert_allclose(g.error(moved), ref_m["error"], rtol=2e-4)
    # two identical calls give identical bits
    a, b = f.linearize(values), f.linearize(values)
    for k in ("H_00", "H_01", "H_11", "b_0", "b_1"):
        np.testing.assert_array_equal(a[k], b[k])
    assert a["error"] == b["error"]
    g.close()
    f.close()


@pytest.mark.gpu
def test_ct_factor_with_equal_poses_sums_to_the_rigid_factor(orc, gpu_ctx):
    from glim_amd import api

    ctx = gpu_ctx
    tp, tc, tg = _target(api, ctx, 32, 1024)
    sp, sc, times, pass_times, sg = _source(api, ctx, "pre10k")
    T0, _ = sweep_poses()
    f = api.IntegratedCT_GICPFactor(0, 1, tg, sg)
    L = f.linearize({0: T0, 1: T0})
    R = api.IntegratedGICPFactor(np.eye(4), 1, tg, sg, target_tree=f.target_tree).linearize({1: T0})
    scale = np.abs(R["H_ss"]).max()
    np.testing.assert_allclose(L["H_00"] + L["H_01"] + L["H_01"].T + L["H_11"], R["H_ss"], rtol=0, atol=2e-4 * scale)
    np.testing.assert_allclose(L["b_0"] + L["b_1"], R["b_s"], rtol=0, atol=2e-4 * np.abs(R["b_s"]).max() + 1e-6 * scale)
    assert L["num_inliers"] == R["num_inliers"]
    np.testing.assert_allclose(L["error"], R["error"], rtol=2e-4)
    f.close()


def _lm_system(L, X, Y, X_pred, delta_pred):
    """the CT factor + PriorFactor(X, 1e-3) + BetweenFactor(X, Y, 1e3) as one 12-dof system (odometry_estimation_ct.cpp:158-183)"""
    H, b = full_system(L)
    H, b = H.copy(), b.copy()
    Hp, bp, _ = _prior(X, X_pred, 1e-3)
    H[:6, :6] += Hp
    b[:6] += bp
    # between: r = Log(delta_pred^-1 X^-1 Y); d r / d X = -J_r^-1(r) Ad((X^-1 Y)^-1), d r / d Y = J_r^-1(r)
    r = logmap(np.linalg.inv(delta_pred) @ np.linalg.inv(X) @ Y)
    Jinv = np.linalg.inv(expmap_derivative(r))
    J = np.hstack([-Jinv @ adjoint(np.linalg.inv(np.linalg.inv(X) @ Y)), Jinv])
    H += 1e3 * J.T @ J
    b += 1e3 * J.T @ r
    return H, b


def _lm_cost(e_ct, X, Y, X_pred, delta_pred):
    r = logmap(np.linalg.inv(delta_pred) @ np.linalg.inv(X) @ Y)
    return e_ct + _prior(X, X_pred, 1e-3)[2] + 1e3 * r @ r


@pytest.mark.gpu
def test_ct_lm_frame_recovers_begin_and_end_poses(orc, gpu_ctx):
    from glim_amd import api

    ctx = gpu_ctx
    tp, tc, tg = _target(api, ctx, 32, 1024)
    sp, sc, times, pass_times, sg = _source(api, ctx, "pre10k")
    T0, T1 = sweep_poses()
    # constant-velocity prediction from a previous frame that moved 30 % slower
    X_pred = T0 @ expmap([0.0, 0.0, 0.004, 0.03, -0.02, 0.0])
    delta_true = np.linalg.inv(T0) @ T1
    delta_pred = expmap(0.7 * logmap(delta_true))
    X, Y = X_pred.copy(), X_pred @ delta_pred
    f = api.IntegratedCT_GICPFactor(0, 1, tg, sg, max_correspondence_distance=1.0)
    lam = 1e-10
    for it in range(8):
        values = {0: X, 1: Y}
        L = f.linearize(values)
        ref = np_ct_linearize(orc, tp, tc, sp, sc, times, X, Y, 1.0, poses=f.debug_poses(values)[1:4])
        H, b = _lm_system(L, X, Y, X_pred, delta_pred)
        Hr, br = _lm_system(ref, X, Y, X_pred, delta_pred)
        cost0 = _lm_cost(L["error"], X, Y, X_pred, delta_pred)
        while True:
            dx = np.linalg.solve(H + lam * np.eye(12), -b)
            dr = np.linalg.solve(Hr + lam * np.eye(12), -br)
            assert np.abs(dx - dr).max() < POSE_TOL, (it, np.abs(dx - dr).max())
            Xn, Yn = X @ expmap(dx[:6]), Y @ expmap(dx[6:])
            if _lm_cost(f.error({0: Xn, 1: Yn}), Xn, Yn, X_pred, delta_pred) <= cost0 or lam > 1e5:
                lam = max(lam / 10.0, 1e-10)
                break
            lam *= 10.0
        X, Y = Xn, Yn
        if np.abs(dx).max() < 1e-6:
            break

    def miss(A, B):
        E = np.linalg.inv(B) @ A
        return np.linalg.norm(E[:3, 3]), np.degrees(np.linalg.norm(logmap(E)[:3]))

    for est, truth in ((X, T0), (Y, T1)):
        dt, dr = miss(est, truth)
        assert dt < 0.02 and dr < 0.2, (dt, dr)
    # a rigid GICP alignment of the same (skewed) scan, from the same prediction, misses the end pose by much more
    rig = api.IntegratedGICPFactor(np.eye(4), 1, tg, sg, target_tree=f.target_tree, max_correspondence_distance=1.0)
    T = X_pred.copy()
    for _ in range(10):
        Lr = rig.linearize({1: T})
        T = T @ expmap(np.linalg.solve(Lr["H_ss"] + 1e-6 * np.trace(Lr["H_ss"]) / 6 * np.eye(6), -Lr["b_s"]))
    assert miss(T, T1)[0] > 5 * max(miss(Y, T1)[0], 0.01)
    rig.close()
    f.close()


@pytest.mark.gpu
def test_ct_deskewed_points_and_cloud(orc, gpu_ctx):
    from glim_amd import api

    ctx = gpu_ctx
    _, _, tg = _target(api, ctx, 16, 512)
    _, _, times, _, sg = _source(api, ctx, "pre10k")
    p64 = sg.download_points64()
    T0, T1 = sweep_poses()
    values = {0: T0, 1: T1}
    f = api.IntegratedCT_GICPFactor(0, 1, tg, sg)
    table, idx = time_table(times)
    T, _, _ = ct_poses(table, T0, T1)
    world = np.einsum("nij,nj->ni", T[idx][:, :3, :3], p64) + T[idx][:, :3, 3]
    local = np.einsum("ij,nj->ni", np.linalg.inv(T[0])[:3, :3], world) + np.linalg.inv(T[0])[:3, 3]
    assert np.abs(f.deskewed_source_points(values) - world).max() < 1e-9
    assert np.abs(f.deskewed_source_points(values, local=True) - local).max() < 1e-9
    assert np.abs(local - world).max() > 1.0  # `local` is honoured
    d = f.deskewed_cloud(values, local=True)
    assert d.size() == sg.size()
    q = d.download_points64()
    assert np.abs(q - local).max() < 1e-9
    d.estimate_covariances(10)
    _, c, _ = d.download(covs=True, normals=False)
    nb = sg.download_frame()["neighbors"]
    _, cref = orc.covariances(q, nb)
    assert np.abs(c.astype(np.float64) - cref).max() < 1e-5
    d.close()
    f.close()


@pytest.mark.gpu
def test_ct_factor_edge_cases(orc, gpu_ctx):
    from glim_amd import api

    ctx = gpu_ctx
    tp, tc, tg = _target(api, ctx, 16, 512)
    p, t = moving_source(16, 256)
    T0, T1 = sweep_poses()
    values = {0: T0, 1: T1}

    def cloud(pts):
        g = api.PointCloudGPU.clone(pts, ctx=ctx)
        g.find_neighbors(10, download=False)
        g.estimate_covariances(10)
        xyz, c, _ = g.download(covs=True, normals=False)
        return xyz.astype(np.float64), c.astype(np.float64), g

    # empty source / empty target
    empty = api.PointCloudGPU.clone(np.zeros((0, 3)), covs=np.zeros((0, 3, 3)), ctx=ctx)
    f = api.IntegratedCT_GICPFactor(0, 1, tg, empty, times=np.zeros(0))
    L = f.linearize(values)
    assert L["num_inliers"] == 0 and L["error"] == 0.0 and not np.any(full_system(L)[0])
    assert f.error(values) == 0.0 and f.deskewed_source_points(values).shape == (0, 3)
    f.close()
    sp, sc, sg = cloud(p[:1000])
    f = api.IntegratedCT_GICPFactor(0, 1, empty, sg, times=t[:1000])
    assert f.linearize(values)["num_inliers"] == 0 and np.all(f.correspondences(values) == -1)
    f.close()
    # a source without covariances, without times; a radius beyond the index
    bare = api.PointCloudGPU.clone(p[:1000], ctx=ctx)
    for kw, src in ((dict(times=t[:1000]), bare), (dict(), sg)):
        with pytest.raises(api.GlimAmdError) as ei:
            api.IntegratedCT_GICPFactor(0, 1, tg, src, **kw)
        assert ei.value.code == -5
    f = api.IntegratedCT_GICPFactor(0, 1, tg, sg, times=t[:1000])
    with pytest.raises(api.GlimAmdError) as ei:
        f.set_max_correspondence_distance(100.0)
    assert ei.value.code == -6 and f.max_correspondence_distance == 1.0
    # the context refuses to go while the factor lives
    from glim_amd._lib import lib

    assert lib().glim_amd_ctx_destroy(ctx._h) == -5
    f.close()
    # one bucket (all times equal); one point per bucket with n not a multiple of 256; non-ascending times
    rng = np.random.default_rng(3)
    n = 1000
    sp, sc, sg = cloud(p[:n])
    X = T0 @ expmap([0.001, 0.0, 0.002, 0.02, 0.01, 0.0])
    Y = T1 @ expmap([0.0, -0.001, 0.0, 0.0, 0.02, -0.01])
    cases = [("one bucket", np.zeros(n), n), ("one point per bucket", np.arange(n) * 0.002, 301),
             ("non-ascending", t[:n][rng.permutation(n)], n)]
    for name, times, m in cases:
        sub_p, sub_c, g = (sp, sc, sg) if m == n else cloud(p[:m])
        tt = times[:m]
        f = api.IntegratedCT_GICPFactor(0, 1, tg, g, times=tt)
        vals = {0: X, 1: Y}
        tab, T, D0, D1, idx = f.debug_poses(vals)
        assert len(tab) == len(time_table(tt)[0]), name
        if name == "one point per bucket":
            assert len(tab) == m
        got = f.linearize(vals)
        ref = np_ct_linearize(orc, tp, tc, sub_p, sub_c, tt, X, Y, 1.0, poses=(T, D0, D1))
        np.testing.assert_array_equal(f.correspondences(vals), ref["corr"])
        _check_record(got, ref)
        if name == "one bucket":
            assert not np.any(got["H_11"]) and not np.any(got["H_01"]) and not np.any(got["b_1"])
        again = f.linearize(vals)
        for k in ("H_00", "H_01", "H_11", "b_0", "b_1"):
            np.testing.assert_array_equal(got[k], again[k])
        f.close()
