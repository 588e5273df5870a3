"""GICP factor: gtsam_points::IntegratedGICPFactor as constructed at sub_mapping.cpp:202,
global_mapping.cpp:400, global_mapping_pose_graph.cpp:393.  Oracle pins on CPU, HIP parity on the GPU."""
import numpy as np
import pytest

from ct_restatement import gn_step

POSE_TOL = 1e-4  # BASELINE.json north_star: pose delta within 1e-4 m / 1e-4 rad per Gauss-Newton iteration


def np_gicp(tp, tc, sp, sc, T, max_d):
    """Independent restatement: scipy kd-tree correspondences, dense J^T M J accumulation."""
    from scipy.spatial import cKDTree

    R, t = T[:3, :3], T[:3, 3]
    q = sp @ R.T + t
    d, j = cKDTree(tp).query(q, k=1)
    ok = d <= max_d
    H, b, e = np.zeros((6, 6)), np.zeros(6), 0.0

    def hat(v):
        return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])

    for i in np.flatnonzero(ok):
        M = np.linalg.inv(tc[j[i]] + R @ sc[i] @ R.T)
        r = tp[j[i]] - q[i]
        Js = np.hstack([R @ hat(sp[i]), -R])
        H += Js.T @ M @ Js
        b += Js.T @ M @ r
        e += r @ M @ r
    return dict(H_ss=H, b_s=b, error=e, num_inliers=int(ok.sum()), corr=np.where(ok, j, -1))


def test_oracle_gicp_matches_numpy_restatement(orc, small_pair):
    t, s = small_pair["target"], small_pair["source"]
    T = small_pair["delta"] @ orc.se3_exp([0.01, -0.02, 0.005, 0.05, 0.02, -0.01])
    for max_d in (1.0, 0.3):
        ref = np_gicp(t["points"], t["covs"], s["points"], s["covs"], T, max_d)
        got = orc.gicp_linearize(t["points"], t["covs"], s["points"], s["covs"], T, max_d, want_corr=True)
        assert got["num_inliers"] == ref["num_inliers"] > 1000
        assert (got["corr"] != ref["corr"]).mean() < 1e-3  # kd-tree vs exact search may differ on exact ties only
        np.testing.assert_allclose(got["H_ss"], ref["H_ss"], rtol=1e-9, atol=1e-9 * np.abs(ref["H_ss"]).max())
        np.testing.assert_allclose(got["b_s"], ref["b_s"], rtol=1e-9, atol=1e-9 * np.abs(ref["b_s"]).max())
        np.testing.assert_allclose(got["error"], ref["error"], rtol=1e-10)
        e, n = orc.gicp_error(t["points"], t["covs"], s["points"], s["covs"], T, max_d)
        assert n == got["num_inliers"] and abs(e - got["error"]) <= 1e-12 * abs(e)
    # binary blocks obey the adjoint identity J_t = -J_s Ad(delta^-1), like the VGICP factor
    from glim_amd import api

    iu = np.triu_indices(6)
    compact = np.concatenate([[got["num_inliers"], got["error"]], got["H_ss"][iu], got["b_s"]])
    ex = api.expand_compact(compact, T, api.FACTOR_BINARY)
    for k in ("H_tt", "H_ts", "b_t"):
        np.testing.assert_allclose(ex[k], got[k], rtol=1e-9, atol=1e-6 * np.abs(got[k]).max())


def test_oracle_gicp_finite_difference_gradient(orc, small_pair):
    """d/dxi sum r^T M r with M and the correspondences frozen == 2 b_s."""
    t, s = small_pair["target"], small_pair["source"]
    sp, sc = s["points"][::7], s["covs"][::7]
    T = small_pair["delta"] @ orc.se3_exp([0.004, -0.003, 0.002, 0.02, 0.01, -0.01])
    L = orc.gicp_linearize(t["points"], t["covs"], sp, sc, T, 0.7, want_corr=True)
    corr = L["corr"]
    R = T[:3, :3]

    def frozen_cost(Tp):
        q = sp @ Tp[:3, :3].T + Tp[:3, 3]
        c = 0.0
        for i in np.flatnonzero(corr >= 0):
            M = np.linalg.inv(t["covs"][corr[i]] + R @ sc[i] @ R.T)
            r = t["points"][corr[i]] - q[i]
            c += r @ M @ r
        return c

    g = np.zeros(6)
    eps = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = eps
        g[k] = (frozen_cost(T @ orc.se3_exp(d)) - frozen_cost(T @ orc.se3_exp(-d))) / (2 * eps)
    np.testing.assert_allclose(g, 2.0 * L["b_s"], rtol=1e-5, atol=1e-6 * np.abs(L["b_s"]).max())


# ------------------------------------------------------------------------------------------------------------------


def clouds(orc, api, ctx, rings=48, az=512):
    from glim_amd import synth

    scene = synth.Scene.default()
    dirs = synth.lidar_directions(rings, az)
    poses = synth.arc_trajectory(2, step=0.6, yaw_step_deg=3.0)
    out = []
    for i, T in enumerate(poses):
        p = synth.scan(scene, T, dirs, frame_id=i).astype(np.float64)
        g = api.PointCloudGPU.clone(p, ctx=ctx)
        g.find_neighbors(10, download=False)
        g.estimate_covariances(10)
        _, c, _ = g.download(covs=True, normals=False)
        out.append((p, c.astype(np.float64), g))
    return out, np.linalg.inv(poses[0]) @ poses[1]


@pytest.mark.gpu
@pytest.mark.parametrize("max_d", [1.0, 0.5, 0.05])
def test_hip_gicp_matches_oracle(orc, max_d):
    """Correspondences bit-exact; H, b, error within the FP32-accumulation tolerance of the VGICP factor; GN step within 1e-4."""
    from glim_amd import api

    ctx = api.Context(0, 1)
    ((tp, tc, tg), (sp, sc, sg)), delta = clouds(orc, api, ctx)
    T = delta @ orc.se3_exp([0.004, -0.003, 0.002, 0.03, 0.02, -0.01])
    for binary in (False, True):
        f = api.IntegratedGICPFactor(0 if binary else np.eye(4), 1, tg, sg, max_correspondence_distance=max_d)
        values = {0: np.eye(4), 1: T}
        got = f.linearize(values)
        ref = orc.gicp_linearize(tp, tc, sp, sc, T, max_d, want_corr=True)
        np.testing.assert_array_equal(f.correspondences(values), ref["corr"])
        assert got["num_inliers"] == ref["num_inliers"] > 50
        scale = np.abs(ref["H_ss"]).max()
        np.testing.assert_allclose(got["error"], ref["error"], rtol=2e-4)
        np.testing.assert_allclose(got["H_ss"], ref["H_ss"], rtol=0, atol=2e-4 * scale)
        np.testing.assert_allclose(got["b_s"], ref["b_s"], rtol=0, atol=2e-4 * np.abs(ref["b_s"]).max() + 1e-6 * scale)
        if binary:
            for k in ("H_tt", "H_ts"):
                np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=2e-4 * np.abs(ref[k]).max())
            np.testing.assert_allclose(got["b_t"], ref["b_t"], rtol=0, atol=2e-4 * np.abs(ref["b_t"]).max() + 1e-6 * scale)
        else:
            assert not np.any(got["H_tt"]) and not np.any(got["H_ts"]) and not np.any(got["b_t"])
        lam = 1e-6 * np.trace(ref["H_ss"]) / 6
        assert np.abs(gn_step(got, lam) - gn_step(ref, lam)).max() < POSE_TOL
        e = f.error(values)
        assert abs(e - ref["error"]) <= 2e-4 * ref["error"]
        assert f.inlier_fraction() == ref["num_inliers"] / len(sp)
        f.close()


@pytest.mark.gpu
def test_hip_gicp_alignment_converges_like_the_oracle(orc):
    """global_mapping.cpp:400-420: a few Gauss-Newton / LM iterations of the factor from a perturbed pose; every iterate within 1e-4."""
    from glim_amd import api

    ctx = api.Context(0, 1)
    ((tp, tc, tg), (sp, sc, sg)), delta = clouds(orc, api, ctx, rings=32, az=384)
    f = api.IntegratedGICPFactor(np.eye(4), 1, tg, sg, max_correspondence_distance=0.5)
    T = delta @ orc.se3_exp([0.01, -0.01, 0.01, 0.08, -0.05, 0.03])
    for it in range(6):
        got = f.linearize({1: T})
        ref = orc.gicp_linearize(tp, tc, sp, sc, T, 0.5)
        assert got["num_inliers"] == ref["num_inliers"]
        lam = 1e-6 * np.trace(ref["H_ss"]) / 6
        dg, dr = gn_step(got, lam), gn_step(ref, lam)
        assert np.abs(dg - dr).max() < POSE_TOL
        T = T @ orc.se3_exp(dr)
    err = np.linalg.inv(delta) @ T
    assert np.linalg.norm(err[:3, 3]) < 0.02 and np.abs(err[:3, :3] - np.eye(3)).max() < 2e-3


@pytest.mark.gpu
def test_hip_gicp_edge_cases(orc):
    from glim_amd import api

    ctx = api.Context(0, 1)
    ((tp, tc, tg), (sp, sc, sg)), delta = clouds(orc, api, ctx, rings=16, az=128)
    # far away: no correspondences -> zero information, never NaN
    far = delta.copy()
    far[0, 3] += 1e3
    f = api.IntegratedGICPFactor(np.eye(4), 1, tg, sg)
    L = f.linearize({1: far})
    assert L["num_inliers"] == 0 and L["error"] == 0.0 and not np.any(L["H_ss"]) and not np.any(L["b_s"])
    assert np.all(f.correspondences({1: far}) == -1)
    # a pre-built index shared by two factors (global_mapping_pose_graph.cpp:393 passes candidate.target->tree)
    g = api.IntegratedGICPFactor(np.eye(4), 1, tg, sg, target_tree=f.target_tree, max_correspondence_distance=0.25)
    assert 0 < g.linearize({1: delta})["num_inliers"] <= f.linearize({1: delta})["num_inliers"]
    # empty source / empty target
    empty = api.PointCloudGPU.clone(np.zeros((0, 3)), covs=np.zeros((0, 3, 3)), ctx=ctx)
    assert api.IntegratedGICPFactor(np.eye(4), 1, tg, empty).linearize({1: delta})["num_inliers"] == 0
    assert api.IntegratedGICPFactor(np.eye(4), 1, empty, sg).linearize({1: delta})["num_inliers"] == 0
    # a source without covariances is a state error, not a crash
    bare = api.PointCloudGPU.clone(sp, ctx=ctx)
    with pytest.raises(api.GlimAmdError):
        api.IntegratedGICPFactor(np.eye(4), 1, tg, bare).linearize({1: delta})
    # a radius far beyond what the index was sized for is refused (bounded ring walk), not searched incompletely
    g.set_max_correspondence_distance(100.0)
    with pytest.raises(api.GlimAmdError):
        g.linearize({1: delta})
    g.set_max_correspondence_distance(5.0)  # 5 x the hint the shared index was built with: fine, and still exact
    np.testing.assert_array_equal(g.correspondences({1: delta}), orc.gicp_linearize(tp, tc, sp, sc, delta, 5.0, want_corr=True)["corr"])


# ---- the edges of the block epilogue and of the fixed-order sums (gicp.hip store_partial_row, ordered_column_sum) ----------------------
BLOCK, FINALISER_TRIP, CT_SUM_TRIP = 256, 8 * 16, 8 * 8  # threads per block; rows per trip of gicp_finalize_kernel / ct_sum_kernel
CT_EDGE_POINTS = 3000


def rigid_edge_sizes(num_cus):
    """1 point, one thread short of a block, a full block, one block and a point, and the smallest source that makes one block more than
    a full finaliser trip -- with the points per thread that gicp.hip's points_per_thread picks on a device of num_cus compute units"""
    def blocks(n):
        ppt = max(1, min(64, -(-n // (BLOCK * 4 * num_cus))))
        return -(-n // (BLOCK * ppt))

    return [1, BLOCK - 1, BLOCK, BLOCK + 1, next(n for n in range(1, 1 << 24) if blocks(n) == FINALISER_TRIP + 1)]


def rigid_edge_subset(sp, n):
    return np.arange(n) * (len(sp) // n)  # spread over the whole scan, so that every size but 1 gives a well-posed system


def ct_edge_times(buckets, n=CT_EDGE_POINTS):
    """times that make `buckets` equal time buckets of a source of n points; from 3 buckets on, the middle bucket keeps a single point and
    hands the rest to the next one (with 2 buckets a single-point bucket would leave the 6 dof of one key to a rank-3 system)"""
    k = (np.arange(n) * buckets) // n
    if buckets >= 3:
        k[np.flatnonzero(k == buckets // 2)[1:]] += 1
    return k * 0.002


CT_EDGE_BUCKETS = [1, 2, CT_SUM_TRIP, CT_SUM_TRIP + 1]
CT_EDGE_X, CT_EDGE_Y = [0.001, 0.0, 0.002, 0.02, 0.01, 0.0], [0.0, -0.001, 0.0, 0.0, 0.02, -0.01]


def test_gicp_sum_edge_cases_all_have_inliers(orc):
    """the cases of test_gicp_sum_edges on the CPU: the correspondences need no covariances, so identity ones stand in"""
    from glim_amd import synth
    from ct_restatement import expmap, moving_source, np_ct_linearize, static_map, sweep_poses, time_table
    from scipy.spatial import cKDTree

    poses = synth.arc_trajectory(2, step=0.6, yaw_step_deg=3.0)
    dirs = synth.lidar_directions(64, 1024)
    tp, sp = (synth.scan(synth.Scene.default(), T, dirs, frame_id=i).astype(np.float64) for i, T in enumerate(poses))
    T = np.linalg.inv(poses[0]) @ poses[1] @ orc.se3_exp([0.004, -0.003, 0.002, 0.03, 0.02, -0.01])
    sizes = rigid_edge_sizes(256)
    assert sizes == [1, 255, 256, 257, 128 * 256 + 1] and len(sp) >= sizes[-1]
    tree = cKDTree(tp)
    for n in sizes:
        q = sp[rigid_edge_subset(sp, n)] @ T[:3, :3].T + T[:3, 3]
        assert (tree.query(q, k=1)[0] <= 1.0).sum() > 0, n
    tp = static_map(16, 512)
    p, _ = moving_source(16, 256)
    sp = p[:CT_EDGE_POINTS]
    eye = lambda m: np.tile(np.eye(3), (m, 1, 1))
    T0, T1 = sweep_poses()
    for buckets in CT_EDGE_BUCKETS:
        times = ct_edge_times(buckets)
        table, idx = time_table(times)
        assert len(table) == buckets and (buckets < 3 or (idx == buckets // 2).sum() == 1)
        L = np_ct_linearize(orc, tp, eye(len(tp)), sp, eye(len(sp)), times, T0 @ expmap(CT_EDGE_X), T1 @ expmap(CT_EDGE_Y), 1.0)
        assert L["num_inliers"] > 0 and (L["corr"][idx == buckets // 2] >= 0).any(), buckets  # the single-point bucket has its inlier too


@pytest.mark.gpu
def test_gicp_sum_edges(orc):
    """Rigid and continuous-time records at the sizes where the shared block epilogue and the ordered column sum change path, against the FP64
    restatements (np_gicp, np_ct_linearize) at the tolerances of test_hip_gicp_matches_oracle and of ct_restatement._check_record.  The GN
    step of the rigid record is compared from BLOCK - 1 points on: one point gives a rank-3 system, whose step the regulariser decides."""
    from ct_restatement import _check_record, _target, expmap, moving_source, np_ct_linearize, sweep_poses, time_table
    from glim_amd import api

    ctx = api.Context(0, 1)
    ((tp, tc, tg), (sp, sc, sg)), delta = clouds(orc, api, ctx, rings=64, az=1024)
    T = delta @ orc.se3_exp([0.004, -0.003, 0.002, 0.03, 0.02, -0.01])
    sizes = rigid_edge_sizes(ctx.device_info()["num_cus"])
    assert len(sp) >= sizes[-1]
    owner = api.IntegratedGICPFactor(np.eye(4), 1, tg, sg, max_correspondence_distance=1.0)  # owns the index the cases borrow: lives to the end
    for n in sizes:
        sel = rigid_edge_subset(sp, n)
        g = api.PointCloudGPU.clone(sp[sel], covs=sc[sel], ctx=ctx)
        f = api.IntegratedGICPFactor(np.eye(4), 1, tg, g, target_tree=owner.target_tree, max_correspondence_distance=1.0)
        got, e = f.linearize({1: T}), f.error({1: T})
        ref = np_gicp(tp, tc, sp[sel], sc[sel], T, 1.0)
        print(f"rigid {n} points: inliers {got['num_inliers']} / {ref['num_inliers']}, error {got['error']:.9g} / {e:.9g} / {ref['error']:.9g}")
        assert got["num_inliers"] == ref["num_inliers"] > 0
        scale = np.abs(ref["H_ss"]).max()
        np.testing.assert_allclose(got["error"], ref["error"], rtol=2e-4)
        np.testing.assert_allclose(got["H_ss"], ref["H_ss"], rtol=0, atol=2e-4 * scale)
        np.testing.assert_allclose(got["b_s"], ref["b_s"], rtol=0, atol=2e-4 * np.abs(ref["b_s"]).max() + 1e-6 * scale)
        assert abs(e - ref["error"]) <= 2e-4 * ref["error"]
        if n > 1:
            lam = 1e-6 * np.trace(ref["H_ss"]) / 6
            assert np.abs(gn_step(got, lam) - gn_step(ref, lam)).max() < POSE_TOL
        f.close()
        g.close()
    owner.close()
    # continuous-time: 1, 2, one full trip and one trip + 1 buckets; the middle bucket of the last two holds one point
    tp, tc, tg = _target(api, ctx, 16, 512)
    p, _ = moving_source(16, 256)
    g = api.PointCloudGPU.clone(p[:CT_EDGE_POINTS], ctx=ctx)
    g.find_neighbors(10, download=False)
    g.estimate_covariances(10)
    sp, sc, _ = g.download(covs=True, normals=False)
    sp, sc = sp.astype(np.float64), sc.astype(np.float64)
    T0, T1 = sweep_poses()
    vals = {0: T0 @ expmap(CT_EDGE_X), 1: T1 @ expmap(CT_EDGE_Y)}
    for buckets in CT_EDGE_BUCKETS:
        times = ct_edge_times(buckets)
        f = api.IntegratedCT_GICPFactor(0, 1, tg, g, times=times)
        tab, Tk, D0, D1, idx = f.debug_poses(vals)
        assert len(tab) == buckets and (buckets < 3 or (idx == buckets // 2).sum() == 1)
        np.testing.assert_array_equal(idx, time_table(times)[1])
        got, e = f.linearize(vals), f.error(vals)
        ref = np_ct_linearize(orc, tp, tc, sp, sc, times, vals[0], vals[1], 1.0, poses=(Tk, D0, D1))
        print(f"ct {buckets} buckets: inliers {got['num_inliers']} / {ref['num_inliers']}, error {got['error']:.9g} / {e:.9g} / {ref['error']:.9g}")
        _check_record(got, ref)
        np.testing.assert_allclose(e, ref["error"], rtol=2e-4)
        f.close()
