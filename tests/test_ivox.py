"""The device iVox (gtsam_points::IncrementalVoxelMap<FlatContainer>) and the GICP / continuous-time GICP factors over it, against the FP64
restatement of tests/ivox_restatement.py: container parity over a drive (with eviction and slot reuse, and one raw 131 072-point frame),
correspondences for the neighbour modes, the rigid and the continuous-time factor on the map, the frame-to-model loop of
odometry_estimation_ct.cpp:147-235, and the edge cases.  CPU tests pin the restatement on cases small enough to verify by eye."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ct_restatement as ctg
import ivox_restatement as ivr
from ct_restatement import _prior

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSE_TOL = 1e-4
EYE3 = np.eye(3, dtype=np.float32)


def _covs(n):
    return np.tile(EYE3 * 0.01, (n, 1, 1))


# ---- CPU: the restatement on hand-made cases ------------------------------------------------------------------------------------------


def test_hand_made_insert_rejects_duplicates_fills_cells_and_keeps_first_seen_order():
    m = ivr.IVox(1.0, min_dist=0.1, max_points=3, lru_horizon=1, lru_clear_cycle=2)
    pts = np.array([
        [0.95, 0.5, 0.5],    # voxel (0,0,0), place 0
        [1.05, 0.5, 0.5],    # straddles the face x = 1: voxel (1,0,0), although it is 0.1 from the first point
        [0.95, 0.55, 0.5],   # 0.05 from place 0 of (0,0,0): rejected
        [0.2, 0.2, 0.2],     # (0,0,0) place 1
        [-0.1, 0.2, 0.2],    # floor(-0.1) = -1: voxel (-1,0,0)
        [0.5, 0.9, 0.1],     # (0,0,0) place 2: the cell is now full
        [0.7, 0.1, 0.9],     # (0,0,0): full, dropped although it is far from the others
    ], dtype=np.float32)
    m.insert(pts, _covs(len(pts)))
    assert [v.coord for v in m.voxels] == [(0, 0, 0), (1, 0, 0), (-1, 0, 0)]  # first-seen order
    v = m.as_dict()
    assert v[(0, 0, 0)].count == 3 and v[(1, 0, 0)].count == 1 and v[(-1, 0, 0)].count == 1
    np.testing.assert_array_equal(v[(0, 0, 0)].pts[:3], pts[[0, 3, 5]])
    assert m.num_points() == 5 and m.lru_counter == 1
    # the rejection is strict: a point at exactly min_dist (squared distance == min_sq in FP64) is accepted
    e = ivr.IVox(1.0, min_dist=0.25, max_points=4)
    e.insert(np.array([[0.25, 0.5, 0.5], [0.5, 0.5, 0.5], [0.5, 0.5, 0.625]], dtype=np.float32), _covs(3))
    assert e.as_dict()[(0, 0, 0)].count == 2  # 0.25 away: kept; 0.125 from the second: rejected


def test_hand_made_eviction_happens_exactly_at_lru_plus_horizon_below_counter_and_keeps_survivor_order():
    m = ivr.IVox(1.0, min_dist=0.0, max_points=4, lru_horizon=1, lru_clear_cycle=2)
    one = lambda x: (np.array([[x + 0.5, 0.5, 0.5]], dtype=np.float32), _covs(1))
    m.insert(*one(0))                    # counter 0 -> 1: voxel 0 lru 0; 1 % 2 != 0
    m.insert(*one(1))                    # counter 1 -> 2: voxel 1 lru 1; sweep: 0 + 1 < 2 evicts voxel 0; 1 + 1 < 2 is false
    assert [v.coord[0] for v in m.voxels] == [1]
    m.insert(*one(2))                    # counter 2 -> 3
    p = np.array([[3.5, 0.5, 0.5], [1.5, 0.6, 0.5]], dtype=np.float32)
    m.insert(p, _covs(2))                # counter 3 -> 4: voxel 3 new, voxel 1 touched; sweep: voxel 2 (lru 2): 2 + 1 < 4 evicted
    assert [v.coord[0] for v in m.voxels] == [1, 3]  # survivors keep their order
    assert m.as_dict()[(1, 0, 0)].count == 2 and m.lru_counter == 4
    # a voxel whose points were all rejected is still touched
    t = ivr.IVox(1.0, min_dist=0.5, max_points=4, lru_horizon=0, lru_clear_cycle=1)
    t.insert(*one(0))                    # 0 + 0 < 1: evicted at once (horizon 0 keeps only what ... nothing: lru is the counter BEFORE the increment)
    assert t.num_voxels() == 0


def test_the_search_is_not_an_exact_nearest_neighbour_search():
    m = ivr.IVox(1.0, min_dist=0.0, max_points=4, mode=1)
    pts = np.array([[0.1, 0.5, 0.5], [1.02, 0.5, 0.5]], dtype=np.float32)
    m.insert(pts, _covs(2))
    q = np.array([0.9, 0.5, 0.5])
    hit = m.nearest(q, 2.0)
    assert hit[0] == (0, 0, 0) and hit[1] == 0 and abs(hit[2] - 0.64) < 1e-6   # the farther in-voxel point: the true neighbour is never seen
    m.mode = 7
    hit = m.nearest(q, 2.0)
    assert hit[0] == (1, 0, 0) and abs(hit[2] - 0.12 ** 2) < 1e-6
    assert m.nearest(q, 0.1) is None                                            # valid iff d^2 <= max^2
    # mode 7 does not see an edge neighbour, 19 and 27 do; 19 does not see a corner, 27 does
    c = ivr.IVox(1.0, min_dist=0.0, max_points=4)
    c.insert(np.array([[1.1, 1.1, 0.5], [1.05, 1.05, 1.05]], dtype=np.float32), _covs(2))
    q = np.array([0.9, 0.9, 0.9])
    seen = {}
    for mode in (1, 7, 19, 27):
        c.mode = mode
        h = c.nearest(q, 2.0)
        seen[mode] = None if h is None else h[0]
    assert seen == {1: None, 7: None, 19: (1, 1, 0), 27: (1, 1, 1)}
    assert len(ivr.OFFSETS[19]) == 19 and len(set(ivr.OFFSETS[19])) == 19 and set(ivr.OFFSETS[19]) < set(ivr.OFFSETS[27])
    assert ivr.OFFSETS[27][0] == (-1, -1, -1) and ivr.OFFSETS[27][1] == (0, -1, -1) and ivr.OFFSETS[27][13] == (0, 0, 0)


def test_ivox_symbols_are_exported_and_check_their_arguments_without_a_device():
    from glim_amd import _lib

    L = _lib.lib()
    names = [n for n in _lib.SYMBOLS if "ivox" in n]
    assert len(names) == 15 and not any("ct_gicp" in n for n in names)
    header = open(os.path.join(ROOT, "include", "glim_amd.h")).read()
    diag = open(os.path.join(ROOT, "include", "glim_amd_diag.h")).read()
    for n in names:
        assert hasattr(L, n), n
        assert (n in diag) if n.startswith("glim_amd_debug_") else (n in header), n
    X = np.eye(4)[:3].reshape(12).copy()
    dp = X.ctypes.data_as(C.POINTER(C.c_double))
    h = C.c_void_p()
    rec = _lib.Linearized6()
    e, n = C.c_double(), C.c_int64()
    assert L.glim_amd_ivox_create(None, 1.0, C.byref(h)) == -1
    assert L.glim_amd_ivox_destroy(None) == 0
    assert L.glim_amd_ivox_set_insertion(None, 0.1, 20) == -1
    assert L.glim_amd_ivox_set_lru(None, 10, 10) == -1
    assert L.glim_amd_ivox_set_neighbor_voxel_mode(None, 7) == -1
    assert L.glim_amd_ivox_insert(None, None, None) == -1
    assert L.glim_amd_ivox_info(None, None, None, None, None) == -1
    assert L.glim_amd_ivox_download(None, None, None, None, None) == -1
    assert L.glim_amd_ivox_voxel_points(None, None) == -1
    assert L.glim_amd_ivox_gicp_linearize(None, None, dp, 1.0, 0, C.byref(rec)) == -1
    assert L.glim_amd_ivox_gicp_error(None, None, dp, 1.0, C.byref(e), C.byref(n)) == -1
    assert L.glim_amd_ivox_gicp_correspondences(None, None, dp, 1.0, None) == -1
    assert L.glim_amd_ivox_ct_factor_create(None, None, None, C.byref(h)) == -1
    assert L.glim_amd_debug_ivox_set_initial_capacity(None, 4) == -1
    assert L.glim_amd_debug_ivox_capacity(None, None, None) == -1
    # the C++ mirror and the gtsam adapter name the new entry points
    compat = open(os.path.join(ROOT, "include", "glim_amd", "gtsam_points_compat.hpp")).read()
    assert re.search(r"class IncrementalVoxelMap\b", compat) and re.search(r"glim_amd_ivox_insert\s*\(", compat)
    assert re.search(r"glim_amd_ivox_ct_factor_create\s*\(", compat) and re.search(r"glim_amd_ivox_gicp_linearize\s*\(", compat)
    adapter = open(os.path.join(ROOT, "adapters", "gtsam", "glim_amd_gtsam.hpp")).read()
    assert re.search(r"IncrementalVoxelMap", adapter)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def gpu_ctx():
    from glim_amd import api

    return api.Context(0, 1)


def drive_poses(n):
    """n + 1 sensor poses along a gentle arc, ~0.5 m and 2 degrees per sweep: sweep i runs from pose i to pose i + 1"""
    from glim_amd import synth

    return synth.arc_trajectory(n + 1, step=0.5, yaw_step_deg=2.0)


@pytest.fixture(scope="module")
def drive(gpu_ctx):
    """20 sweeps of a moving sensor through the shipped preprocessing (~10 000 points each) with covariances: device clouds + their host images"""
    from glim_amd import api, synth

    poses = drive_poses(20)
    frames = []
    for i in range(20):
        p, t = synth.moving_scan(synth.Scene.default(), poses[i], poses[i + 1], 64, 1024, duration=0.1, frame_id=40 + i)
        g = api.PointCloudGPU.preprocess(p.astype(np.float64), t, None, ctx=gpu_ctx)
        g.estimate_covariances(10)
        xyz, covs, _ = g.download(covs=True, normals=False)
        assert 8000 < len(xyz) < 14000
        frames.append((g, xyz.astype(np.float32), covs.astype(np.float32), g.download_frame()["times"]))
    return poses, frames


def _glim_ct_map(api, ctx, horizon=30, cycle=10, mode=1, min_dist=0.05, max_points=20, leaf=1.0):
    m = api.IncrementalVoxelMap(leaf, ctx=ctx)
    m.voxel_insertion_setting(min_dist=min_dist, max_points=max_points)
    m.set_lru_horizon(horizon)
    m.set_lru_clear_cycle(cycle)
    m.set_neighbor_voxel_mode(mode)
    ref = ivr.IVox(leaf, min_dist=min_dist, max_points=max_points, lru_horizon=horizon, lru_clear_cycle=cycle, mode=mode)
    return m, ref


def assert_same_map(dev, ref, ordered=True):
    """download() voxel by voxel, keyed by coordinate: same voxel set, same counts, same points bit for bit in the same in-cell order,
    covariances within 1e-6 relative; info() and voxel_points() agree with the same data"""
    coords, counts, points, covs = dev.download()
    info = dev.info()
    assert info["num_voxels"] == len(coords) == ref.num_voxels()
    assert info["lru_counter"] == ref.lru_counter and info["leaf_size"] == ref.leaf
    keys = [tuple(int(x) for x in c) for c in coords]
    assert len(set(keys)) == len(keys)
    rd = ref.as_dict()
    assert set(keys) == set(rd)
    if ordered:  # slot order is upstream's voxel order: first seen first, survivors keep their order
        assert keys == [v.coord for v in ref.voxels]
    for s, k in enumerate(keys):
        v = rd[k]
        assert counts[s] == v.count, (k, counts[s], v.count)
        np.testing.assert_array_equal(points[s, : v.count].view(np.uint32), v.pts[: v.count].view(np.uint32))
        a, b = covs[s, : v.count].astype(np.float64), v.covs[: v.count].astype(np.float64)
        if v.count:
            scale = np.abs(b).reshape(v.count, -1).max(axis=1)[:, None, None]
            assert np.all(np.abs(a - b) <= 1e-6 * scale), (k, np.abs(a - b).max(), scale.max())
        assert not points[s, v.count:].any()
    assert info["num_points"] == int(counts.sum()) == ref.num_points()
    np.testing.assert_array_equal(dev.voxel_points(), ref.voxel_points())
    return coords, counts, points, covs


@pytest.mark.gpu
@pytest.mark.parametrize("horizon,cycle", [(30, 10), (3, 2)])
def test_container_matches_the_sequential_insert_over_a_drive(gpu_ctx, drive, horizon, cycle):
    from glim_amd import api

    poses, frames = drive
    dev, ref = _glim_ct_map(api, gpu_ctx, horizon, cycle)
    sizes, evicted = [], 0
    for i, (g, xyz, covs, _) in enumerate(frames):
        before = ref.num_voxels()
        dev.insert(g, poses[i])
        ref.insert(xyz, covs, poses[i])
        assert_same_map(dev, ref)
        sizes.append(ref.num_points())
        evicted += ref.lru_counter % cycle == 0 and ref.num_voxels() < before
    print(f"horizon {horizon} cycle {cycle}: voxels {ref.num_voxels()}, points per insert {sizes}, sweeps that evicted {evicted}")
    if horizon == 3:
        assert evicted >= 3  # eviction and slot reuse happened several times
    else:
        assert evicted == 0
    dev.close()


@pytest.mark.gpu
def test_container_takes_a_raw_131072_point_frame_in_one_call_and_is_deterministic(gpu_ctx, drive):
    from glim_amd import api

    poses, frames = drive
    p, _ = ctg.moving_source(128, 1024)
    g = api.PointCloudGPU.clone(p, ctx=gpu_ctx)
    g.find_neighbors(10, download=False)
    g.estimate_covariances(10)
    xyz, covs, _ = g.download(covs=True, normals=False)
    assert len(xyz) == 131072
    T0, _ = ctg.sweep_poses()
    dev, ref = _glim_ct_map(api, gpu_ctx)
    dev.insert(g, T0)
    ref.insert(xyz.astype(np.float32), covs.astype(np.float32), T0)
    _, counts, _, _ = assert_same_map(dev, ref)
    # the case that breaks a racy insert: many voxels receive hundreds of candidates in the one call (counted from the input alone)
    vc, ok = ivr.voxel_coords(ivr.transform_points(xyz, T0), 1.0)
    per_voxel = np.unique(vc[ok], axis=0, return_counts=True)[1]
    print(f"raw frame: {len(counts)} voxels, candidates per voxel mean {per_voxel.mean():.0f} max {per_voxel.max()}, {int((per_voxel >= 200).sum())} voxels "
          f"with >= 200, {int(counts.sum())} points kept, {int((counts == 20).sum())} full cells")
    assert (per_voxel >= 200).sum() >= 50 and (counts == 20).sum() >= 50
    # two identical insert sequences give identical downloads
    downloads = []
    for _ in range(2):
        m, _r = _glim_ct_map(api, gpu_ctx, 3, 2)
        for i in range(4):
            m.insert(frames[i][0], poses[i])
        m.insert(g, T0)
        downloads.append(m.download())
        m.close()
    for a, b in zip(*downloads):
        np.testing.assert_array_equal(a, b)
    dev.close()


def _hits_to_pairs(dev, corr):
    coords = dev.download()[0]
    cap = dev.max_points
    return [None if c < 0 else (tuple(int(x) for x in coords[c // cap]), int(c % cap)) for c in corr]


def _compare_hits(got, ref_hits, fragile, what):
    """exact, except -- by the rule of the issue -- at no more than 2 fragile points; the caller has asserted that there are none"""
    bad = [i for i in range(len(ref_hits)) if got[i] != ref_hits[i]]
    print(f"{what}: {len(ref_hits)} points, {sum(h is not None for h in ref_hits)} matched, fragile {len(fragile)}, mismatches {len(bad)}")
    assert len(bad) <= 2 and set(bad) <= set(fragile), (what, bad[:10])


@pytest.fixture(scope="module")
def model_and_frame(gpu_ctx, drive):
    """the first 6 sweeps of the drive in a map (device + restatement), and the 7th as source at a slightly wrong pose"""
    from glim_amd import api

    poses, frames = drive
    dev, ref = _glim_ct_map(api, gpu_ctx)
    for i in range(6):
        dev.insert(frames[i][0], poses[i])
        ref.insert(frames[i][1], frames[i][2], poses[i])
    T = poses[6] @ ctg.expmap([0.002, -0.001, 0.003, 0.03, -0.02, 0.01])
    return dev, ref, frames[6], T


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 7, 27])
def test_correspondences_match_the_bounded_search(gpu_ctx, model_and_frame, mode):
    from glim_amd import api

    dev, ref, (g, xyz, covs, _), T = model_and_frame
    dev.set_neighbor_voxel_mode(mode)
    ref.mode = mode
    q = ivr.transform_q(T, xyz)
    ref_hits, fragile = ivr.search_all(ref, q, 1.0)
    assert fragile == []  # the inputs were chosen so that the allowance below never hides a failure
    f = api.IntegratedGICPFactor(np.eye(4), 1, dev, g, max_correspondence_distance=1.0)
    got = _hits_to_pairs(dev, f.correspondences({1: T}))
    _compare_hits(got, ref_hits, fragile, f"mode {mode}")
    assert sum(h is not None for h in ref_hits) > 0.5 * len(xyz)
    dev.set_neighbor_voxel_mode(1)
    ref.mode = 1


def _check6(got, ref):
    assert got["num_inliers"] == ref["num_inliers"] > 0
    np.testing.assert_allclose(got["error"], ref["error"], rtol=2e-4)
    scale = np.abs(ref["H_ss"]).max()
    np.testing.assert_allclose(got["H_ss"], ref["H_ss"], rtol=0, atol=2e-4 * scale)
    np.testing.assert_allclose(got["b_s"], ref["b_s"], rtol=0, atol=2e-4 * np.abs(ref["b_s"]).max() + 1e-6 * scale)
    lam = 1e-6 * np.trace(ref["H_ss"]) / 6
    step = lambda L: np.linalg.solve(L["H_ss"] + lam * np.eye(6), -L["b_s"])
    assert np.abs(step(got) - step(ref)).max() < POSE_TOL


@pytest.mark.gpu
def test_rigid_gicp_factor_on_the_map_matches_the_restatement(gpu_ctx, model_and_frame):
    from glim_amd import api

    dev, ref, (g, xyz, covs, _), T = model_and_frame
    sp, sc = xyz.astype(np.float64), covs.astype(np.float64)
    hits, fragile = ivr.search_all(ref, ivr.transform_q(T, sp), 1.0)
    assert fragile == []
    want = ivr.gicp_on_hits(ref, hits, sp, sc, T)
    f = api.IntegratedGICPFactor(np.eye(4), 1, dev, g, max_correspondence_distance=1.0)
    got = f.linearize({1: T})
    _check6(got, want)
    np.testing.assert_allclose(f.error({1: T}), want["error"], rtol=2e-4)
    assert f.inlier_fraction() == want["num_inliers"] / len(sp)
    # binary form: the target blocks come from the same record
    b = api.IntegratedGICPFactor(0, 1, dev, g, max_correspondence_distance=1.0).linearize({0: np.eye(4), 1: T})
    np.testing.assert_array_equal(b["H_ss"], got["H_ss"])
    assert np.abs(b["H_tt"]).max() > 0
    again = f.linearize({1: T})
    np.testing.assert_array_equal(again["H_ss"], got["H_ss"])


def _frozen_error(ref, hits, sp, sc, idx, T_lin, T_eval):
    vox = ref.as_dict()
    e = 0.0
    for i, h in enumerate(hits):
        if h is None:
            continue
        k = idx[i]
        R = T_lin[k][:3, :3]
        v = vox[h[0]]
        M = np.linalg.inv(v.covs[h[1]].astype(np.float64) + R @ sc[i] @ R.T)
        r = v.pts[h[1]].astype(np.float64) - (T_eval[k][:3, :3] @ sp[i] + T_eval[k][:3, 3])
        e += r @ M @ r
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["pre10k", "raw131k"])
def test_ct_factor_on_the_map_matches_the_restatement_on_a_moving_scan(gpu_ctx, kind):
    from glim_amd import api

    ctx = gpu_ctx
    tp, tc, tg = ctg._target(api, ctx, 64, 1024)
    sp, sc, times, pass_times, sg = ctg._source(api, ctx, kind)
    assert (kind == "pre10k" and 8000 < len(sp) < 14000) or len(sp) == 131072
    dev, ref = _glim_ct_map(api, ctx)
    dev.insert(tg)
    ref.insert(tp.astype(np.float32), tc.astype(np.float32))
    assert_same_map(dev, ref)
    T0, T1 = ctg.sweep_poses()
    X = T0 @ ctg.expmap([0.002, -0.001, 0.003, 0.03, -0.02, 0.01])
    Y = T1 @ ctg.expmap([-0.001, 0.002, -0.002, 0.02, 0.03, -0.01])
    values = {0: X, 1: Y}
    f = api.IntegratedCT_GICPFactor(0, 1, dev, sg, target_tree=dev, max_correspondence_distance=1.0, times=pass_times)
    tab, T, D0, D1, idx = f.debug_poses(values)
    table, idx_ref = ctg.time_table(times)
    np.testing.assert_array_equal(idx, idx_ref)
    want, hits, fragile = ivr.ct_on_ivox(ref, sp, sc, idx, (T, D0, D1), 1.0)
    assert fragile == []
    got = f.linearize(values)
    _compare_hits(_hits_to_pairs(dev, f.correspondences(values)), hits, fragile, kind)
    ctg._check_record(got, want)
    # error(): the correspondences and M of the last linearize, at other values
    moved = {0: X @ ctg.expmap([0.001, 0.0, -0.001, 0.01, 0.0, 0.01]), 1: Y @ ctg.expmap([0.0, 0.002, 0.0, -0.01, 0.02, 0.0])}
    e, n = f.error(moved, with_inliers=True)
    assert n == want["num_inliers"]
    Tm = f.debug_poses(moved)[1]
    if kind == "pre10k":
        np.testing.assert_allclose(e, _frozen_error(ref, hits, sp, sc, idx, T, Tm), rtol=2e-4)
    np.testing.assert_allclose(f.error(values), got["error"], rtol=2e-5)
    # two identical calls give identical bits
    a, b = f.linearize(values), f.linearize(values)
    for k in ("H_00", "H_01", "H_11", "b_0", "b_1"):
        np.testing.assert_array_equal(a[k], b[k])
    assert a["error"] == b["error"]
    if kind == "pre10k":
        # an insert after linearize invalidates the kept state: error() recomputes the correspondences in the map as it now is.  The inserted
        # points are the source itself at the moved poses' deskewed positions: every point then finds a neighbour at distance ~0
        f.linearize(values)
        e_kept = f.error(moved)
        dsk = f.deskewed_cloud(moved, local=False)
        dsk.estimate_covariances(10)
        dxyz, dcov, _ = dsk.download(covs=True, normals=False)
        dev.insert(dsk)
        ref.insert(dxyz.astype(np.float32), dcov.astype(np.float32))
        assert_same_map(dev, ref)
        want2, hits2, fragile2 = ivr.ct_on_ivox(ref, sp, sc, idx, (Tm, D0, D1), 1.0)
        e_new, n_new = f.error(moved, with_inliers=True)
        assert n_new == want2["num_inliers"]
        np.testing.assert_allclose(e_new, want2["error"], rtol=2e-4, atol=1e-6 * want["error"])
        assert hits2 != hits and e_new < 0.9 * e_kept  # the inserted points change the answer
        dsk.close()
    # the map cannot be destroyed under the factor
    with pytest.raises(api.GlimAmdError):
        dev.close()
    f.close()
    dev.close()


def _between_identity(X, Y, prec):
    """BetweenFactor(X, Y, Pose3()): r = Log(X^-1 Y); d r / d X = -J_r^-1(r) Ad((X^-1 Y)^-1), d r / d Y = J_r^-1(r)"""
    D = np.linalg.inv(X) @ Y
    r = ctg.logmap(D)
    Jinv = np.linalg.inv(ctg.expmap_derivative(r))
    J = np.hstack([-Jinv @ ctg.adjoint(np.linalg.inv(D)), Jinv])
    return prec * J.T @ J, prec * J.T @ r, prec * r @ r


def _miss(A, B):
    E = np.linalg.inv(B) @ A
    return np.linalg.norm(E[:3, 3]), np.degrees(np.linalg.norm(ctg.logmap(E)[:3]))


@pytest.mark.gpu
def test_frame_to_model_loop_recovers_every_sweep(gpu_ctx):
    """odometry_estimation_ct.cpp:147-235 over 12 sweeps: the CT factor over the map, Prior(X, last end, 1e-3), Between(X, Y, identity, 1e-3), LM
    <= 8 iterations from a constant-velocity guess, deskewed_cloud(local), estimate_covariances, insert at the estimated begin pose."""
    from glim_amd import api, synth

    ctx = gpu_ctx
    poses = drive_poses(12)
    dev, _ = _glim_ct_map(api, ctx)
    sizes = []
    last_X = last_Y = None
    for i in range(12):
        p, t = synth.moving_scan(synth.Scene.default(), poses[i], poses[i + 1], 64, 1024, duration=0.1, frame_id=70 + i)
        sg = api.PointCloudGPU.preprocess(p.astype(np.float64), t, None, ctx=ctx)
        sg.estimate_covariances(10)
        if i == 0:
            X, Y = poses[0], poses[1]  # the first frame is the origin of the map (its sweep poses are given)
            f = api.IntegratedCT_GICPFactor(0, 1, dev, sg, max_correspondence_distance=1.0)
        else:
            twist = 0.85 * ctg.logmap(np.linalg.inv(last_X) @ last_Y) if i >= 2 else ctg.logmap(np.linalg.inv(last_X) @ last_Y)
            X_pred = last_Y.copy()
            X, Y = X_pred.copy(), X_pred @ ctg.expmap(twist)
            f = api.IntegratedCT_GICPFactor(0, 1, dev, sg, max_correspondence_distance=1.0)
            lam = 1e-10
            for it in range(8):
                L = f.linearize({0: X, 1: Y})
                H, b = ctg.full_system(L)
                H, b = H.copy(), b.copy()
                Hp, bp, cp = _prior(X, X_pred, 1e-3)
                Hb, bb, cb = _between_identity(X, Y, 1e-3)
                H[:6, :6] += Hp
                b[:6] += bp
                H += Hb
                b += bb
                cost0 = L["error"] + cp + cb
                while True:
                    dx = np.linalg.solve(H + lam * np.eye(12), -b)
                    Xn, Yn = X @ ctg.expmap(dx[:6]), Y @ ctg.expmap(dx[6:])
                    cost = f.error({0: Xn, 1: Yn}) + _prior(Xn, X_pred, 1e-3)[2] + _between_identity(Xn, Yn, 1e-3)[2]
                    if cost <= cost0 or lam > 1e5:
                        lam = max(lam / 10.0, 1e-10)
                        break
                    lam *= 10.0
                X, Y = Xn, Yn
                if np.abs(dx).max() < 1e-6:
                    break
            for est, truth, name in ((X, poses[i], "begin"), (Y, poses[i + 1], "end")):
                dt, dr = _miss(est, truth)
                print(f"sweep {i} {name}: {dt:.4f} m, {dr:.4f} deg")
                assert dt < 0.02 and dr < 0.2, (i, name, dt, dr)
        dsk = f.deskewed_cloud({0: X, 1: Y}, local=True)
        dsk.estimate_covariances(10)
        f.close()
        dev.insert(dsk, X)
        sizes.append(dev.info()["num_points"])
        dsk.close()
        sg.close()
        last_X, last_Y = X, Y
    print("map points after each sweep:", sizes)
    # sub-linear growth: min_dist rejects re-observed surface.  Linear growth would add a whole sweep (the first entry) per insert; every later
    # insert adds less than that, and the late inserts add less than the early ones (the sensor moves 0.5 m per sweep through a closed room)
    inc = np.diff(sizes)
    assert (inc < sizes[0]).all() and sizes[-1] < 12 * sizes[0]
    assert inc[-3:].mean() < inc[:3].mean()
    dev.close()


@pytest.mark.gpu
def test_ivox_edge_cases(gpu_ctx, drive):
    from glim_amd import api

    poses, frames = drive
    g, xyz, covs, _ = frames[0]
    ctx = api.Context(0, 1)
    src = api.PointCloudGPU.clone(xyz[:500], covs=covs[:500], ctx=ctx)
    # empty map, empty source
    m = api.IncrementalVoxelMap(1.0, ctx=ctx)
    assert m.info() == {"num_voxels": 0, "num_points": 0, "lru_counter": 0, "leaf_size": 1.0}
    assert m.voxel_points().shape == (0, 3) and m.download()[0].shape == (0, 3)
    f = api.IntegratedGICPFactor(np.eye(4), 1, m, src)
    L = f.linearize({1: np.eye(4)})
    assert L["num_inliers"] == 0 and L["error"] == 0.0 and not L["H_ss"].any()
    assert (f.correspondences({1: np.eye(4)}) == -1).all()
    empty = api.PointCloudGPU.clone(np.zeros((0, 3)), covs=np.zeros((0, 3, 3)), ctx=ctx)
    m.insert(empty)
    assert m.info()["num_voxels"] == 0 and m.info()["lru_counter"] == 1
    m.insert(src)
    assert api.IntegratedGICPFactor(np.eye(4), 1, m, empty).linearize({1: np.eye(4)})["num_inliers"] == 0
    ct = api.IntegratedCT_GICPFactor(0, 1, m, empty, times=np.zeros(0))
    assert ct.linearize({0: np.eye(4), 1: np.eye(4)})["num_inliers"] == 0
    # the settings are refused once the map is non-empty; bad values are refused always
    with pytest.raises(api.GlimAmdError) as ei:
        m.voxel_insertion_setting(max_points=10)
    assert ei.value.code == -5
    for bad in (0, 65):
        with pytest.raises(api.GlimAmdError) as ei:
            api.IncrementalVoxelMap(1.0, ctx=ctx).voxel_insertion_setting(max_points=bad)
        assert ei.value.code == -1
    with pytest.raises(api.GlimAmdError):
        m.set_neighbor_voxel_mode(9)
    # a cloud without covariances
    bare = api.PointCloudGPU.clone(xyz[:100], ctx=ctx)
    with pytest.raises(api.GlimAmdError) as ei:
        m.insert(bare)
    assert ei.value.code == -5
    # the context refuses to go while the map or a factor on it lives; the map while the factor lives
    with pytest.raises(api.GlimAmdError):
        m.close()
    ct.close()
    with pytest.raises(api.GlimAmdError):
        ctx.close()
    m.close()
    # max_points_in_cell of 1 and of 64
    for cap in (1, 64):
        d, r = _glim_ct_map(api, ctx, max_points=cap, min_dist=0.01, leaf=4.0)  # 4 m voxels: hundreds of candidates in the densest ones
        gg = api.PointCloudGPU.clone(xyz, covs=covs, ctx=ctx)
        d.insert(gg, poses[0])
        r.insert(xyz, covs, poses[0])
        _, counts, _, _ = assert_same_map(d, r)
        assert counts.max() == cap and (counts < cap).any() == (cap == 64)
        d.close()
        gg.close()
    # non-finite points and points outside the key range are skipped
    odd = xyz[:64].copy()
    odd[3] = [np.nan, 0, 0]
    odd[7] = [np.inf, 1, 1]
    odd[11] = [3e6, 0, 0]     # 3e6 / leaf 1.0 >= 2^20
    odd[12] = [-1048576.5, 0, 0]
    odd[13] = [1048575.5, 0.5, 0.5]  # the last voxel inside the range
    d, r = _glim_ct_map(api, ctx)
    go = api.PointCloudGPU.clone(odd, covs=covs[:64], ctx=ctx)
    d.insert(go)
    r.insert(odd, covs[:64])
    assert_same_map(d, r)
    assert (1048575, 0, 0) in r.as_dict() and r.num_points() <= 60
    # a source point outside the key range has no correspondence
    far = api.IntegratedGICPFactor(np.eye(4), 1, d, go, max_correspondence_distance=1.0)
    c = far.correspondences({1: np.eye(4)})
    assert c[3] == c[7] == c[11] == c[12] == -1 and c[13] >= 0 and c[0] >= 0
    d.close()
    go.close()
    # table and slot growth forced by a tiny initial capacity: compared before and after, and against an untouched twin
    small, r = _glim_ct_map(api, ctx)
    small.debug_set_initial_capacity(4)
    twin, _ = _glim_ct_map(api, ctx)
    gs = [api.PointCloudGPU.clone(xyz[a:b], covs=covs[a:b], ctx=ctx) for a, b in ((0, 40), (40, 400), (400, len(xyz)))]
    caps = []
    for (a, b), gg in zip(((0, 40), (40, 400), (400, len(xyz))), gs):
        before = small.download()
        small.insert(gg, poses[0])
        twin.insert(gg, poses[0])
        r.insert(xyz[a:b], covs[a:b], poses[0])
        after = assert_same_map(small, r)
        nb = len(before[0])
        for x, y in zip(before, after):  # growth is invisible: the voxels that were there kept slot, count and bits (cells may have gained points)
            if x.ndim == 1:
                assert (y[:nb] >= x).all()
        np.testing.assert_array_equal(after[0][:nb], before[0])
        caps.append(small.debug_capacity())
    assert caps[0]["slots"] < caps[1]["slots"] < caps[2]["slots"] and caps[0]["table"] < caps[2]["table"]
    for a, b in zip(small.download(), twin.download()):
        np.testing.assert_array_equal(a, b)
    for o in gs + [small, twin, src, empty, bare]:
        o.close()
    ctx.close()
