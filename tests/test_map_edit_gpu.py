"""Map editing on the device (glim_amd/csrc/map_edit.hip) against the NumPy restatement (tests/map_edit_restatement.py).  Every comparison is
an equality: the predicates are FP64 in a stated operation order, the region-growing semantics do not depend on a traversal order, and the
removal is a gather.

Scene: 4 clouds of 1, 257, 1000 and 0 points from a 2 cm slab plus clutter, poses with translations of order 20 m; the 1000-point cloud is
an FP32 cloud, the others keep FP64 points.  The clouds with normals are FP32 clouds throughout.

Figures of the scene (computed by the tests on the CPU; one run on an MI355X agreed with every one): the four modes select 606 / 1 169 /
444 / 365 of 1 258 points; the outlier ball holds 986 candidates and 17 outliers, the smallest |d_i - threshold| / threshold is 1.5e-3
(required: > 1e-9); region growing at 0.15 takes 1 148 of 1 258 candidates in 16 rounds plus 13 dilated points, 1 122 with normals at
10 degrees; the two-blob scene bridges 17 of 120 points.
"""
import ctypes as C

import numpy as np
import pytest

import map_edit_restatement as R

pytestmark = pytest.mark.gpu

THR = 0.15  # the scene's distance threshold: about twice the slab's point spacing, so that the cluster has many levels


@pytest.fixture(scope="module")
def ctx():
    from glim_amd import api

    return api.Context(0, 1)


def _exact(api, ctx, clouds):
    return [api.clone_exact(p, ctx=ctx) for p in clouds]


@pytest.fixture(scope="module")
def scene(ctx):
    from glim_amd import api

    clouds, poses, _ = R.make_scene()
    gpu = [api.PointCloudGPU.clone(p.astype(np.float32), ctx=ctx) if s == 2 else api.clone_exact(p, ctx=ctx) for s, p in enumerate(clouds)]
    return {"clouds": clouds, "poses": poses, "gpu": gpu}


@pytest.fixture(scope="module")
def normal_scene(ctx):
    from glim_amd import api

    clouds, poses, normals = R.make_scene(fp32=True)
    gpu = [api.PointCloudGPU.clone(p.astype(np.float32), normals=n, ctx=ctx) for p, n in zip(clouds, normals)]
    return {"clouds": clouds, "poses": poses, "normals": normals, "gpu": gpu}


def _same_region(got, want):
    np.testing.assert_array_equal(got["pairs"], want["pairs"])
    np.testing.assert_array_equal(got["levels"], want["levels"])
    for k in ("count", "num_candidates", "seed", "seed_qq", "rounds", "status"):
        assert got[k] == want[k], k


# ---- predicates ------------------------------------------------------------------------------------------------------------------------------------
def test_each_mode_equals_the_restatement_and_capacity_is_honoured(scene):
    from glim_amd import api

    gpu, clouds, poses = scene["gpu"], scene["clouds"], scene["poses"]
    local = api.edit_local_matrices(R.MODEL, poses)
    cases = [(api.EDIT_BOX, dict(model_matrix=R.MODEL), (local, R.BOX)),
             (api.EDIT_SPHERE, dict(model_matrix=R.MODEL), (local, R.SPHERE)),
             (api.EDIT_WINDOW, dict(center=R.CENTER, resolution=0.5, window=1), (poses, R.WINDOW, R.CENTER, 0.0, 0.5, 1)),
             (api.EDIT_WINDOW_BALL, dict(center=R.CENTER, radius=0.8), (poses, R.WINDOW_BALL, R.CENTER, 0.8))]
    for mode, kw, ref in cases:
        want, _ = R.select(clouds, *ref)
        pairs, count = api.edit_select(gpu, poses, mode, **kw)
        print("mode", mode, "selected", count, "of", sum(len(c) for c in clouds))
        assert 0 < len(want) < sum(len(c) for c in clouds)
        assert count == len(want)
        np.testing.assert_array_equal(pairs, want)
        part, count2 = api.edit_select(gpu, poses, mode, capacity=37, **kw)
        assert count2 == count and len(part) == 37
        np.testing.assert_array_equal(part, want[:37])
        none, count3 = api.edit_select(gpu, poses, mode, capacity=0, **kw)
        assert count3 == count and len(none) == 0
    # no sub-map at all
    for mode, kw in ((api.EDIT_BOX, dict(model_matrix=R.MODEL)), (api.EDIT_WINDOW_BALL, dict(center=R.CENTER, radius=0.8))):
        pairs, count = api.edit_select([], [], mode, capacity=4, **kw)
        assert count == 0 and len(pairs) == 0


def test_a_point_on_each_strict_boundary_is_out(ctx):
    from glim_amd import api

    eye = [np.eye(4)]
    below = np.nextafter(0.5, 0.0)
    # box: l_x == 0.5 (the gizmo is the identity, so l = p)
    p = np.array([[0.5, 0.0, 0.0], [below, 0.0, 0.0], [-0.5, 0.1, 0.1], [0.0, 0.0, 0.5], [0.25, -0.25, below], [0.0, -below, 0.0]])
    local = api.edit_local_matrices(np.eye(4), eye)
    assert R.transform(p, local[0])[0, 0] == 0.5 and R.transform(p, local[0])[2, 0] == -0.5 and R.transform(p, local[0])[3, 2] == 0.5
    pairs, _ = api.edit_select(_exact(api, ctx, [p]), eye, api.EDIT_BOX, model_matrix=np.eye(4))
    np.testing.assert_array_equal(pairs[:, 1], [1, 4, 5])
    # sphere: squared norm == 1
    p = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.5, 0.5, 0.5], [np.nextafter(1.0, 0.0), 0.0, 0.0], [0.0, 0.0, np.nextafter(1.0, 2.0)]])
    assert (R.sq3(R.transform(p, local[0]))[:2] == 1.0).all()
    pairs, _ = api.edit_select(_exact(api, ctx, [p]), eye, api.EDIT_SPHERE, model_matrix=np.eye(4))
    np.testing.assert_array_equal(pairs[:, 1], [2, 3])
    # ball: qq == r r
    r = 2.0
    p = R.CENTER + np.array([[r, 0.0, 0.0], [r - 2.0**-40, 0.0, 0.0], [0.0, -r, 0.0], [0.0, 0.0, 1.0]])  # (2^-40 survives the sum with the centre)
    qq = R.center_qq(R.transform(p, np.eye(4)), R.CENTER)
    assert qq[0] == r * r and qq[2] == r * r and qq[1] < r * r
    pairs, _ = api.edit_select(_exact(api, ctx, [p]), eye, api.EDIT_WINDOW_BALL, center=R.CENTER, radius=r)
    np.testing.assert_array_equal(pairs[:, 1], [1, 3])
    # window: resolution 2, 5 cells to either side of the centre's cell (10, -7, 1): x cells 5 .. 15, y cells -12 .. -2, z cells -4 .. 6
    c = R.CENTER
    p = np.array([[32.0, c[1], c[2]], [np.nextafter(32.0, 0.0), c[1], c[2]], [10.0, c[1], c[2]], [np.nextafter(10.0, 0.0), c[1], c[2]],
                  [c[0], -24.0, c[2]], [c[0], np.nextafter(-24.0, -30.0), c[2]], [c[0], -2.0, c[2]], [c[0], np.nextafter(-2.0, -3.0), c[2]],
                  [c[0], c[1], -8.0], [c[0], c[1], np.nextafter(-8.0, -9.0)]])
    cells = np.floor(p * (1.0 / 2.0))
    centre = np.floor(c / 2.0)
    assert (centre == [10, -7, 1]).all()
    assert cells[0, 0] == centre[0] + 6 and cells[3, 0] == centre[0] - 6  # one past the window on either side
    assert cells[5, 1] == centre[1] - 6 and cells[5, 1] == -13 and cells[6, 1] == centre[1] + 6 and cells[6, 1] == -1  # floor below zero
    assert cells[9, 2] == centre[2] - 6 and cells[9, 2] == -5
    want, _ = R.select([p], eye, R.WINDOW, c)
    np.testing.assert_array_equal(want[:, 1], [1, 2, 4, 7, 8])
    pairs, _ = api.edit_select(_exact(api, ctx, [p]), eye, api.EDIT_WINDOW, center=c)
    np.testing.assert_array_equal(pairs, want)


# ---- outliers ----------------------------------------------------------------------------------------------------------------------------------------
def test_outliers_in_a_radius_equal_the_restatement(scene, ctx, orc):
    from glim_amd import api

    rng = np.random.default_rng(5)
    clutter = R.CENTER + rng.uniform(-0.9, 0.9, size=(30, 3))
    clouds = scene["clouds"] + [clutter]
    poses = scene["poses"] + [np.eye(4)]
    gpu = scene["gpu"] + [api.clone_exact(clutter, ctx=ctx)]
    radius, offset, k, thresh = 0.9, 0.4, 10, 2.0
    want, status, w = R.select_outliers(orc, clouds, poses, R.CENTER, radius, offset, k, thresh)
    # a condition on the scene, not a tolerance: no mean neighbour distance sits where the order of the sum of the d_i could turn a decision
    margin = R.outlier_margin(w, k, thresh)
    print("candidates", len(w), "outliers", len(want), "smallest |d_i - threshold| / threshold", margin)
    assert margin > 1e-9
    assert status == "ok" and len(want) > 0
    inner, _ = R.select(clouds, poses, R.WINDOW_BALL, R.CENTER, radius)
    assert len(inner) < len(w)  # points between r and r + offset take part in the statistic
    pairs, count, st = api.edit_select_outliers(gpu, poses, R.CENTER, radius, offset, k, thresh)
    assert st == "ok" and count == len(want)
    np.testing.assert_array_equal(pairs, want)
    part, count2, _ = api.edit_select_outliers(gpu, poses, R.CENTER, radius, offset, k, thresh, capacity=2)
    assert count2 == count
    np.testing.assert_array_equal(part, want[:2])
    # fewer candidates than k: nothing, and a status
    far = R.CENTER + np.array([1.25, 1.25, 1.25])
    few, _ = R.select(clouds, poses, R.WINDOW_BALL, far, 0.2 + 0.1)
    assert len(few) < k
    pairs, count, st = api.edit_select_outliers(gpu, poses, far, 0.2, 0.1, k, thresh)
    assert st == "few_points" and count == 0 and len(pairs) == 0


# ---- region growing ----------------------------------------------------------------------------------------------------------------------------------
def test_region_growing_on_the_scene_equals_the_restatement(scene, normal_scene):
    from glim_amd import api

    prm = api.RegionGrowingParams(distance_threshold=THR, dilation_radius=0.25)
    want = R.region_grow(scene["clouds"], scene["poses"], R.CENTER, THR, dilation_radius=0.25)
    got = api.edit_region_grow(scene["gpu"], scene["poses"], R.CENTER, prm)
    print("without normals: candidates", want["num_candidates"], "cluster", want["count"], "rounds", want["rounds"], "levels", np.bincount(want["levels"]))
    assert want["rounds"] >= 3 and want["count"] < want["num_candidates"] and (want["levels"] == want["rounds"] + 1).any()
    _same_region(got, want)
    # capacity below the count: the prefix, and the true count
    part = api.edit_region_grow(scene["gpu"], scene["poses"], R.CENTER, prm, capacity=10)
    assert part["count"] == want["count"]
    np.testing.assert_array_equal(part["pairs"], want["pairs"][:10])
    np.testing.assert_array_equal(part["levels"], want["levels"][:10])
    # with normals
    ns = normal_scene
    prm = api.RegionGrowingParams(distance_threshold=THR, angle_threshold=np.deg2rad(10.0), dilation_radius=0.0, use_normals=True)
    want = R.region_grow(ns["clouds"], ns["poses"], R.CENTER, THR, cos_angle=prm.cos_angle_threshold(), normals=ns["normals"], dilation_radius=0.0)
    plain = R.region_grow(ns["clouds"], ns["poses"], R.CENTER, THR, dilation_radius=0.0)
    print("with normals: cluster", want["count"], "rounds", want["rounds"], "against", plain["count"], "without")
    assert 1 < want["count"] < plain["count"]
    _same_region(api.edit_region_grow(ns["gpu"], ns["poses"], R.CENTER, prm), want)
    # use_normals on clouds without normals
    with pytest.raises(api.GlimAmdError) as e:
        api.edit_region_grow(scene["gpu"], scene["poses"], R.CENTER, prm)
    assert e.value.code == -5


def test_a_chain_longer_than_two_looks_is_reached_to_its_last_point(ctx):
    from glim_amd import api

    n = 2 * api.EDIT_ROUNDS_PER_LOOK + 5
    thr = 0.2
    step = 0.9 * thr / np.sqrt(3.0)
    p = R.CENTER + step * np.arange(n)[:, None] * np.ones(3)
    d = np.sqrt(R.sq3(p[1:] - p[:-1]))
    assert (d < thr).all() and (np.sqrt(R.sq3(p[2:] - p[:-2])) > thr).all()
    got = api.edit_region_grow(_exact(api, ctx, [p]), [np.eye(4)], R.CENTER, api.RegionGrowingParams(distance_threshold=thr, dilation_radius=0.0))
    assert got["count"] == n and got["rounds"] == n - 1 and got["seed"] == (0, 0)
    np.testing.assert_array_equal(got["pairs"][:, 1], np.arange(n))
    np.testing.assert_array_equal(got["levels"], np.arange(n))
    _same_region(got, R.region_grow([p], [np.eye(4)], R.CENTER, thr, dilation_radius=0.0))


def test_a_distance_equal_to_the_threshold_is_no_edge(ctx):
    from glim_amd import api

    g = np.arange(4.0)
    p = np.array([20.0, -13.0, 3.0]) + np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    picked = p[0]
    gpu = _exact(api, ctx, [p])
    alone = api.edit_region_grow(gpu, [np.eye(4)], picked, api.RegionGrowingParams(distance_threshold=1.0, dilation_radius=0.0))
    assert alone["count"] == 1 and alone["rounds"] == 0 and alone["seed"] == (0, 0) and alone["seed_qq"] == 0.0
    thr = np.nextafter(1.0, 2.0)
    whole = api.edit_region_grow(gpu, [np.eye(4)], picked, api.RegionGrowingParams(distance_threshold=thr, dilation_radius=0.0))
    assert whole["count"] == 64 and whole["rounds"] == 9
    np.testing.assert_array_equal(whole["levels"], (p - picked).sum(axis=1).astype(np.int32))  # the hop count on a lattice: the Manhattan distance
    _same_region(whole, R.region_grow([p], [np.eye(4)], picked, thr, dilation_radius=0.0))


def test_a_second_blob_is_excluded_and_dilation_takes_exactly_its_bridging_points(ctx):
    from glim_amd import api

    rng = np.random.default_rng(3)
    a = R.CENTER + rng.uniform(-0.2, 0.2, size=(120, 3))
    b = R.CENTER + np.array([0.7, 0.0, 0.0]) + rng.uniform(-0.2, 0.2, size=(120, 3))  # a gap of at least 0.3 along x
    a[0] = R.CENTER
    clouds, poses = [a, b], [np.eye(4), np.eye(4)]
    gpu = _exact(api, ctx, clouds)
    want = R.region_grow(clouds, poses, R.CENTER, THR, dilation_radius=0.0)
    got = api.edit_region_grow(gpu, poses, R.CENTER, api.RegionGrowingParams(distance_threshold=THR, dilation_radius=0.0))
    _same_region(got, want)
    assert got["num_candidates"] == 240 and got["count"] > 60 and (got["pairs"][:, 0] == 0).all()
    want = R.region_grow(clouds, poses, R.CENTER, THR, dilation_radius=0.38)
    got = api.edit_region_grow(gpu, poses, R.CENTER, api.RegionGrowingParams(distance_threshold=THR, dilation_radius=0.38))
    _same_region(got, want)
    bridged = got["pairs"][:, 0] == 1
    print("bridging points", int(bridged.sum()), "of 120, at level", got["rounds"] + 1)
    assert 0 < bridged.sum() < 120 and (got["levels"][bridged] == got["rounds"] + 1).all()


def test_an_isolated_seed_and_an_empty_window(scene):
    from glim_amd import api

    gpu, poses = scene["gpu"], scene["poses"]
    alone = api.edit_region_grow(gpu, poses, R.CENTER, api.RegionGrowingParams(distance_threshold=1e-4, dilation_radius=0.0))
    assert alone["count"] == 1 and alone["rounds"] == 0 and alone["status"] == "ok" and list(alone["levels"]) == [0]
    _same_region(alone, R.region_grow(scene["clouds"], poses, R.CENTER, 1e-4, dilation_radius=0.0))
    empty = api.edit_region_grow(gpu, poses, [1000.0, 1000.0, 1000.0])
    assert empty["count"] == 0 and empty["num_candidates"] == 0 and empty["status"] == "empty" and empty["seed"] == (-1, -1) and len(empty["pairs"]) == 0


def test_max_hops_cuts_by_level_and_two_calls_give_identical_arrays(scene):
    from glim_amd import api

    gpu, poses = scene["gpu"], scene["poses"]
    for dilation in (0.0, 0.1):
        want = R.region_grow(scene["clouds"], poses, R.CENTER, THR, dilation_radius=dilation, max_hops=3)
        prm = api.RegionGrowingParams(distance_threshold=THR, dilation_radius=dilation, max_hops=3)
        got = api.edit_region_grow(gpu, poses, R.CENTER, prm)
        assert want["rounds"] == 3 and want["levels"].max() == (4 if dilation else 3)
        _same_region(got, want)
        again = api.edit_region_grow(gpu, poses, R.CENTER, prm)
        assert got["pairs"].tobytes() == again["pairs"].tobytes() and got["levels"].tobytes() == again["levels"].tobytes()
    full = R.region_grow(scene["clouds"], poses, R.CENTER, THR, dilation_radius=0.0)
    cut = R.region_grow(scene["clouds"], poses, R.CENTER, THR, dilation_radius=0.0, max_hops=3)
    np.testing.assert_array_equal(cut["pairs"], full["pairs"][full["levels"] <= 3])


# ---- removal -------------------------------------------------------------------------------------------------------------------------------------------
def _no_neighbors(cloud):
    from glim_amd import _lib

    nb = np.zeros(max(cloud.size(), 1) * 32, dtype=np.int32)
    return _lib.lib().glim_amd_cloud_download(cloud._h, None, None, None, nb.ctypes.data_as(C.POINTER(C.c_int32))) == -5  # GLIM_AMD_ERR_STATE


def _indices(rng, n):
    idx = rng.choice(n, size=n // 3, replace=False)
    return np.concatenate([idx, idx[:7], [n - 1, 0]]).astype(np.int32)  # unsorted, with duplicates, both ends


def test_removal_gathers_every_array_of_a_covariance_estimated_cloud(ctx, small_pair):
    from glim_amd import api

    rng = np.random.default_rng(0)
    pts = small_pair["source"]["points"].astype(np.float32)
    cloud = api.PointCloudGPU.clone(pts, ctx=ctx)
    cloud.find_neighbors(10, download=False)
    cloud.estimate_covariances(10)
    before = cloud.download()
    n = cloud.size()
    idx = _indices(rng, n)
    new = api.edit_remove_points(cloud, idx)
    keep = np.ones(n, dtype=bool)
    keep[idx] = False
    assert new.size() == keep.sum() and 0 < new.size() < n
    for got, old, again in zip(new.download(), before, cloud.download()):
        assert got.tobytes() == old[keep].tobytes()
        assert again.tobytes() == old.tobytes()  # the input cloud is untouched
    assert _no_neighbors(new) and not _no_neighbors(cloud)
    # an index == size is refused; removing everything gives a valid empty cloud
    with pytest.raises(api.GlimAmdError) as e:
        api.edit_remove_points(cloud, [0, n])
    assert e.value.code == -1
    with pytest.raises(api.GlimAmdError):
        api.edit_remove_points(cloud, [-1])
    empty = api.edit_remove_points(cloud, np.arange(n))
    assert empty.size() == 0 and all(len(a) == 0 for a in empty.download())
    same = api.edit_remove_points(cloud, [])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(same.download(), before))
    # the edited cloud as the source of a VGICP factor: the same bits as a cloud freshly created from the same kept arrays
    t = small_pair["target"]
    vm = api.GaussianVoxelMapGPU(0.5, ctx=ctx).insert(api.PointCloudGPU.clone(t["points"].astype(np.float64), t["covs"], ctx=ctx))
    fresh = api.PointCloudGPU.clone(before[0][keep], before[1][keep], before[2][keep], ctx=ctx)
    out = []
    for src in (new, fresh):
        fset = api.NonlinearFactorSetGPU(ctx)
        fset.add(api.IntegratedVGICPFactorGPU(np.eye(4), 1, vm, src))
        out.append(fset.linearize({1: small_pair["delta"]})[0])
    assert out[0]["num_inliers"] == out[1]["num_inliers"] > 100
    for k in ("error", "H_ss", "b_s"):
        assert np.asarray(out[0][k]).tobytes() == np.asarray(out[1][k]).tobytes(), k


def test_removal_of_a_preprocessed_and_of_a_merged_cloud(ctx):
    from glim_amd import api

    rng = np.random.default_rng(1)
    # preprocessed: exact points, times, intensities (and the host copy of the times, which deskewing needs)
    raw = rng.uniform(-20.0, 20.0, size=(3000, 3))
    # voxels far smaller than the point spacing and stamps 2e-4 s apart: no two points are averaged, and every point is a time-table entry
    # of its own in the deskewing (which merges stamps within 1e-4 s), so that a point's deskewed position does not depend on the others
    prm = api.preprocess_params(downsample_resolution=0.01, k_correspondences=5)
    pre = api.PointCloudGPU.preprocess(raw, rng.permutation(3000) * 2e-4, rng.uniform(0.0, 255.0, size=3000), prm, ctx=ctx)
    before = pre.download_frame()
    n = pre.size()
    idx = _indices(rng, n)
    keep = np.ones(n, dtype=bool)
    keep[idx] = False
    new = api.edit_remove_points(pre, idx)
    after, again = new.download_frame(), pre.download_frame()
    assert new.size() == keep.sum() and after["neighbors"] is None and _no_neighbors(new)
    for k in ("points", "times", "intensities"):
        assert after[k].tobytes() == before[k][keep].tobytes(), k
        assert again[k].tobytes() == before[k].tobytes(), k
    assert new.download(covs=False, normals=False)[0].tobytes() == pre.download(covs=False, normals=False)[0][keep].tobytes()
    vel = dict(linear_vel=[1.0, 0.5, 0.0], angular_vel=[0.0, 0.1, 0.3])
    assert new.deskew(np.eye(4), **vel).download_points64().tobytes() == pre.deskew(np.eye(4), **vel).download_points64()[keep].tobytes()
    # merged: exact points and exact covariances
    frames = [rng.uniform(-5.0, 5.0, size=(700, 3)) for _ in range(2)]
    A = rng.normal(size=(2, 700, 3, 3))
    covs = [a @ np.transpose(a, (0, 2, 1)) * 0.01 + 1e-3 * np.eye(3) for a in A]
    merged = api.merge_frames([np.eye(4), np.eye(4)], frames, covs, 0.25, ctx=ctx)
    mp, mc = merged.download_merged()
    n = merged.size()
    idx = _indices(rng, n)
    keep = np.ones(n, dtype=bool)
    keep[idx] = False
    new = api.edit_remove_points(merged, idx)
    np_, nc = new.download_merged()
    assert np_.tobytes() == mp[keep].tobytes() and nc.tobytes() == mc[keep].tobytes() and len(np_) == keep.sum() > 100
    for got, old in zip(new.download(normals=False)[:2], merged.download(normals=False)[:2]):  # the FP32 points and covariances
        assert len(got) == keep.sum() and got.tobytes() == old[keep].tobytes()
    mp2, mc2 = merged.download_merged()
    assert mp2.tobytes() == mp.tobytes() and mc2.tobytes() == mc.tobytes()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------
def test_grow_a_blob_remove_it_and_select_again(scene):
    from glim_amd import api

    gpu, poses = scene["gpu"], scene["poses"]
    grown = api.edit_region_grow(gpu, poses, R.CENTER, api.RegionGrowingParams(distance_threshold=THR, dilation_radius=0.0, max_hops=4))
    touched = sorted(set(grown["pairs"][:, 0].tolist()))
    assert grown["count"] > 20 and 3 not in touched
    edited = api.edit_remove_selected(gpu, grown["pairs"])
    for s in range(4):
        assert (edited[s] is gpu[s]) == (s not in touched)  # the untouched sub-maps' handles are returned unchanged
    radius = 1.0
    before, _ = api.edit_select(gpu, poses, api.EDIT_WINDOW_BALL, center=R.CENTER, radius=radius)
    after, count = api.edit_select(edited, poses, api.EDIT_WINDOW_BALL, center=R.CENTER, radius=radius)
    # what is left are the old ball's points that were not grown, renumbered inside their sub-maps by the removal
    ids, removed = R.pack_ids(before), R.pack_ids(grown["pairs"])
    assert np.isin(removed, ids).all()  # the blob lies inside the ball
    left = before[~np.isin(ids, removed)]
    assert count == len(left) == len(before) - grown["count"]
    want = left.copy()
    for s in touched:
        gone = np.sort(grown["pairs"][grown["pairs"][:, 0] == s, 1])
        rows = want[:, 0] == s
        want[rows, 1] -= np.searchsorted(gone, want[rows, 1]).astype(np.int32)
    np.testing.assert_array_equal(after, want)
    # no removed point remains: the edited clouds' world points against the removed points' world points
    clouds = scene["clouds"]
    removed_w = np.concatenate([R.transform(clouds[s][grown["pairs"][grown["pairs"][:, 0] == s, 1]], poses[s]) for s in touched])
    kept_w = np.concatenate([R.transform(R.remove(clouds[s], grown["pairs"][grown["pairs"][:, 0] == s, 1]), poses[s]) for s in range(4)])
    assert not (kept_w[:, None, :] == removed_w[None, :, :]).all(axis=2).any()
    for s in touched:
        assert edited[s].size() == len(clouds[s]) - int((grown["pairs"][:, 0] == s).sum())
