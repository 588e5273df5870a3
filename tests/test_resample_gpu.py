"""Resampling of resident clouds on the device (glim_amd/csrc/resample.hip) against the NumPy restatement (tests/resample_restatement.py).
Every comparison is an equality: the selection is a total order on integers, the gathers copy bits, and the transform is FP64 in a stated
operation order.

Four kinds of cloud: `f32` (FP32 points only), `est` (FP32 points whose covariances and normals were estimated on the device: plane form,
factor streams and neighbour lists present), `exact` (a preprocessed cloud: exact FP64 points, times, intensities and the host copy of the
times) and `merged` (a merged sub-map: exact FP64 points and covariances).  The sizes of `exact` and `merged` clouds are decided by the
preprocessing and the merge, and a neighbour search needs spread-out points, so the small sizes of those kinds (and of `est` below 1000) are
cut from a larger cloud with edit_remove_points, which tests/test_map_edit_gpu.py checks on its own.
"""
import functools

import numpy as np
import pytest

import resample_restatement as R

pytestmark = pytest.mark.gpu

SCAN_TILE = 4096  # glim_amd/csrc/scan.hpp
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000, SCAN_TILE + 1)
SEEDS = (0, 0x9E3779B97F4A7C15)
KINDS = ("f32", "est", "exact", "merged")
BELOW_SIZE = 49  # none of SIZES has a target for which n * (target / n) lands below the target in FP64; 49 has several (49 * (1 / 49) < 1)


@pytest.fixture(scope="module")
def ctx():
    from glim_amd import api

    return api.Context(0, 1)


@functools.lru_cache(maxsize=None)
def _keys(seed):
    return R.keys(SCAN_TILE + 1, seed)


def _indices(n, rate, seed):
    """R.random_sample_indices with the keys computed once per seed"""
    m = R.count(n, rate)
    if m >= n:
        return np.arange(n, dtype=np.int64)
    order = np.lexsort((np.arange(n), _keys(seed)[:n]))
    return np.sort(order[:m]).astype(np.int64)


def _target_rate(n):
    """target / n for a target at which n * (target / n) lands just below target, where n has one; else a third"""
    for t in range(1, n):
        if float(t) / float(n) < R.FULL_RATE and float(n) * (float(t) / float(n)) < float(t):
            return float(t) / float(n), True
    return float(max(1, n // 3)) / float(max(n, 1)), False


# ---- the four kinds of cloud -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bases(ctx):
    """per kind: the host data the clouds are made of, and the large cloud the small ones are cut from"""
    from glim_amd import api, synth

    rng = np.random.default_rng(11)
    scene = synth.Scene.default()
    scan = synth.scan(scene, synth.arc_trajectory(2)[1], synth.lidar_directions(48, 160), frame_id=1)
    assert len(scan) > SCAN_TILE
    scan = scan[np.sort(rng.choice(len(scan), size=SCAN_TILE + 1, replace=False))].astype(np.float32)
    out = {"f32": scan}
    for n in (1000, SCAN_TILE + 1):
        c = api.PointCloudGPU.clone(scan[np.sort(rng.choice(len(scan), size=n, replace=False))], ctx=ctx)
        c.find_neighbors(10, download=False)
        c.estimate_covariances(10)
        out[("est", n)] = c
    raw = rng.uniform(-20.0, 20.0, size=(6000, 3))
    # voxels far smaller than the point spacing and stamps 2e-4 s apart: no two points are averaged, and every point is a time-table entry
    # of its own in the deskewing, so that a point's deskewed position does not depend on the others
    prm = api.preprocess_params(downsample_resolution=0.01, k_correspondences=5)
    out["exact"] = api.PointCloudGPU.preprocess(raw, rng.permutation(6000) * 2e-4, rng.uniform(0.0, 255.0, size=6000), prm, ctx=ctx)
    frames = [rng.uniform(-8.0, 8.0, size=(3000, 3)) for _ in range(2)]
    A = rng.normal(size=(2, 3000, 3, 3))
    covs = [a @ np.transpose(a, (0, 2, 1)) * 0.01 + 1e-3 * np.eye(3) for a in A]
    out["merged"] = api.merge_frames([np.eye(4), np.eye(4)], frames, covs, 0.25, ctx=ctx)
    assert out["exact"].size() > SCAN_TILE and out["merged"].size() > SCAN_TILE
    return out


def _cut(api, cloud, n):
    return cloud if cloud.size() == n else api.edit_remove_points(cloud, np.arange(n, cloud.size()))


def _make(api, ctx, bases, kind, n):
    if kind == "f32":
        return api.PointCloudGPU.clone(bases["f32"][:n], ctx=ctx)
    if kind == "est":
        return bases[("est", n)] if ("est", n) in bases else _cut(api, bases[("est", 1000)], n)
    return _cut(api, bases[kind], n)


def _arrays(cloud, kind):
    """every array of the cloud that can be downloaded"""
    out = {"xyz": cloud.download(covs=False, normals=False)[0]}
    if kind == "est":
        _, out["covs"], out["normals"] = cloud.download()
    elif kind == "exact":
        f = cloud.download_frame()
        out["points64"], out["times"], out["intensities"] = f["points"], f["times"], f["intensities"]
    elif kind == "merged":
        out["covs"] = cloud.download(normals=False)[1]
        out["points64"], out["covs64"] = cloud.download_merged()
    return out


def _same(got, want, equal_nan=False):
    assert got.keys() == want.keys()
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        if equal_nan:
            assert np.array_equal(got[k], want[k], equal_nan=True), k
        else:
            assert got[k].tobytes() == want[k].tobytes(), k


def _gather(arrays, idx):
    return {k: v[idx] for k, v in arrays.items()}


def _no_neighbors(cloud):
    import ctypes as C

    from glim_amd import _lib

    nb = np.zeros(max(cloud.size(), 1) * 32, dtype=np.int32)
    return _lib.lib().glim_amd_cloud_download(cloud._h, None, None, None, nb.ctypes.data_as(C.POINTER(C.c_int32))) == -5  # GLIM_AMD_ERR_STATE


# ---- the selection on supplied keys --------------------------------------------------------------------------------------------------------------------
def _key_sets(rng, n):
    yield "equal", np.full(n, 0x80000001, dtype=np.uint32)
    yield "two values", np.where(rng.random(n) < 0.5, 7, 0xFFE00007).astype(np.uint32)
    k = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    k[rng.integers(0, n, size=max(1, n // 8))] = 0
    k[rng.integers(0, n, size=max(1, n // 8))] = 0xFFFFFFFF
    yield "ends", k
    yield "alphabet", rng.choice(np.array([0, 0x00000400, 0x00200000, 0xFFFFFFFF], dtype=np.uint32), size=n)
    yield "random", rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)


def test_selection_on_supplied_keys_equals_the_restatement(ctx):
    from glim_amd import api

    rng = np.random.default_rng(5)
    compared = ties = 0
    for n in SIZES:
        for name, keys in _key_sets(rng, n):
            for m in sorted({0, 1, n // 2, n - 1, n}):
                want = R.select_smallest(keys, m)
                got = api.debug_select_smallest(keys, m, ctx=ctx)
                assert got.dtype == np.int32 and got.tobytes() == want.tobytes(), (n, name, m)
                compared += 1
                if 0 < m < n:  # the threshold key is held by kept and by dropped points: the tie rank decided
                    t = np.sort(keys, kind="stable")[m - 1]
                    ties += int((keys[want == 1] == t).any() and (keys[want == 0] == t).any())
    assert ties >= 24  # equal keys alone: 8 sizes above 1, three values of m strictly between 0 and n
    print("selections compared:", compared, "with a tie cut at the threshold:", ties)
    assert len(api.debug_select_smallest(np.zeros(0, dtype=np.uint32), 0, ctx=ctx)) == 0
    with pytest.raises(api.GlimAmdError) as e:
        api.debug_select_smallest(np.zeros(4, dtype=np.uint32), 5, ctx=ctx)
    assert e.value.code == -1


# ---- random_sampling -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_random_sampling_gathers_every_array_at_the_restatements_indices(ctx, bases, kind):
    from glim_amd import api

    below = 0
    for n in (0,) + SIZES + (BELOW_SIZE,):
        cloud = _make(api, ctx, bases, kind, n)
        assert cloud.size() == n
        before = _arrays(cloud, kind)
        target_rate, is_below = _target_rate(n)
        below += is_below
        for rate in (0.0, 1e-9, 0.1, 0.5, 0.98, 0.99, 1.0, 3.0, target_rate):
            for seed in SEEDS:
                idx = _indices(n, rate, seed)
                new = cloud.random_sampling(rate, seed)
                assert new.size() == len(idx) == R.count(n, rate), (n, rate, seed)
                _same(_arrays(new, kind), _gather(before, idx))
                assert _no_neighbors(new)
        _same(_arrays(cloud, kind), before)  # the input is untouched
        if n == 1000:  # the result outlives its input
            new = cloud.random_sampling(0.5, 3)
            if cloud is not bases.get(kind) and cloud is not bases.get((kind, n)):
                cloud.close()
            _same(_arrays(new, kind), _gather(before, _indices(n, 0.5, 3)))
    assert below == 1 and R.count(BELOW_SIZE, _target_rate(BELOW_SIZE)[0]) == round(_target_rate(BELOW_SIZE)[0] * BELOW_SIZE) - 1
    with pytest.raises(api.GlimAmdError) as e:
        _make(api, ctx, bases, kind, 64).random_sampling(float("nan"))
    assert e.value.code == -1
    for bad in (-0.5, float("inf")):
        with pytest.raises(api.GlimAmdError):
            _make(api, ctx, bases, kind, 64).random_sampling(bad)


def test_sampled_preprocessed_cloud_keeps_the_host_times_the_deskewing_reads(ctx, bases):
    from glim_amd import api

    pre = _make(api, ctx, bases, "exact", SCAN_TILE + 1)
    vel = dict(linear_vel=[1.0, 0.5, 0.0], angular_vel=[0.0, 0.1, 0.3])
    want = pre.deskew(np.eye(4), **vel).download_points64()
    idx = _indices(pre.size(), 0.5, 1)
    assert pre.random_sampling(0.5, 1).deskew(np.eye(4), **vel).download_points64().tobytes() == want[idx].tobytes()
    # ascending indices: the deskewing builds its time table from stamps in ascending order (a permuted cloud is no scan)
    perm = np.sort(np.random.default_rng(2).permutation(pre.size())[:777])
    assert pre.sample(perm).deskew(np.eye(4), **vel).download_points64().tobytes() == want[perm].tobytes()
    assert pre.transform(np.eye(4)).deskew(np.eye(4), **vel).download_points64().tobytes() == want.tobytes()


# ---- sample --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_sample_gathers_every_array_in_the_order_of_the_indices(ctx, bases, kind):
    from glim_amd import api

    rng = np.random.default_rng(7)
    for n in (257, 1000):
        cloud = _make(api, ctx, bases, kind, n)
        before = _arrays(cloud, kind)
        cases = {"permutation": rng.permutation(n), "reversed": np.arange(n)[::-1], "duplicates": rng.integers(0, n, size=n // 2),
                 "more than n": rng.integers(0, n, size=2 * n + 3), "empty": np.zeros(0, dtype=np.int64)}
        for name, idx in cases.items():
            new = cloud.sample(idx)
            assert new.size() == len(idx), name
            _same(_arrays(new, kind), _gather(before, idx))
            assert _no_neighbors(new)
        # removal is the sample of the ascending complement
        drop = rng.choice(n, size=n // 3, replace=False)
        keep = np.setdiff1d(np.arange(n), drop)
        _same(_arrays(api.edit_remove_points(cloud, drop), kind), _arrays(cloud.sample(keep), kind))
        _same(_arrays(cloud, kind), before)
        for bad in ([0, n], [-1]):
            with pytest.raises(api.GlimAmdError) as e:
                cloud.sample(bad)
            assert e.value.code == -1


# ---- transform -----------------------------------------------------------------------------------------------------------------------------------------
def _poses():
    c, s = np.cos(0.7), np.sin(0.7)
    rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    c, s = np.cos(-0.3), np.sin(-0.3)
    rx = np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
    rigid = np.eye(4)
    rigid[:3, :3], rigid[:3, 3] = rz @ rx, [21.5, -19.25, 3.125]
    shear = np.eye(4)
    shear[:3, :4] = [[1.5, 0.25, -0.125, 1.0], [0.0, -2.0, 0.5, -3.0], [0.75, 0.0, 0.3, 20.0]]
    return {"rigid": rigid, "identity": np.eye(4), "non-rigid": shear}


def _transformed(arrays, kind, T):
    """the restatement applied to downloaded arrays: FP64 arrays where the kind holds them, the FP32 ones their roundings"""
    n = len(arrays["xyz"])
    out = dict(arrays)
    with np.errstate(all="ignore"):
        if "points64" in arrays:
            p = np.concatenate([arrays["points64"], np.ones((n, 1))], axis=1)
        else:
            p = np.concatenate([arrays["xyz"].astype(np.float64), np.ones((n, 1))], axis=1)
        c6 = None
        if "covs64" in arrays:
            c6 = R.cov6(arrays["covs64"])
        elif "covs" in arrays:
            c6 = R.cov6(arrays["covs"].astype(np.float64))
        nr = arrays["normals"].astype(np.float64) if "normals" in arrays else None
        q, d, m = R.transform(p, c6, nr, T)
        out["xyz"] = q[:, :3].astype(np.float32)
        if "points64" in arrays:
            out["points64"] = q[:, :3].copy()
        if "covs64" in arrays:
            out["covs64"] = R.cov33(d)
        if "covs" in arrays:
            out["covs"] = R.cov33(d).astype(np.float32)
        if nr is not None:
            out["normals"] = m.astype(np.float32)
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_transform_equals_the_restatement_on_every_array(ctx, bases, kind):
    from glim_amd import api

    for n in (0, 257, 1000):
        cloud = _make(api, ctx, bases, kind, n)
        before = _arrays(cloud, kind)
        for name, T in _poses().items():
            new = cloud.transform(T)
            assert new.size() == n
            got = _arrays(new, kind)
            _same(got, _transformed(before, kind, T))
            if name == "identity":
                _same(got, before)  # bit-identical arrays back
            assert _no_neighbors(new)
        _same(_arrays(cloud, kind), before)
    with pytest.raises(api.GlimAmdError) as e:
        T = np.eye(4)
        T[1, 3] = np.inf
        cloud.transform(T)
    assert e.value.code == -1


def test_transform_of_points_that_are_not_finite_gives_what_the_expression_gives(ctx, bases):
    from glim_amd import api

    pts = bases["f32"][:300].copy()
    pts[17, 1], pts[200, 2] = np.nan, np.inf
    cloud = api.PointCloudGPU.clone(pts, ctx=ctx)
    before = _arrays(cloud, "f32")
    for T in _poses().values():
        got = _arrays(cloud.transform(T), "f32")
        want = _transformed(before, "f32", T)
        _same(got, want, equal_nan=True)
        assert np.isnan(want["xyz"]).any() and np.isfinite(want["xyz"]).sum() >= 3 * 298


# ---- members a cloud builds on first use are not carried over ---------------------------------------------------------------------------------------------
def _linearize(api, ctx, vm, src, delta):
    fset = api.NonlinearFactorSetGPU(ctx)
    fset.add(api.IntegratedVGICPFactorGPU(np.eye(4), 1, vm, src))
    return fset.linearize({1: delta})[0]


def _same_factor(a, b):
    assert a["num_inliers"] == b["num_inliers"] > 100
    for k in ("error", "H_ss", "b_s"):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_factor_over_a_derived_cloud_has_the_bits_of_one_over_a_clone_of_its_arrays(ctx, bases, small_pair):
    from glim_amd import api

    src = bases[("est", SCAN_TILE + 1)]
    t = small_pair["target"]
    vm = api.GaussianVoxelMapGPU(0.5, ctx=ctx).insert(api.PointCloudGPU.clone(t["points"].astype(np.float64), t["covs"], ctx=ctx))
    delta = small_pair["delta"]
    _linearize(api, ctx, vm, src, delta)  # the input now holds its factor streams (and its neighbour lists, from the estimation)
    assert not _no_neighbors(src)
    before = _arrays(src, "est")
    # sampled: the plane form follows the input, the streams are the result's own
    idx = _indices(src.size(), 0.5, 9)
    new = src.random_sampling(0.5, 9)
    fresh = api.PointCloudGPU.clone(before["xyz"][idx], before["covs"][idx], before["normals"][idx], ctx=ctx)
    _same_factor(_linearize(api, ctx, vm, new, delta), _linearize(api, ctx, vm, fresh, delta))
    assert new.memory_usage_gpu() == fresh.memory_usage_gpu()  # the same arrays and the same form of streams
    # transformed: the plane form is decided on the result, as the clone decides it.  The non-rigid map of this test is a mild one, so that the
    # moved cloud still lies on the target
    mild = np.eye(4)
    mild[:3, :4] = [[1.01, 0.004, 0.0, 0.02], [0.0, 0.99, 0.003, -0.01], [0.002, 0.0, 1.005, 0.0]]
    poses = _poses()
    for name, T, pose in (("rigid", poses["rigid"], delta @ np.linalg.inv(poses["rigid"])), ("identity", np.eye(4), delta), ("non-rigid", mild, delta)):
        moved = src.transform(T)
        got = _arrays(moved, "est")
        fresh = api.PointCloudGPU.clone(got["xyz"], got["covs"], got["normals"], ctx=ctx)
        _same_factor(_linearize(api, ctx, vm, moved, pose), _linearize(api, ctx, vm, fresh, pose))
        assert moved.memory_usage_gpu() == fresh.memory_usage_gpu(), name
    _same(_arrays(src, "est"), before)
