"""Raw records and the host's rotation (switch host_rotate, vgicp.hip finalize_tail / finish_raw_records).

A synchronous linearisation of at most HOST_ROTATE_MAX_FACTORS factors through the single-dispatch form or the resident session returns the summed
accumulators and the host applies the R^T B R rotation and the slot mapping; larger sets, host_rotate=0 and the two-dispatch form rotate on the
device.  Every form has to return the same bits.  Shapes: the smallest at which the tail can go wrong -- 16 x 128 (fewer than 32 partial rows: some
of the finaliser's 32 groups have no row) and 64 x 512 (128 rows: every group, and both (group, piece) pairs of threads 0..63, in use)."""
import os
import re
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = np.array([0.002, -0.001, 0.003, 0.02, 0.01, -0.02])


@pytest.fixture(scope="module")
def api():
    from glim_amd import api as _api

    assert _api.device_count() >= 1
    return _api


@pytest.fixture(scope="module")
def ctx(api):
    return api.Context(0, 1)


def _host_rotate_max_factors():
    src = open(os.path.join(ROOT, "glim_amd", "csrc", "vgicp.hip")).read()
    m = re.search(r"^#define GLIM_AMD_HOST_ROTATE_MAX (\d+)$", src, re.M)
    assert m and "HOST_ROTATE_MAX_FACTORS = GLIM_AMD_HOST_ROTATE_MAX;" in src
    return int(m.group(1))


def _scan_pair(api, ctx, rings, azimuths):
    from glim_amd import synth

    scene = synth.Scene.default()
    dirs = synth.lidar_directions(rings, azimuths)
    poses = synth.arc_trajectory(2)
    tgt, src = synth.scan(scene, poses[0], dirs, 0), synth.scan(scene, poses[1], dirs, 1)
    tg, sg = api.PointCloudGPU.clone(tgt, ctx=ctx), api.PointCloudGPU.clone(src, ctx=ctx)
    for g in (tg, sg):
        g.find_neighbors(10, download=False)
        g.estimate_covariances(10)
    return tg, sg, synth.relative_pose(poses[0], poses[1])


def _same(L, B, what):
    assert L["num_inliers"] == B["num_inliers"], what
    for key in ("H_ss", "b_s", "H_tt", "H_ts", "b_t"):
        np.testing.assert_array_equal(L[key], B[key], err_msg=f"{what} {key}")
    assert L["error"] == B["error"], what


def _values(orc, delta, copies, rep):
    values = {0: np.eye(4)}
    for k in range(copies):
        values[1 + k] = delta @ orc.se3_exp(STEP * (1 + 0.1 * k + 0.05 * rep))
    return values


def _run_modes(api, ctx, orc, factors, delta, modes, reps=5):
    """reps calls with a moving pose in every mode (a fresh set per mode, each mode on top of the defaults): {mode: [records per call]}"""
    res = {}
    for mode in modes:
        with ctx.diag(mode):
            fset = api.NonlinearFactorSetGPU(ctx)
            for f in factors:
                fset.add(f)
            res[mode] = [fset.linearize(_values(orc, delta, len(factors), rep)) for rep in range(reps)]
            fset.close()
    return res


def _assert_modes_equal(res, reference):
    assert res[reference][0][0]["num_inliers"] > 100
    for mode, calls in res.items():
        for rep, (Ls, Bs) in enumerate(zip(calls, res[reference])):
            assert len(Ls) == len(Bs)
            for k, (L, B) in enumerate(zip(Ls, Bs)):
                _same(L, B, f"mode '{mode}' call {rep} factor {k}")


@pytest.mark.parametrize("rings,azimuths", [(16, 128), (64, 512)])
def test_single_factor_modes_give_identical_bits(api, ctx, orc, rings, azimuths):
    """One factor, unary and binary, 5 calls with a moving pose (calls 4 and 5 of a resident mode go through the session): raw records finished on
    the host (default, resident=1) against the device rotation (host_rotate=0) and the two-dispatch form (fuse=0)."""
    tg, sg, delta = _scan_pair(api, ctx, rings, azimuths)
    vm = api.GaussianVoxelMapGPU(0.5, ctx=ctx).insert(tg)
    try:
        for target in (0, np.eye(4)):
            factors = [api.IntegratedVGICPFactorGPU(target, 1, vm, sg)]
            res = _run_modes(api, ctx, orc, factors, delta, ("fuse=0", "", "host_rotate=0", "resident=1", "resident=1,host_rotate=0"))
            _assert_modes_equal(res, "fuse=0")
    finally:
        api.resident_stop(ctx)


def test_both_sides_of_the_threshold(api, ctx, orc):
    """Sets of HOST_ROTATE_MAX_FACTORS factors (raw records, host rotation) and of one more (device rotation), two voxel resolutions alternating,
    in the default mode and through the resident session, against the two-dispatch form."""
    nmax = _host_rotate_max_factors()
    assert nmax >= 1
    tg, sg, delta = _scan_pair(api, ctx, 16, 256)
    vms = [api.GaussianVoxelMapGPU(r, ctx=ctx).insert(tg) for r in (0.5, 1.0)]
    try:
        for copies in (nmax, nmax + 1):
            factors = [api.IntegratedVGICPFactorGPU(0, 1 + k, vms[k % 2], sg) for k in range(copies)]
            res = _run_modes(api, ctx, orc, factors, delta, ("fuse=0", "", "resident=1"))
            _assert_modes_equal(res, "fuse=0")
    finally:
        api.resident_stop(ctx)


def test_switch_flipped_under_a_live_session(api, ctx, orc):
    """The session's kernel keeps the record form it was launched with: flipping host_rotate under a live session restarts it, and every call is
    finished the way its producer was told to.  A record finished the wrong way would be wrong in every rotated slot; a lost row costs about a
    second, which the time bound would show."""
    t0 = time.monotonic()
    tg, sg, delta = _scan_pair(api, ctx, 16, 128)
    vm = api.GaussianVoxelMapGPU(0.5, ctx=ctx).insert(tg)
    factors = [api.IntegratedVGICPFactorGPU(0, 1, vm, sg)]
    poses = [_values(orc, delta, 1, rep) for rep in range(8)]
    with ctx.diag("fuse=0"):
        ref = api.NonlinearFactorSetGPU(ctx)
        ref.add(factors[0])
        want = [ref.linearize(v)[0] for v in poses]
        ref.close()
    assert want[0]["num_inliers"] > 100
    fset = api.NonlinearFactorSetGPU(ctx)
    fset.add(factors[0])
    try:
        api.resident_stop(ctx)
        served = []
        for group, mode in enumerate(("resident=1", "resident=1,host_rotate=0", "resident=1")):
            before = api.resident_stats(ctx)["requests"]
            with ctx.diag(mode):
                for rep, v in enumerate(poses):
                    _same(fset.linearize(v)[0], want[rep], f"group {group} ({mode}) call {rep}")
            served.append(api.resident_stats(ctx)["requests"] - before)
        # group 0: the plan's first three synchronous linearisations are launches (warm-up), the other five go through the session; group 2: all eight
        assert served[0] >= 5 and served[2] >= 8, served
    finally:
        api.resident_stop(ctx)
        fset.close()
    assert time.monotonic() - t0 < 20.0
