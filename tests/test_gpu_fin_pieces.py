"""One finalising block per record piece in a resident session (switch fin_pieces, vgicp.hip piece_finalize).

A session that returns raw records (at most HOST_ROTATE_MAX_FACTORS factors) finalises every factor in ten blocks, one per granule of a row; each
adds what fused_finalize + finalize_tail add, in the same order.  Every field of every record has to equal the two-dispatch launch-per-call form
(resident=0,fuse=0) and the session with one finalising block per factor (fin_pieces=0), bit for bit.  Shapes: 16 x 256 (16 rows: fewer than the
32 groups, chains of one row, idle poller threads), 64 x 512 (128 rows: chains of four) and 20 x 500 (a point count that is no multiple of 256
and a row count that is no multiple of 32: chains of unequal length)."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = np.array([0.002, -0.001, 0.003, 0.02, 0.01, -0.02])
WARMUP = 3  # synchronous linearisations of a plan that are launches before a session serves it (vgicp.hip RESIDENT_WARMUP)
BLOCK = 256


@pytest.fixture(scope="module")
def api():
    from glim_amd import api as _api

    assert _api.device_count() >= 1
    return _api


@pytest.fixture(scope="module")
def ctx(api):
    return api.Context(0, 1)


@pytest.fixture(scope="module")
def scans(api, ctx):
    """(rings, azimuths) -> (target cloud, source cloud, two voxel maps, relative pose), made once"""
    from glim_amd import synth

    made = {}

    def get(rings, azimuths):
        if (rings, azimuths) not in made:
            scene = synth.Scene.default()
            dirs = synth.lidar_directions(rings, azimuths)
            poses = synth.arc_trajectory(2)
            tgt, src = synth.scan(scene, poses[0], dirs, 0), synth.scan(scene, poses[1], dirs, 1)
            tg, sg = api.PointCloudGPU.clone(tgt, ctx=ctx), api.PointCloudGPU.clone(src, ctx=ctx)
            for g in (tg, sg):
                g.find_neighbors(10, download=False)
                g.estimate_covariances(10)
            vms = [api.GaussianVoxelMapGPU(r, ctx=ctx).insert(tg) for r in (0.5, 1.0)]
            made[(rings, azimuths)] = (tg, sg, vms, synth.relative_pose(poses[0], poses[1]))
        return made[(rings, azimuths)]

    return get


def _host_rotate_max_factors():
    src = open(os.path.join(ROOT, "glim_amd", "csrc", "vgicp.hip")).read()
    m = re.search(r"^#define GLIM_AMD_HOST_ROTATE_MAX (\d+)$", src, re.M)
    assert m and "HOST_ROTATE_MAX_FACTORS = GLIM_AMD_HOST_ROTATE_MAX;" in src
    return int(m.group(1))


def _same(L, B, what):
    assert L["num_inliers"] == B["num_inliers"], what
    for key in ("H_ss", "b_s", "H_tt", "H_ts", "b_t"):
        np.testing.assert_array_equal(L[key], B[key], err_msg=f"{what} {key}")
    assert L["error"] == B["error"], what


def _poses(orc, delta, copies, n=3):
    out = []
    for which in range(n):
        values = {0: np.eye(4)}
        for k in range(copies):
            values[1 + k] = delta @ orc.se3_exp(STEP * (1 + 0.1 * k + which))
        out.append(values)
    return out


def _reference(api, ctx, factors, poses):
    with ctx.diag("resident=0,fuse=0"):
        ref = api.NonlinearFactorSetGPU(ctx)
        for f in factors:
            ref.add(f)
        want = [ref.linearize(v) for v in poses]
        ref.close()
    assert want[0][0]["num_inliers"] > 100
    return want


def _serve(api, ctx, factors, poses, calls):
    """`calls` linearisations of a fresh set over the poses in turn; returns the records and how many requests the session served meanwhile"""
    before = api.resident_stats(ctx)
    fset = api.NonlinearFactorSetGPU(ctx)
    for f in factors:
        fset.add(f)
    try:
        got = [fset.linearize(poses[rep % len(poses)]) for rep in range(calls)]
    finally:
        fset.close()
    after = api.resident_stats(ctx)
    return got, {k: after[k] - before[k] for k in ("launches", "requests")}


def _compare(got, want, what):
    """got: records per call; want: records per pose (call rep used pose rep % len(want)) or per call"""
    for rep, Ls in enumerate(got):
        Bs = want[rep % len(want)]
        assert len(Ls) == len(Bs)
        for k, (L, B) in enumerate(zip(Ls, Bs)):
            _same(L, B, f"{what} call {rep} factor {k}")


def _both_forms(api, ctx, factors, poses, want, calls, what):
    """the session with piece blocks (default) and with one finaliser per factor (fin_pieces=0): each against the reference, and against each other"""
    got = {}
    for mode in ("resident=1", "resident=1,fin_pieces=0"):
        api.resident_stop(ctx)
        with ctx.diag(mode):
            got[mode], served = _serve(api, ctx, factors, poses, calls)
        # (a request that raced an idle-out is answered by a fresh session or by a launch: at least one launch, most calls through the session)
        assert served["launches"] >= 1 and served["requests"] >= calls - WARMUP - 2, (what, mode, served)
        _compare(got[mode], want, f"{what} [{mode}] against the two-dispatch form:")
    _compare(got["resident=1"], got["resident=1,fin_pieces=0"], f"{what} piece blocks against fin_pieces=0:")


@pytest.mark.parametrize("rings,azimuths", [(16, 256), (64, 512), (20, 500)])
def test_single_factor_piece_blocks_give_the_reference_bits(api, ctx, orc, scans, rings, azimuths):
    """One factor, unary and binary, 40 calls over 3 moving poses through the session."""
    tg, sg, vms, delta = scans(rings, azimuths)
    n = sg.size()
    rows = (n + BLOCK - 1) // BLOCK  # one point per thread: a single factor of at most 256 x 256 points is planned into ceil(n / 256) rows
    print(f"{rings} x {azimuths}: {n} points, {rows} partial rows")
    if (rings, azimuths) == (20, 500):
        assert n % BLOCK != 0 and rows % 32 != 0 and rows > 32, (n, rows)  # (10 000 points: 40 rows -- groups 0..7 add two rows, the others one)
    poses = _poses(orc, delta, 1)
    try:
        for target in (0, np.eye(4)):
            factors = [api.IntegratedVGICPFactorGPU(target, 1, vms[0], sg)]
            want = _reference(api, ctx, factors, poses)
            _both_forms(api, ctx, factors, poses, want, 40, f"{rings}x{azimuths} {'binary' if isinstance(target, int) else 'unary'}")
    finally:
        api.resident_stop(ctx)


def test_sets_on_both_sides_of_the_threshold(api, ctx, orc, scans):
    """Sets of 2, HOST_ROTATE_MAX_FACTORS and one more factor on 16 x 256 frames: up to the threshold the session ships raw records and runs ten piece
    blocks per factor, above it one finaliser per factor that rotates on the device.  Every one starts a session and returns the reference bits."""
    nmax = _host_rotate_max_factors()
    assert nmax == 8
    tg, sg, vms, delta = scans(16, 256)
    try:
        for copies in (2, nmax, nmax + 1):
            factors = [api.IntegratedVGICPFactorGPU(0 if k < 4 else np.eye(4), 1 + k, vms[k % 2], sg) for k in range(copies)]
            poses = _poses(orc, delta, copies)
            want = _reference(api, ctx, factors, poses)
            _both_forms(api, ctx, factors, poses, want, 12, f"{copies} factors")
    finally:
        api.resident_stop(ctx)


def test_switch_flipped_under_a_live_session(api, ctx, orc, scans):
    """fin_pieces flipped three times under a live session: the kernel keeps the form it was launched with, so every flip restarts it (`launches`
    grows) and every record is right."""
    tg, sg, vms, delta = scans(16, 256)
    factors = [api.IntegratedVGICPFactorGPU(0, 1, vms[0], sg)]
    poses = _poses(orc, delta, 1, n=8)
    want = _reference(api, ctx, factors, poses)
    fset = api.NonlinearFactorSetGPU(ctx)
    fset.add(factors[0])
    try:
        api.resident_stop(ctx)
        with ctx.diag("resident=1"):
            for rep, v in enumerate(poses):  # (the warm-up launches, then the session)
                _same(fset.linearize(v)[0], want[rep][0], f"group 0 call {rep}")
        assert api.resident_stats(ctx)["alive"]
        for group, pieces in enumerate((0, 1, 0), start=1):
            before = api.resident_stats(ctx)
            with ctx.diag(f"resident=1,fin_pieces={pieces}"):
                for rep, v in enumerate(poses):
                    _same(fset.linearize(v)[0], want[rep][0], f"group {group} (fin_pieces={pieces}) call {rep}")
            after = api.resident_stats(ctx)
            assert after["launches"] >= before["launches"] + 1, (group, pieces, before, after)
            assert after["requests"] >= before["requests"] + len(poses), (group, pieces, before, after)
    finally:
        api.resident_stop(ctx)
        fset.close()


def test_surface_validation_rows_without_inliers(api, ctx, orc, scans):
    """Surface validation on: points are rejected by the normal test, rows with few or no inliers occur and the chains add signed zeros."""
    tg, sg, vms, delta = scans(64, 512)
    poses = _poses(orc, delta, 1)
    try:
        for target in (0, np.eye(4)):
            f = api.IntegratedVGICPFactorGPU(target, 1, vms[0], sg)
            f.set_enable_surface_validation(True)
            want = _reference(api, ctx, [f], poses)
            off = api.IntegratedVGICPFactorGPU(target, 1, vms[0], sg)
            plain = _reference(api, ctx, [off], poses)
            assert want[0][0]["num_inliers"] < plain[0][0]["num_inliers"]  # (the validation does reject points here)
            _both_forms(api, ctx, [f], poses, want, 40, f"surface validation {'binary' if isinstance(target, int) else 'unary'}")
    finally:
        api.resident_stop(ctx)
