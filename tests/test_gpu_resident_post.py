"""How a resident session gets its poses (switch resident_post, vgicp.hip resident_post_direct / resident_kernel).

lines: the host leaves the poses in request lines in pinned host memory, the session's leader fetches them and re-publishes them on the device.
direct: the host stores the pose granules {lo32, tag, hi32, tag} itself, through the large BAR into fine-grained device memory; the leader only
keeps the lifecycle.  auto (default): direct for sets of at most RESIDENT_DIRECT_MAX_FACTORS factors where the device memory is host-visible.
Every way has to return the bits of the two-dispatch launch-per-call form (resident=0,fuse=0), on every field.  Shapes: 16 x 256 (16 partial rows:
more worker blocks than pose replicas, fewer than finaliser groups) and 64 x 512 (128 rows: a chip-wide factor)."""
import os
import re
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = np.array([0.002, -0.001, 0.003, 0.02, 0.01, -0.02])
WARMUP = 3  # synchronous linearisations of a plan that are launches before a session serves it (vgicp.hip RESIDENT_WARMUP)


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


def _direct_max_factors():
    src = open(os.path.join(ROOT, "glim_amd", "csrc", "vgicp.hip")).read()
    m = re.search(r"^#define GLIM_AMD_RESIDENT_DIRECT_MAX (\d+)$", src, re.M)
    assert m and "RESIDENT_DIRECT_MAX_FACTORS = GLIM_AMD_RESIDENT_DIRECT_MAX;" in src
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


def _serve(api, ctx, factors, poses, want, calls, what):
    """`calls` linearisations of a fresh set over the poses in turn, each compared with the reference; returns how the session's requests were posted"""
    before = api.resident_post_stats(ctx)
    fset = api.NonlinearFactorSetGPU(ctx)
    for f in factors:
        fset.add(f)
    try:
        for rep in range(calls):
            got = fset.linearize(poses[rep % len(poses)])
            for k, (L, B) in enumerate(zip(got, want[rep % len(poses)])):
                _same(L, B, f"{what} call {rep} factor {k}")
    finally:
        fset.close()
    after = api.resident_post_stats(ctx)
    return {k: after[k] - before[k] for k in after}


@pytest.mark.parametrize("rings,azimuths", [(16, 256), (64, 512)])
def test_single_factor_direct_and_lines_give_the_reference_bits(api, ctx, orc, scans, rings, azimuths):
    """One factor, unary and binary, 60 calls over 3 moving poses under either way of posting: the reference bits, and the requests of calls 4
    onwards went the way the mode says."""
    tg, sg, vms, delta = scans(rings, azimuths)
    poses = _poses(orc, delta, 1)
    try:
        for target in (0, np.eye(4)):
            factors = [api.IntegratedVGICPFactorGPU(target, 1, vms[0], sg)]
            want = _reference(api, ctx, factors, poses)
            for way, other in (("direct", "lines"), ("lines", "direct")):
                api.resident_stop(ctx)
                with ctx.diag(f"resident=1,resident_post={way}"):
                    posted = _serve(api, ctx, factors, poses, want, 60, f"{rings}x{azimuths} {'binary' if isinstance(target, int) else 'unary'} {way}")
                # (a request that raced an idle-out is posted twice: at least, not exactly)
                assert posted[way] >= 60 - WARMUP and posted[other] == 0, (way, posted)
    finally:
        api.resident_stop(ctx)


def test_sets_on_both_sides_of_the_threshold(api, ctx, orc, scans):
    """Sets of 2, 4, 5 and 34 factors on 16 x 256 frames through the session in its default mode: the reference bits; posted direct up to
    RESIDENT_DIRECT_MAX_FACTORS factors and through the lines above."""
    nmax = _direct_max_factors()
    assert nmax >= 1  # (it has to cover the single factor)
    tg, sg, vms, delta = scans(16, 256)
    try:
        for copies in (2, 4, 5, 34):
            factors = [api.IntegratedVGICPFactorGPU(0 if k < 4 else np.eye(4), 1 + k, vms[k % 2], sg) for k in range(copies)]
            poses = _poses(orc, delta, copies)
            want = _reference(api, ctx, factors, poses)
            api.resident_stop(ctx)
            with ctx.diag("resident=1"):
                posted = _serve(api, ctx, factors, poses, want, 12, f"{copies} factors")
            way, other = ("direct", "lines") if copies <= nmax else ("lines", "direct")
            assert posted[way] >= 12 - WARMUP and posted[other] == 0, (copies, nmax, posted)
    finally:
        api.resident_stop(ctx)


def test_switch_flipped_under_a_live_session(api, ctx, orc, scans):
    """resident_post flipped three times under a live session: the kernel keeps the way it was launched with, so every flip restarts it
    (`launches`), every record is right and every request goes the way the switch says at the time."""
    tg, sg, vms, delta = scans(16, 256)
    factors = [api.IntegratedVGICPFactorGPU(0, 1, vms[0], sg)]
    poses = _poses(orc, delta, 1, n=8)
    want = _reference(api, ctx, factors, poses)
    fset = api.NonlinearFactorSetGPU(ctx)
    fset.add(factors[0])
    try:
        api.resident_stop(ctx)
        with ctx.diag("resident=1,resident_post=direct"):
            for rep, v in enumerate(poses):  # (the warm-up launches, then the session)
                _same(fset.linearize(v)[0], want[rep][0], f"group 0 call {rep}")
        assert api.resident_stats(ctx)["alive"]
        for group, way in enumerate(("lines", "direct", "lines"), start=1):
            launches = api.resident_stats(ctx)["launches"]
            before = api.resident_post_stats(ctx)
            with ctx.diag(f"resident=1,resident_post={way}"):
                for rep, v in enumerate(poses):
                    _same(fset.linearize(v)[0], want[rep][0], f"group {group} ({way}) call {rep}")
            after = api.resident_post_stats(ctx)
            other = "direct" if way == "lines" else "lines"
            assert after[way] - before[way] >= len(poses) and after[other] == before[other], (group, way, before, after)
            assert api.resident_stats(ctx)["launches"] >= launches + 1, (group, way)
    finally:
        api.resident_stop(ctx)
        fset.close()


def test_direct_requests_that_race_the_idle_out(api, ctx, orc, scans):
    """In a direct session nobody decides atomically between "serve" and "leave": the host's granules of a request and the leader's exit granules
    can interleave.  Calls of the chip-wide factor spaced around a 100 us idle time-out (pauses of 0..400 us) hit that moment many times: every call
    returns the reference bits, the session was restarted many times, and NO call comes near the host's 200 ms give-up -- a call that reaches it
    means a block went on waiting for a request the session had left (exit did not dominate)."""
    tg, sg, vms, delta = scans(64, 512)
    factors = [api.IntegratedVGICPFactorGPU(0, 1, vms[0], sg)]
    poses = _poses(orc, delta, 1)
    want = _reference(api, ctx, factors, poses)
    rng = np.random.default_rng(11)
    api.resident_stop(ctx)
    fset = api.NonlinearFactorSetGPU(ctx)
    fset.add(factors[0])
    try:
        with ctx.diag("resident=1,resident_post=direct,resident_idle_us=100"):
            before = api.resident_stats(ctx)
            posted0 = api.resident_post_stats(ctx)
            slowest = 0.0
            t0 = time.perf_counter()
            for rep in range(1500):
                t1 = time.perf_counter()
                got = fset.linearize(poses[rep % 3])[0]
                slowest = max(slowest, time.perf_counter() - t1)
                _same(got, want[rep % 3][0], f"call {rep}")
                pause = rng.uniform(0.0, 400e-6)
                t1 = time.perf_counter()
                while time.perf_counter() - t1 < pause:
                    pass
            elapsed = time.perf_counter() - t0
            after = api.resident_stats(ctx)
            posted1 = api.resident_post_stats(ctx)
        print(f"direct idle-out race: 1500 calls in {elapsed:.2f} s, slowest call {slowest * 1e3:.2f} ms, launches +{after['launches'] - before['launches']}, "
              f"posted direct +{posted1['direct'] - posted0['direct']}, lines +{posted1['lines'] - posted0['lines']}")
        assert posted1["direct"] - posted0["direct"] >= 1500 - WARMUP and posted1["lines"] == posted0["lines"], (posted0, posted1)
        assert after["launches"] >= before["launches"] + 10, (before, after)
        assert slowest < 0.150, slowest
        assert elapsed < 60.0, elapsed
    finally:
        api.resident_stop(ctx)
        fset.close()
