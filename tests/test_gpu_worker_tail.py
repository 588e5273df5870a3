"""The worker tail of a resident session (vgicp.hip publish_row_tagged, one value per lane, and the flat two-point schedule of compute_row).

A row is published one value per lane (lane 4p + v of wavefront 0 forms value 3p + v, two quad_perm moves collect a granule in lane 4p), and a
resident worker loads the stream data of both points of a lane before the pose arrives and runs a row of exactly two points per lane through a flat
schedule (both key gathers, both record gathers, then the two algebras in order).  Neither changes an addition: every field of every record has to be
equal, bit for bit, between the session at its default switches, the single-dispatch form (resident=0, which publishes its rows through the same
function) and the two-dispatch form (resident=0,fuse=0, which does not).

Shapes: 4 x 256 (4 rows: fewer workers than record pieces), 16 x 256 (16 rows: fewer than the finalisers' 32 groups), 20 x 500 (40 rows, a point
count that is no multiple of 256), 66 x 1024 and 100 x 1024 (more than 256 hands of 256 points: two points per lane, the flat schedule) and
67 x 1000 (two points per lane and a last hand that is not full: lanes without a second point).  A single factor of n points is planned into
ceil(n / 256) one-point rows up to one row per compute unit and into ceil(n / 512) two-point rows above; what the plan of the 1024-wide shapes is
is read back from the library (the worker blocks of the stamped session, glim_amd_factor_set_trip_stats), not assumed."""
import time

import numpy as np
import pytest

from test_gpu_fin_pieces import BLOCK, WARMUP, _compare, _poses, _reference, _serve
from test_gpu_fin_pieces import api, ctx, scans  # noqa: F401 -- module-scoped fixtures: one context, every scan made once

pytestmark = pytest.mark.gpu

FORMS = ("resident=1", "resident=0", "resident=0,fuse=0")  # the session, one dispatch per call, two dispatches per call (the reference)


def _factor(api, target, vmap, cloud, validate):
    f = api.IntegratedVGICPFactorGPU(target, 1, vmap, cloud)
    if validate:
        f.set_enable_surface_validation(True)
    return f


def _forms_agree(api, ctx, factors, poses, calls, what):
    """the three forms on the same factors and poses; returns the reference records.  The session has to have served the calls behind the warm-up."""
    want = _reference(api, ctx, factors, poses)
    for mode in FORMS[:2]:
        api.resident_stop(ctx)
        with ctx.diag(mode):
            got, served = _serve(api, ctx, factors, poses, calls)
        if mode == "resident=1":
            # (a request that raced an idle-out is answered by a fresh session or by a launch: at least one launch, most calls through the session)
            assert served["launches"] >= 1 and served["requests"] >= calls - WARMUP - 2, (what, served)
        else:
            assert served["requests"] == 0, (what, mode, served)
        _compare(got, want, f"{what} [{mode}] against the two-dispatch form:")
    return want


def _plan_of_the_session(api, ctx, factor, pose):
    """(worker blocks = plan rows, points per lane) of the session that serves this single factor, from the library's own account"""
    fset = api.NonlinearFactorSetGPU(ctx)
    fset.add(factor)
    try:
        with ctx.diag("resident=1"):
            api.resident_timeline(0, enable=True, read=False)  # (ends a running session; the next one is stamped)
            for _ in range(WARMUP + 3):
                fset.linearize(pose)
            t = api.resident_timeline(0, enable=False, read=True, per_block=True)
            _, trips = fset.trip_stats()  # blocks x 4 wavefronts x points per lane
    finally:
        fset.close()
    assert t is not None and "blocks" in t
    rows = int(t["blocks"]["worker"].sum())
    assert rows > 0 and trips % (4 * rows) == 0, (rows, trips)
    return rows, trips // (4 * rows), t


@pytest.mark.parametrize("rings,azimuths", [(4, 256), (16, 256), (20, 500), (66, 1024), (100, 1024), (67, 1000)])
def test_single_factor_forms_give_the_same_bits(api, ctx, orc, scans, rings, azimuths):
    """One factor -- unary and binary, surface validation off and on -- through the session, in one dispatch and in two: 12 calls over 3 poses each."""
    tg, sg, vms, delta = scans(rings, azimuths)
    n = sg.size()
    print(f"{rings} x {azimuths}: {n} points")
    poses = _poses(orc, delta, 1)
    try:
        if azimuths >= 1000:
            rows, ppt, t = _plan_of_the_session(api, ctx, _factor(api, 0, vms[0], sg, False), poses[0])
            print(f"  plan: {rows} rows, {ppt} points per lane; stamped blocks {len(t['blocks']['worker'])}")
            # more hands than one row per compute unit can take: two points per lane, i.e. the flat schedule, in ceil(n / 512) rows
            assert ppt == 2 and rows == (n + 2 * BLOCK - 1) // (2 * BLOCK), (n, rows, ppt)
            assert np.all(t["blocks"]["row_published"][:rows] > 0.0)  # every worker accounted for its row
            assert len(np.unique(t["blocks"]["cu"][:rows])) > 1  # the blocks say where they run
            if (rings, azimuths) == (67, 1000):
                assert n % (2 * BLOCK) != 0 and n > (rows - 1) * 2 * BLOCK + BLOCK, n  # the last block's second hand exists and is not full
        for target in (0, np.eye(4)):
            for validate in (False, True):
                what = f"{rings}x{azimuths} {'binary' if isinstance(target, int) else 'unary'}{' validated' if validate else ''}"
                _forms_agree(api, ctx, [_factor(api, target, vms[0], sg, validate)], poses, 12, what)
    finally:
        api.resident_stop(ctx)


@pytest.mark.parametrize("rings,copies", [(16, 2), (16, 8), (4, 8), (16, 9)])
def test_sets_give_the_same_bits(api, ctx, orc, scans, rings, copies):
    """Sets of 2 and 8 factors of 16 x 256 (128 worker blocks beside 80 piece blocks), 8 factors of 4 x 256 (32 worker blocks) and 9 factors (one
    finalising block per factor, records rotated on the device): every form returns the same bits."""
    tg, sg, vms, delta = scans(rings, 256)
    factors = [api.IntegratedVGICPFactorGPU(0 if k < 4 else np.eye(4), 1 + k, vms[k % 2], sg) for k in range(copies)]
    poses = _poses(orc, delta, copies)
    try:
        _forms_agree(api, ctx, factors, poses, 12, f"{copies} factors of {rings}x256")
    finally:
        api.resident_stop(ctx)


def test_calls_around_the_idle_out(api, ctx, orc, scans):
    """300 calls of the 16-row factor with a 100 us idle time-out and about 100 us of host work between calls: sessions leave and start again and
    again, every record is the reference's, and no call comes near the host's 200 ms give-up."""
    tg, sg, vms, delta = scans(16, 256)
    factors = [api.IntegratedVGICPFactorGPU(0, 1, vms[0], sg)]
    poses = _poses(orc, delta, 1)
    want = _reference(api, ctx, factors, poses)
    api.resident_stop(ctx)
    fset = api.NonlinearFactorSetGPU(ctx)
    fset.add(factors[0])
    try:
        with ctx.diag("resident=1,resident_idle_us=100"):
            before = api.resident_stats(ctx)
            slowest = 0.0
            got = []
            for rep in range(300):
                t1 = time.perf_counter()
                got.append(fset.linearize(poses[rep % 3]))
                slowest = max(slowest, time.perf_counter() - t1)
                t1 = time.perf_counter()
                while time.perf_counter() - t1 < 100e-6:  # (the optimiser's own work between two linearisations)
                    pass
            after = api.resident_stats(ctx)
        print(f"idle-out: slowest call {slowest * 1e3:.2f} ms, launches +{after['launches'] - before['launches']}, requests +{after['requests'] - before['requests']}")
        _compare(got, want, "around the idle-out:")
        assert after["launches"] >= before["launches"] + 2, (before, after)
        assert slowest < 0.2, slowest
    finally:
        api.resident_stop(ctx)
        fset.close()
