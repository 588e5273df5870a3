"""ICP fine registration on the device (include/glim_amd.h "ICP fine registration", glim_amd/csrc/gicp_align.hip): every trial record is the bits
of IntegratedICPFactor.linearize at the trial's pose, the decisions are those of tests/lm_restatement.py, the result depends neither on the
number of rounds enqueued at a time nor on the batch a problem runs in."""
import numpy as np
import pytest

import icp_restatement as icpr
import lm_restatement as lmr
from align_cases import BIG, MOVES, PERT_A, PERT_B, PERT_C, SMALL, api_params, ctx, moves, pair, same_result, teacher_forced  # noqa: F401 (ctx: a fixture)
from test_gicp import POSE_TOL, rigid_edge_subset

pytestmark = pytest.mark.gpu
ICP = "icp_align_params"  # the factory of the loop's own defaults (max_iterations 200)
S = lmr

# (size, perturbation of the planted motion, max_correspondence_distance, parameters, expected (status, iterations, trials)).  Found with
# lm_restatement.run over the oracle's GICP factor with M = I (point-to-point) and over tests/icp_restatement.py (point-to-plane) on the CPU: in
# every case each trial moves the error by at least 1.2e-2 of itself, more than twice align_cases.MOVES, so no decision hinges on the record
# tolerance and status, iterations and trials are compared exactly -- no "close trial" allowance.
POINT_CASES = [
    (SMALL, PERT_A, 0.5, dict(max_iterations=2), (S.MAX_TRIALS, 1, 4)),
    (BIG, PERT_A, 0.5, dict(relative_error_tol=5e-2), (S.CONVERGED, 3, 14)),
    ((24, 256), PERT_B, 1.0, dict(lambda_initial=1e-12, max_iterations=3), (S.MAX_ITERATIONS, 3, 3)),
    ((32, 128), PERT_C, 1.0, dict(relative_error_tol=5e-2), (S.CONVERGED, 6, 6)),
    (SMALL, PERT_A, 0.5, dict(), (S.LAMBDA_BOUND, 1, 12)),
]
PLANE_CASES = [
    (SMALL, PERT_B, 1.0, dict(lambda_initial=1e-12, max_iterations=3), (S.MAX_ITERATIONS, 3, 3)),
    (SMALL, PERT_C, 1.0, dict(relative_error_tol=5e-2), (S.CONVERGED, 3, 3)),
]
CASES = [(False,) + c for c in POINT_CASES] + [(True,) + c for c in PLANE_CASES]


def icp_params(kw):
    return lmr.params(dict(lmr.DEFAULTS, max_iterations=200), **kw)


def factor_records(f):
    return lambda poses: [f.linearize({1: poses[0]})]


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_every_trial_is_the_factor_record_and_the_restatement_decision(orc, ctx, plane):
    from glim_amd import api

    ((tp, tc, tg), (sp, sc, sg)), delta = pair(orc, ctx, BIG)
    T0 = delta @ orc.se3_exp(PERT_A)
    f = api.IntegratedICPFactor(np.eye(4), 1, tg, sg, max_correspondence_distance=0.5, use_point_to_plane=plane)
    flags = api.ICP_POINT_TO_PLANE if plane else 0
    for kw in (dict(), dict(lambda_initial=1e-12, max_iterations=3)):
        results, traces = api.icp_align_debug_trace([f.target_tree], [sg], [T0], 0.5, flags, api_params(kw, ICP))
        s = teacher_forced(factor_records(f), results, traces, [T0], icp_params(kw))[0]
        print(plane, kw, "status", results[0].status_name, "iterations", results[0].iterations, "trials", results[0].trials, "inliers", results[0].num_inliers)
        assert s["iterations"] >= 1 and results[0].num_inliers > 100
        assert same_result(results[0], f.align(T0, api_params(kw, ICP)))  # the B = 1 form of the factor, without the trace
    f.close()


def same_traces(a, b):
    return len(a) == len(b) and all(np.array_equal(x["T"], y["T"]) and x["lam"] == y["lam"] and np.array_equal(x["compact"], y["compact"]) and
                                    (x["accepted"], x["status"]) == (y["accepted"], y["status"]) for x, y in zip(a, b))


def test_the_chunk_length_moves_no_bit(orc, ctx):
    """the state lives on the device between chunks: 1, 7, the default 41 and every round up front return the same results and traces.  Two
    problems, one of which (case 5 of the table: 12 trials) crosses several chunk ends while the other has already stopped"""
    from glim_amd import api

    ((tp, tc, tg), (sp, sc, sg)), delta = pair(orc, ctx, SMALL)
    owner = api.IntegratedICPFactor(np.eye(4), 1, tg, sg, max_correspondence_distance=0.5)
    for flags in (0, api.ICP_POINT_TO_PLANE):
        args = ([owner.target_tree] * 2, [sg, sg], [delta @ orc.se3_exp(PERT_A), delta @ orc.se3_exp(PERT_B)], [0.5, 1.0], flags)
        want, want_traces = api.icp_align_debug_trace(*args, rounds_per_chunk=0)
        if not flags:
            assert want[0].trials >= 12 and want[0].status == lmr.LAMBDA_BOUND
        assert want[0].trials != want[1].trials
        for chunk in (1, 7, 41, "all"):
            got, got_traces = api.icp_align_debug_trace(*args, rounds_per_chunk=chunk)
            for i in range(2):
                assert same_result(got[i], want[i]) and same_traces(got_traces[i], want_traces[i]), (flags, chunk, i)
        for i, r in enumerate(api.icp_align_batch(*args)):
            assert same_result(r, want[i])
    owner.close()


def test_a_problem_does_not_depend_on_its_batch(orc, ctx):
    """five problems of mixed sizes over one shared index: one ends in round 0 (a far pose: no correspondences), one stops early; each returns
    the bits it returns alone, in any window of the batch"""
    from glim_amd import api

    ((tp, tc, tg), (sp, sc, sg)), delta = pair(orc, ctx, BIG)
    owner = api.IntegratedICPFactor(np.eye(4), 1, tg, sg, max_correspondence_distance=1.0)
    tree = owner.target_tree
    far = delta.copy()
    far[0, 3] += 1e3
    near = delta @ orc.se3_exp([0.004, -0.003, 0.002, 0.03, 0.02, -0.01])
    subs = [api.PointCloudGPU.clone(sp[rigid_edge_subset(sp, n)], ctx=ctx) for n in (257, 3000)]
    plist = [(tree, sg, delta @ orc.se3_exp(PERT_A), 0.5), (tree, sg, far, 1.0), (tree, subs[0], near, 1.0), (tree, subs[1], delta @ orc.se3_exp(PERT_B), 0.7),
             (tg, sg, near, 1.0)]  # (the last: a target given as a cloud, an index of its own)
    for flags in (0, api.ICP_POINT_TO_PLANE):
        # (on the CPU oracle, point-to-point: CONVERGED after 14, 3, 9 and 3 trials)
        prm = api_params(dict(relative_error_tol=5e-2), ICP)
        alone = [api.icp_align_batch([t], [s], [T], d, flags, prm)[0] for t, s, T, d in plist]
        print([(r.status_name, r.iterations, r.trials, r.num_inliers) for r in alone])
        assert alone[1].status == lmr.NO_CORRESPONDENCES and alone[1].trials == 0 and np.array_equal(alone[1].T_target_source, far)
        assert len({r.trials for r in alone}) >= (2 if flags else 3)  # problems that finish in different rounds; one of them early
        ran = [r.trials for r in alone if r.status != lmr.NO_CORRESPONDENCES]
        assert 0 < min(ran) < max(ran) and (flags or min(ran) <= 4)
        for r in alone:
            assert r.status in range(1, 7) and np.all(np.isfinite(r.T_target_source)) and np.all(np.isfinite(r.compact))
        for idx in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [1, 0], [2, 1, 3]):
            got = api.icp_align_batch([plist[i][0] for i in idx], [plist[i][1] for i in idx], [plist[i][2] for i in idx], [plist[i][3] for i in idx], flags, prm)
            for i, r in zip(idx, got):
                assert same_result(r, alone[i]), (flags, idx, i, r.status_name, alone[i].status_name)
    for c in subs:
        c.close()
    owner.close()


@pytest.fixture(scope="module")
def end_to_end(orc, ctx):
    """per case, computed once: the device result, the restatement over IntegratedICPFactor.linearize (the host-driven loop), and the restatement
    over the FP64 reference -- the oracle's GICP factor with M = I for point-to-point, tests/icp_restatement.py with the device's normals for
    point-to-plane"""
    from glim_amd import api

    out = []
    for plane, size, pert, max_d, kw, expected in CASES:
        ((tp, tc, tg), (sp, sc, sg)), delta = pair(orc, ctx, size)
        T0 = delta @ orc.se3_exp(pert)
        f = api.IntegratedICPFactor(np.eye(4), 1, tg, sg, max_correspondence_distance=max_d, use_point_to_plane=plane)
        p = icp_params(kw)
        dev = f.align(T0, api_params(kw, ICP))
        host, _ = lmr.run(lambda T: f.linearize({1: T}), T0, p)
        if plane:
            normals = tg.download(covs=False, normals=True)[2].astype(np.float64)
            ref, ref_trace = lmr.run(lambda T: icpr.icp_linearize(tp, sp, T, max_d, normals=normals), T0, p)
        else:
            eye, zero = np.tile(np.eye(3), (len(tp), 1, 1)), np.zeros((len(sp), 3, 3))
            ref, ref_trace = lmr.run(lambda T: orc.gicp_linearize(tp, eye, sp, zero, T, max_d), T0, p)
        f.close()
        out.append(dict(dev=dev, host=host, ref=ref, ref_trace=ref_trace))
    return out


@pytest.mark.parametrize("case", range(len(CASES)))
def test_end_to_end_against_the_host_driven_and_the_reference_driven_loop(end_to_end, case):
    """(no gate against the planted motion: on the oracle itself point-to-point ICP stalls 1.3e-2 m and 1.1e-2 in the rotation entries away on
    these ring scans -- that is ICP, not a defect)"""
    r, expected = end_to_end[case], CASES[case][-1]
    dev, host, ref = r["dev"], r["host"], r["ref"]
    m = moves(r["ref_trace"])
    dh, dr = np.abs(dev.T_target_source - host["T"]).max(), np.abs(dev.T_target_source - ref["T"]).max()
    print(f"case {case}: device {dev.status_name} {dev.iterations}/{dev.trials}, host-driven {host['status']} {host['iterations']}/{host['trials']}, reference "
          f"{ref['status']} {ref['iterations']}/{ref['trials']}, least move {min(m):.3e}, |dT| host {dh:.3e} reference {dr:.3e}")
    assert min(m) >= 1.2e-2 > 2 * MOVES  # the margin the cases were chosen under, on the reference trace
    assert (ref["status"], ref["iterations"], ref["trials"]) == expected
    assert (host["status"], host["iterations"], host["trials"]) == expected
    assert (dev.status, dev.iterations, dev.trials) == expected
    assert dh <= POSE_TOL and dr <= POSE_TOL


def test_every_refusal_returns_its_code_and_the_next_call_works(orc, ctx):
    from glim_amd import api

    ((tp, tc, tg), (sp, sc, sg)), delta = pair(orc, ctx, SMALL)
    owner = api.IntegratedICPFactor(np.eye(4), 1, tg, sg, max_correspondence_distance=1.0)
    bare_t, bare_s = api.PointCloudGPU.clone(tp, ctx=ctx), api.PointCloudGPU.clone(sp, ctx=ctx)
    valid = lambda: api.icp_align_batch([owner.target_tree], [sg], [delta], 1.0, 0, api_params(dict(max_iterations=2), ICP))[0]
    good = valid()
    assert good.num_inliers > 100

    def refused(code, targets, sources, dist=1.0, flags=0, params=None):
        with pytest.raises(api.GlimAmdError) as e:
            api.icp_align_batch(targets, sources, [delta] * len(sources), dist, flags, params)
        assert e.value.code == code, e.value
        assert same_result(valid(), good)  # the next valid call still works

    # covariances are not required of either cloud
    r = api.icp_align_batch([bare_t], [bare_s], [delta], 1.0, 0, api_params(dict(max_iterations=2), ICP))[0]
    assert r.num_inliers == good.num_inliers and r.status in range(1, 5)
    refused(-5, [bare_t], [bare_s], flags=api.ICP_POINT_TO_PLANE)  # point-to-plane over a target without normals
    refused(-5, [owner.target_tree, bare_t], [sg, sg], flags=api.ICP_POINT_TO_PLANE)
    assert api.icp_align_batch([owner.target_tree], [bare_s], [delta], 1.0, api.ICP_POINT_TO_PLANE, api_params(dict(max_iterations=2), ICP))[0].num_inliers > 100
    refused(-1, [owner.target_tree], [sg], flags=api.FACTOR_BINARY)  # the target is fixed
    refused(-1, [owner.target_tree], [sg], flags=0x8)
    refused(-1, [owner.target_tree], [sg], dist=-1.0)
    refused(-1, [owner.target_tree], [sg], dist=float("nan"))
    refused(-6, [owner.target_tree], [sg], dist=100.0)  # a radius beyond the ring walk of an index built for 1.0
    ctx2 = api.Context(0, 1)
    other = api.PointCloudGPU.clone(sp, ctx=ctx2)
    refused(-1, [owner.target_tree], [other])  # clouds of two contexts
    empty = api.PointCloudGPU.clone(np.zeros((0, 3)), ctx=ctx)
    refused(-1, [owner.target_tree], [empty])
    refused(-1, [empty], [sg])
    refused(-1, [owner.target_tree], [sg], params=api_params(dict(lambda_factor=1.0), ICP))
    refused(-1, [owner.target_tree], [sg], params=api_params(dict(max_trials=5000), ICP))
    refused(-1, [owner.target_tree], [sg], params=api_params(dict(error_scale=0.0), ICP))
    with pytest.raises(api.GlimAmdError):
        api.icp_align_batch([api.IncrementalVoxelMap(1.0, ctx=ctx).insert(tg)], [sg], [delta], 1.0)  # an iVox target: out of scope, refused
    assert api.icp_align_batch([], [], [], 1.0) == []
    for c in (other, empty, bare_t, bare_s):
        c.close()
    ctx2.close()
    owner.close()
