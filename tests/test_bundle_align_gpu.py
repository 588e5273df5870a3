"""Sub-map bundle optimisation on the device (include/glim_amd.h "Sub-map bundle optimisation"): N poses, all-pairs binary VGICP factors, a
prior and between terms, one call and one host synchronisation.

Scenes: synth.arc_trajectory(N, 0.6, 3.0), scans of (16, 128) = 2 048 points.  Factors: all pairs i < j, target the map of i, source the cloud
of j.  One prior of precision 1e8 I sits on pose 0 at its true pose.  Poses k >= 1 start at truth Exp(+-PERT), the sign alternating with k.
The oracle's trials of this graph on the CPU (A accepted, r rejected; relative cost change per trial):
  N 3, 0.5 m, PERT_A   AA then r...  -0.908 -0.0341, then +0.00404 on every further trial
  N 3, 1.0 m, PERT_B   AAAA          -0.941 -0.0704 -6.6e-5 -4.8e-7
  N 4, 0.5 m, PERT_B   AA then r...  -0.888 -0.172, then +8.7e-5
  N 4, 1.0 m, PERT_A   AA then r...  -0.911 -0.0100, then +7.9e-4
A trial whose margin is under 5e-3 of the cost must not decide a test (25 x the record tolerance 2e-4 of tests/test_gpu_parity.py: MOVES of
tests/test_vgicp_align_gpu.py).  So the first and fourth case run with relative_error_tol = 5e-2 (CONVERGED after 2 iterations) and the second
and third with max_iterations = 2 (MAX_ITERATIONS).  The reject case is the first with max_iterations = 3: AArrrr, MAX_TRIALS, 2 iterations,
6 trials; its margin 4.0e-3 is 20 x the record tolerance, the one case under 5e-3.  The device's clouds carry the device's own FP32
covariances, so each test that rests on such a margin asserts it again on the oracle run it makes."""
from functools import partial

import numpy as np
import pytest

import align_cases
import bundle_lm_restatement as blr
import lm_restatement as lmr
from align_cases import MOVES, PERT_A, PERT_B, RECORD_TOL, ctx, same_result  # noqa: F401 (ctx: a fixture)
from test_gicp import POSE_TOL

pytestmark = pytest.mark.gpu
api_params = partial(align_cases.api_params, factory="bundle_align_params")
moves = partial(align_cases.moves, cost=True)
SIZE = (16, 128)
MAX_POSES = 32
CONV, TWO, THREE = dict(relative_error_tol=5e-2), dict(max_iterations=2), dict(max_iterations=3)
# (N, resolution, perturbation, parameters, the status and the iterations the oracle-driven loop ends with)
CASES = [
    (3, 0.5, PERT_A, CONV, lmr.CONVERGED, 2),
    (3, 1.0, PERT_B, TWO, lmr.MAX_ITERATIONS, 2),
    (4, 0.5, PERT_B, TWO, lmr.MAX_ITERATIONS, 2),
    (4, 1.0, PERT_A, CONV, lmr.CONVERGED, 2),
]
REJECT_CASE = (3, 0.5, PERT_A, THREE)
REJECT_MARGIN = 20 * RECORD_TOL  # 4.0e-3


_SCENES, _MAPS, _ORACLE_MAPS = {}, {}, {}


def scene(ctx, N, stride=1):
    """N scans along the arc, cut to every stride-th point, with the device's covariances: built once per module"""
    from glim_amd import api, synth

    key = (id(ctx), N, stride)
    if key not in _SCENES:
        world = synth.Scene.default()
        dirs = synth.lidar_directions(*SIZE)
        poses = synth.arc_trajectory(N, 0.6, 3.0)
        frames = []
        for i, T in enumerate(poses):
            p = synth.scan(world, T, dirs, frame_id=i).astype(np.float64)[::stride]
            g = api.PointCloudGPU.clone(p, ctx=ctx)
            g.find_neighbors(10, download=False)
            g.estimate_covariances(10)
            _, c, _ = g.download(covs=True, normals=False)
            frames.append((p, c.astype(np.float64), g))
        _SCENES[key] = (poses, frames)
    return _SCENES[key]


def vmap(ctx, N, stride, res, i):
    from glim_amd import api

    key = (id(ctx), N, stride, res, i)
    if key not in _MAPS:
        _MAPS[key] = api.GaussianVoxelMapGPU(res, ctx=ctx).insert(scene(ctx, N, stride)[1][i][2])
    return _MAPS[key]


def problem(orc, ctx, N, res, pert, stride=1, band=None, chain=None):
    """-> dict: the graph (restatement form), the api arguments, the initial poses, the true poses.  band: only the factors with j - i <= band;
    chain: a between chain of that precision along the true relative poses"""
    poses, frames = scene(ctx, N, stride)
    pairs = [(i, j) for i in range(N) for j in range(i + 1, N) if band is None or j - i <= band]
    priors = [(0, poses[0], 1e8 * np.eye(6))]
    betweens = [(k, k + 1, np.linalg.inv(poses[k]) @ poses[k + 1], chain * np.eye(6)) for k in range(N - 1)] if chain else []
    X0 = [poses[0]] + [poses[k] @ orc.se3_exp(np.array(pert) * (1 if k % 2 else -1)) for k in range(1, N)]
    factors = [(vmap(ctx, N, stride, res, i), frames[j][2], i, j) for i, j in pairs]
    return dict(g=blr.graph(N, pairs, priors, betweens), factors=factors, priors=priors, betweens=betweens, X0=np.stack(X0), truth=np.stack(poses), pairs=pairs,
                key=(N, stride, res))


def oracle_linearize(orc, ctx, pr):
    N, stride, res = pr["key"]
    _, frames = scene(ctx, N, stride)
    for i in {i for i, _ in pr["pairs"]}:
        if (N, stride, res, i) not in _ORACLE_MAPS:
            _ORACLE_MAPS[(N, stride, res, i)] = orc.VoxelMap(res).insert(frames[i][0], frames[i][1])
    return lambda Tfs: [orc.vgicp_linearize(_ORACLE_MAPS[(N, stride, res, i)], frames[j][0], frames[j][1], Tf) for (i, j), Tf in zip(pr["pairs"], Tfs)]


def caller_set(ctx, pr):
    """a caller's NonlinearFactorSetGPU of the same pairs in the same order"""
    from glim_amd import api

    fset = api.NonlinearFactorSetGPU(ctx)
    for vm, cloud, i, j in pr["factors"]:
        fset.add(api.IntegratedVGICPFactorGPU(i, j, vm, cloud))
    return fset


def run(pr, kw, **more):
    from glim_amd import api

    return api.bundle_align_debug_trace(pr["factors"], pr["priors"], pr["betweens"], list(pr["X0"]), 0, api_params(kw), **more)


def same_lin(a, b):
    return len(a) == len(b) and all(x["num_inliers"] == y["num_inliers"] and x["error"] == y["error"] and all(np.array_equal(x[k], y[k]) for k in ("H_ss", "b_s", "H_tt", "H_ts", "b_t"))
                                    for x, y in zip(a, b))


def pose44(v):
    return np.vstack([np.asarray(v).reshape(3, 4), [0, 0, 0, 1]])


def teacher_forced(ctx, pr, res, rows, p):
    """Every trace record is the caller's set's record at the trace's relative poses, bit for bit, blocks included; those poses are X_t^-1 X_s of
    the trace's candidates to 1e-12; the restatement, fed the device's records from the device's own previous state, takes the same decision
    and proposes the same candidates within pose_gate (cond of the 6N system)."""
    from glim_amd import api

    g = pr["g"]
    fset = caller_set(ctx, pr)
    s = blr.new_state(pr["X0"], p)
    assert len(rows) == res.trials + 1
    for k, e in enumerate(rows):
        if g["factors"]:
            records = fset.linearize_poses(e["Tf"])
            mine = [api.expand_compact(c, Tf, api.FACTOR_BINARY) for c, Tf in zip(e["compact"], e["Tf"])]
            assert same_lin(mine, records), k
            want = np.stack([np.linalg.inv(e["X"][t]) @ e["X"][u] for t, u in g["factors"]])
            got = np.stack([pose44(Tf) for Tf in e["Tf"]])
            assert np.abs(got - want).max() <= 1e-12, (k, np.abs(got - want).max())
        assert e["lam"] == s["lam"], k
        if k == 0:
            assert np.array_equal(e["X"], pr["X0"])
        else:
            gate = lmr.pose_gate(s)
            assert np.abs(e["X"] - s["cand"]).max() <= gate, (k, np.abs(e["X"] - s["cand"]).max(), gate)
        s["cand"] = e["X"]  # teacher forcing: the device's poses are the ones the records belong to
        s = blr.step(p, g, s, [lmr.record_of_compact(c) for c in e["compact"]])
        assert (e["accepted"], e["status"]) == (s["accepted"], s["status"]), k
        S = blr.assemble(g, e["X"], [lmr.record_of_compact(c) for c in e["compact"]])
        assert abs(e["cost"] - S["cost"]) <= 1e-9 * abs(S["cost"]), k  # (the sums of a few hundred FP64 terms on either side)
    fset.close()
    assert s["status"] != lmr.RUNNING and (res.status, res.iterations, res.trials) == (s["status"], s["iterations"], s["trials"])
    assert np.array_equal(res.poses, s["X"]) and res.lam == s["lam"]
    assert np.array_equal(res.compact, np.stack([lmr.compact_of_record(r) for r in s["recs"]]).reshape(res.compact.shape))
    assert res.num_inliers == s["sys"]["inliers"] and abs(res.cost - s["sys"]["cost"]) <= 1e-9 * abs(s["sys"]["cost"])
    assert res.cost == (res.factor_cost + res.prior_cost) + res.between_cost
    return s


# ---- 1. the teacher-forced trace ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(CASES) + 1))
def test_every_trial_is_the_set_record_and_the_restatement_decision(orc, ctx, case):
    N, res, pert, kw = (CASES[case][:4] if case < len(CASES) else REJECT_CASE)
    pr = problem(orc, ctx, N, res, pert)
    result, rows, _ = run(pr, kw)
    s = teacher_forced(ctx, pr, result, rows, blr.params(**kw))
    print("case", case, result.status_name, result.iterations, result.trials, "inliers", result.num_inliers, "cost", result.cost)
    assert s["iterations"] >= 1 and result.num_inliers > 100 * len(pr["pairs"])


@pytest.mark.parametrize("N", [5, 11])  # 30 and 66 dimensions: below and across a wavefront's width
def test_the_trace_at_larger_sizes(orc, ctx, N):
    pr = problem(orc, ctx, N, 0.5, PERT_A, stride=4, band=2, chain=1e3)
    result, rows, _ = run(pr, TWO)
    s = teacher_forced(ctx, pr, result, rows, blr.params(**TWO))
    print("N", N, result.status_name, result.iterations, result.trials, "inliers", result.num_inliers, "cost", result.cost)
    assert s["iterations"] >= 1 and result.num_inliers > 10 * len(pr["pairs"])


# ---- 2. against the oracle ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_runs(orc, ctx):
    out = {}
    for case, (N, res, pert, kw, _, _) in enumerate(CASES):
        pr = problem(orc, ctx, N, res, pert)
        out[case] = (pr,) + blr.run(oracle_linearize(orc, ctx, pr), pr["g"], pr["X0"], blr.params(**kw))
    pr = problem(orc, ctx, *REJECT_CASE[:3])
    out["reject"] = (pr,) + blr.run(oracle_linearize(orc, ctx, pr), pr["g"], pr["X0"], blr.params(**REJECT_CASE[3]))
    out["linearize"] = lambda pr: oracle_linearize(orc, ctx, pr)
    return out


@pytest.mark.parametrize("case", range(len(CASES)))
def test_end_to_end_against_the_oracle_driven_loop(oracle_runs, case):
    """The decision sequence is equal; the final poses are within iterations x POSE_TOL (1e-4 m / rad per Gauss-Newton iteration, the project's
    gate); the cost within the record tolerance."""
    from glim_amd import api

    N, res, pert, kw, status, iterations = CASES[case]
    pr, ref, trace = oracle_runs[case]
    print("oracle:", "".join("A" if e["accepted"] else "r" for e in trace), ["%.2e" % m for m in moves(trace)], ref["status"], ref["iterations"], ref["trials"])
    assert min(moves(trace)) > MOVES, moves(trace)  # the condition the case was chosen for, on this run's oracle
    assert (ref["status"], ref["iterations"]) == (status, iterations)
    dev, rows, _ = run(pr, kw)
    assert [e["accepted"] for e in rows] == [e["accepted"] for e in trace]
    assert (dev.status, dev.iterations, dev.trials) == (ref["status"], ref["iterations"], ref["trials"])
    d = np.abs(dev.poses - ref["X"]).max()
    at_dev = blr.assemble(pr["g"], dev.poses, oracle_runs["linearize"](pr)(blr.relative_poses(pr["g"], dev.poses)))  # the oracle AT the device's poses
    print(f"case {case}: |dX| {d:.3e}, cost {dev.cost}, the oracle's there {at_dev['cost']}, at its own poses {ref['sys']['cost']}")
    assert d <= ref["iterations"] * POSE_TOL
    assert abs(dev.cost - at_dev["cost"]) <= RECORD_TOL * at_dev["cost"] and dev.num_inliers > 0  # the record tolerance, at equal poses
    assert np.abs(dev.poses - pr["truth"]).max() < np.abs(pr["X0"] - pr["truth"]).max() / 5  # it moved towards the truth
    plain = api.bundle_align(pr["factors"], pr["priors"], pr["betweens"], list(pr["X0"]), 0, api_params(kw))
    assert same_result(plain, dev)  # the stable entry is the traced one


def test_a_rejected_trial_on_the_device(orc, ctx, oracle_runs):
    pr, ref, trace = oracle_runs["reject"]
    accepted = [e["accepted"] for e in trace]
    print("oracle:", "".join("A" if a else "r" for a in accepted), ["%.2e" % m for m in moves(trace)], ref["status"], ref["iterations"], ref["trials"])
    assert accepted == [True, True, True, False, False, False, False] and (ref["status"], ref["iterations"], ref["trials"]) == (lmr.MAX_TRIALS, 2, 6)
    assert min(moves(trace)) >= 0.9 * REJECT_MARGIN > 10 * RECORD_TOL, moves(trace)  # the margin 4.0e-3 of the docstring, on this run's oracle
    dev, rows, _ = run(pr, REJECT_CASE[3])
    assert [e["accepted"] for e in rows] == accepted
    assert (dev.status, dev.iterations, dev.trials) == (lmr.MAX_TRIALS, 2, 6)
    k = accepted.index(False)
    assert rows[k + 1]["lam"] == rows[k]["lam"] * 10  # the next candidates are solved from the kept system with the new lambda
    assert np.abs(dev.poses - ref["X"]).max() <= ref["iterations"] * POSE_TOL


# ---- 3. parallel equals serial -----------------------------------------------------------------------------------------------------------------
def test_the_workgroup_form_equals_the_one_thread_form(orc, ctx):
    pr = problem(orc, ctx, *REJECT_CASE[:3])
    a, rows_a, _ = run(pr, REJECT_CASE[3])
    b, rows_b, _ = run(pr, REJECT_CASE[3], one_thread=True)
    assert same_result(a, b) and a.trials == 6
    for x, y in zip(rows_a, rows_b):
        assert np.array_equal(x["X"], y["X"]) and np.array_equal(x["Tf"], y["Tf"]) and np.array_equal(x["compact"], y["compact"])
        assert (x["lam"], x["cost"], x["accepted"], x["status"]) == (y["lam"], y["cost"], y["accepted"], y["status"])


def test_the_two_forms_at_the_cap(orc, ctx):
    pr = problem(orc, ctx, MAX_POSES, 0.5, PERT_A, stride=8, band=2, chain=1e3)
    kw = dict(max_iterations=2)
    a, _, _ = run(pr, kw, trace=False)
    b, _, _ = run(pr, kw, one_thread=True, trace=False)
    print("N", MAX_POSES, a.status_name, a.iterations, a.trials, "inliers", a.num_inliers, "cost", a.cost)
    assert same_result(a, b) and a.iterations >= 1  # (clouds of 256 points: the bits are the point here, not the registration)


# ---- 4. determinism and hygiene ----------------------------------------------------------------------------------------------------------------
def test_determinism_in_one_context_and_in_another(orc, ctx):
    from glim_amd import api

    pr = problem(orc, ctx, 3, 0.5, PERT_A)
    a, _, _ = run(pr, CONV)
    b, _, _ = run(pr, CONV)
    assert same_result(a, b) and a.iterations == 2
    ctx2 = api.Context(0, 1)
    pr2 = problem(orc, ctx2, 3, 0.5, PERT_A)
    c, _, _ = run(pr2, CONV)
    assert same_result(a, c)
    for key in [k for k in _MAPS if k[0] == id(ctx2)]:
        _MAPS.pop(key).close()
    for _, _, g in _SCENES.pop((id(ctx2), 3, 1))[1]:
        g.close()
    ctx2.close()


def test_a_callers_set_and_its_plan_are_left_alone(orc, ctx):
    from glim_amd import api

    pr = problem(orc, ctx, 3, 0.5, PERT_A)
    fset = caller_set(ctx, pr)
    Tf = np.stack([api.pose12(np.linalg.inv(pr["X0"][i]) @ pr["X0"][j]) for i, j in pr["pairs"]])
    before = fset.linearize_poses(Tf)
    plans = api.plan_stats(ctx)
    r, _, _ = run(pr, CONV)
    assert r.iterations == 2
    assert api.plan_stats(ctx) == plans  # no plan of the context built, recycled, parked or taken
    assert same_lin(fset.linearize_poses(Tf), before) and before[0]["num_inliers"] > 100
    values = {k: r.poses[k] for k in range(3)}
    got, res = fset.optimize({k: pr["X0"][k] for k in range(3)}, pr["priors"], pr["betweens"], api_params(CONV))
    assert same_result(res, r) and all(np.array_equal(got[k], values[k]) for k in values)  # the set's own entry is the same call
    fset.close()


def test_a_resident_session_of_the_context_is_left_alone(orc):
    from glim_amd import api

    ctx1 = api.Context(0, 1, priority=1)
    try:
        pr = problem(orc, ctx1, 3, 0.5, PERT_A)
        vm, cloud, i, j = pr["factors"][0]
        fset = api.NonlinearFactorSetGPU(ctx1)
        fset.add(api.IntegratedVGICPFactorGPU(np.eye(4), 1, vm, cloud))
        T = {1: np.linalg.inv(pr["X0"][i]) @ pr["X0"][j]}
        with ctx1.diag("resident=1,resident_idle_us=200000"):
            before = [fset.linearize(T) for _ in range(6)]
            stats = api.resident_stats(ctx1)
            assert stats["alive"] and same_lin(before[0], before[-1])
            r, _, _ = run(pr, CONV)
            assert r.iterations >= 1
            assert api.resident_stats(ctx1)["alive"]
            after = fset.linearize(T)
            now = api.resident_stats(ctx1)
            assert same_lin(after, before[0])
            assert now["launches"] == stats["launches"] and now["requests"] == stats["requests"] + 1, (stats, now)  # the same session answered
        fset.close()
    finally:
        api.resident_stop(ctx1)


def test_later_rounds_of_a_finished_problem_change_nothing(orc, ctx):
    pr = problem(orc, ctx, 3, 0.5, PERT_A)
    a, rows_a, _ = run(pr, CONV)
    b, rows_b, raw = run(pr, dict(CONV, max_trials=12))
    assert same_result(a, b) and a.trials == 2 and len(rows_a) == len(rows_b) == 3
    tX, tTf, trec, tr = raw
    assert not tX[3:].any() and not tTf[3:].any() and not trec[3:].any()  # the rounds after the last are never written
    assert all((tr[k].lam, tr[k].cost, tr[k].accepted, tr[k].status) == (0.0, 0.0, 0, 0) for k in range(3, 13))


# ---- 5. edge cases -----------------------------------------------------------------------------------------------------------------------------
def test_terms_alone_converge_to_their_minimum(orc, ctx):
    from glim_amd import api

    poses, _ = scene(ctx, 3)
    priors = [(0, poses[0], 1e4 * np.eye(6))]
    betweens = [(k, k + 1, np.linalg.inv(poses[k]) @ poses[k + 1], 1e2 * np.eye(6) + 10.0 * np.ones((6, 6))) for k in range(2)]
    X0 = [poses[0] @ orc.se3_exp(np.array(PERT_A))] + [poses[k] @ orc.se3_exp(np.array(PERT_B) * (1 if k % 2 else -1)) for k in (1, 2)]
    r = api.bundle_align([], priors, betweens, X0, ctx=ctx)
    ref, _ = blr.run(lambda Tf: [], blr.graph(3, [], priors, betweens), np.stack(X0), blr.params())
    print("terms alone:", r.status_name, r.iterations, r.trials, r.cost)
    # the last accepted step moved the cost by <= 1e-5 under quadratic convergence: what is left is far below 1e-8, and with informations
    # >= 100 the poses are within sqrt(1e-8 / 100) = 1e-5
    assert r.status == lmr.CONVERGED == ref["status"] and (r.iterations, r.trials) == (ref["iterations"], ref["trials"])
    assert r.cost < 1e-8 and r.factor_cost == 0.0 and r.num_inliers == 0 and np.abs(r.poses - np.stack(poses)).max() < 1e-5


def test_an_untouched_pose_keeps_its_bits(orc, ctx):
    from glim_amd import api

    pr = problem(orc, ctx, 3, 0.5, PERT_A)
    lone = pr["truth"][1] @ orc.se3_exp([0.3, -0.2, 0.1, 5.0, -4.0, 3.0])
    X0 = list(pr["X0"]) + [lone]
    r = api.bundle_align(pr["factors"], pr["priors"], pr["betweens"], X0, 0, api_params(CONV))
    want, _, _ = run(pr, CONV)
    assert r.iterations == 2 and np.array_equal(r.poses[3], lone)
    assert (r.status, r.iterations, r.trials, r.num_inliers) == (want.status, want.iterations, want.trials, want.num_inliers)
    assert np.abs(r.poses[:3] - want.poses).max() <= 2 * POSE_TOL


def test_no_overlap_anywhere(orc, ctx):
    from glim_amd import api

    pr = problem(orc, ctx, 3, 0.5, PERT_A)
    X0 = [pr["X0"][0]] + [x.copy() for x in pr["X0"][1:]]
    for k in (1, 2):
        X0[k][0, 3] += 1e3 * k
    r = api.bundle_align(pr["factors"], pr["priors"], pr["betweens"], X0, 0, api_params(CONV))
    assert r.status == lmr.NO_CORRESPONDENCES and (r.iterations, r.trials, r.num_inliers) == (0, 0, 0) and np.array_equal(r.poses, np.stack(X0))


def test_the_caps_and_the_argument_errors_with_real_handles(orc, ctx):
    from glim_amd import api

    pr = problem(orc, ctx, 3, 0.5, PERT_A)
    good, _, _ = run(pr, CONV)

    def refused(code, factors=pr["factors"], priors=pr["priors"], betweens=pr["betweens"], X0=list(pr["X0"]), flags=0, c=None):
        with pytest.raises(api.GlimAmdError) as e:
            api.bundle_align(factors, priors, betweens, X0, flags, api_params(CONV), ctx=c)
        assert e.value.code == code, e.value
        assert same_result(run(pr, CONV)[0], good)  # the next valid call still works

    refused(-6, X0=list(pr["X0"]) + [np.eye(4)] * (MAX_POSES + 1 - 3))  # N = MAX + 1
    vm, cloud, i, j = pr["factors"][0]
    refused(-1, factors=[(vm, cloud, 1, 1)])  # t == s
    refused(-1, factors=[(vm, cloud, 0, 3)])  # an index out of range
    refused(-1, flags=api.FACTOR_BINARY)
    ctx2 = api.Context(0, 1)
    refused(-1, c=ctx2)  # handles of another context than the call's
    p, cov, _ = scene(ctx, 3)[1][1]
    refused(-5, factors=[(vm, api.PointCloudGPU.clone(p, ctx=ctx), 0, 1)])  # a source without covariances (glim_amd_factor_set_add's answer)
    refused(-5, factors=[(api.GaussianVoxelMapGPU(0.5, ctx=ctx), cloud, 0, 1)])  # a map nothing was inserted into (likewise)
    refused(-1, factors=[(vm, api.PointCloudGPU.clone(np.zeros((0, 3)), covs=np.zeros((0, 3, 3)), ctx=ctx), 0, 1)])  # an empty source
    ctx2.close()
