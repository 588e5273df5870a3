"""Global-graph optimisation on the device (include/glim_amd.h "Global-graph optimisation"): the bundle's rule beyond the bundle's cap, the
systems in device memory, a round as a sequence of launches.

Scenes, maps and problems are those of tests/test_bundle_align_gpu.py at its cap case: synth.arc_trajectory(N, 0.6, 3.0), scans of (16, 128) cut
with stride 8 to 256 points, the factors (i, j) with 0 < j - i <= 2, a between chain of precision 1e3 along the true relative poses, one prior
of precision 1e8 on pose 0.  Clouds of 256 points: the bits and the decisions are the point here, not the registration.

The oracle's trials of the N = 45 graph on the CPU with the oracle's own covariances (A accepted, r rejected; relative cost change per trial),
default parameters:
  PERT_A   AAAAAA then r...  -0.733 -0.183 -0.141 -0.0712 -0.166 -0.0053*, then +0.0053 on the rejected trials
  PERT_B   AAAAAA then r...  -0.348 -0.383 -0.261 -0.0737 -0.138 -0.054*, then +0.054          (*: the first rejected trial's margin)
A trial whose margin is under 5e-3 of the cost must not decide a test (MOVES of tests/align_cases.py), and PERT_A's first rejected trial is at
that edge.  So the convergence cases stop well before it: PERT_A runs with max_iterations = 2 and PERT_B with max_iterations = 3 (MAX_ITERATIONS
both; every deciding margin is above 0.18), and each asserts its margins again on the oracle run it makes, since the device's clouds carry the
device's own FP32 covariances."""
import numpy as np
import pytest

import bundle_lm_restatement as blr
import lm_restatement as lmr
from align_cases import MOVES, PERT_A, PERT_B, build_driver, ctx, same_result  # noqa: F401 (ctx: a fixture)
from test_bundle_align_gpu import api_params, moves, oracle_linearize, problem, teacher_forced
from test_gicp import POSE_TOL
from test_graph_align import blocked_solve, spd_system

pytestmark = pytest.mark.gpu
BUNDLE_MAX_POSES = 32
SHORT = dict(max_iterations=2, max_trials=3)  # at most four rounds: the one-thread form takes a good part of a second per round at 270 rows


def graph_problem(orc, ctx, N, pert=PERT_A, lone=()):
    """the cap case's problem at N poses; lone: poses that lose every factor and term"""
    pr = dict(problem(orc, ctx, N, 0.5, pert, stride=8, band=2, chain=1e3))
    if lone:
        keep = [k for k, (i, j) in enumerate(pr["pairs"]) if i not in lone and j not in lone]
        pr["pairs"] = [pr["pairs"][k] for k in keep]
        pr["factors"] = [pr["factors"][k] for k in keep]
        pr["betweens"] = [b for b in pr["betweens"] if b[0] not in lone and b[1] not in lone]
        pr["g"] = blr.graph(N, pr["pairs"], pr["priors"], pr["betweens"])
    return pr


def run(pr, kw, **more):
    from glim_amd import api

    return api.graph_align_debug_trace(pr["factors"], pr["priors"], pr["betweens"], list(pr["X0"]), 0, api_params(kw), **more)


def same_rows(rows_a, rows_b):
    return len(rows_a) == len(rows_b) and all(
        np.array_equal(x["X"], y["X"]) and np.array_equal(x["Tf"], y["Tf"]) and np.array_equal(x["compact"], y["compact"]) and
        (x["lam"], x["cost"], x["accepted"], x["status"]) == (y["lam"], y["cost"], y["accepted"], y["status"]) for x, y in zip(rows_a, rows_b))


# ---- 1. beside the bundle ----------------------------------------------------------------------------------------------------------------------
def test_at_the_bundles_cap_the_graph_returns_the_bundles_bits(orc, ctx):
    """the blocked solver over device memory beside the one-workgroup solver in LDS: poses, records, the cost and its parts, lambda, the counts,
    the status and the inliers"""
    from glim_amd import api

    pr = graph_problem(orc, ctx, BUNDLE_MAX_POSES)
    kw = dict(max_iterations=2)
    args = (pr["factors"], pr["priors"], pr["betweens"], list(pr["X0"]), 0, api_params(kw))
    a = api.bundle_align(*args)
    b = api.graph_align(*args)
    print("N", BUNDLE_MAX_POSES, b.status_name, b.iterations, b.trials, "inliers", b.num_inliers, "cost", b.cost)
    assert same_result(a, b) and b.iterations >= 1 and b.num_inliers > 0
    _, rows_a, _ = api.bundle_align_debug_trace(*args)
    _, rows_b, _ = run(pr, kw)
    assert same_rows(rows_a, rows_b)  # and every round on the way
    fset = api.NonlinearFactorSetGPU(ctx)
    for vm, cloud, i, j in pr["factors"]:
        fset.add(api.IntegratedVGICPFactorGPU(i, j, vm, cloud))
    values = {k: x for k, x in enumerate(pr["X0"])}
    got, res = fset.optimize_graph(values, pr["priors"], pr["betweens"], api_params(kw))
    assert same_result(res, b) and all(np.array_equal(got[k], b.poses[k]) for k in values)  # the set's own entry is the same call
    fset.close()


# ---- 2. beyond the cap: the launches against one thread, a caller's set and the host's step --------------------------------------------------
@pytest.mark.parametrize("N", [33, 45])  # 198 rows: the first size over the cap; 270: five tiles, the last one ragged
def test_beyond_the_cap_every_round_is_the_one_thread_round_and_the_hosts_decision(orc, ctx, N):
    pr = graph_problem(orc, ctx, N)
    a, rows_a, _ = run(pr, SHORT)
    b, rows_b, _ = run(pr, SHORT, one_thread=True)
    print("N", N, a.status_name, a.iterations, a.trials, "inliers", a.num_inliers, "cost", a.cost)
    assert same_result(a, b) and same_rows(rows_a, rows_b) and a.iterations >= 1
    # every trace record is the caller's set's at the traced T_f; the host's step, fed the device's records, decides the same and proposes the
    # same candidates within pose_gate
    s = teacher_forced(ctx, pr, a, rows_a, blr.params(**SHORT))
    assert s["iterations"] >= 1 and a.num_inliers > 10 * len(pr["pairs"])
    from glim_amd import api

    with pytest.raises(api.GlimAmdError) as e:  # the bundle keeps its refusal
        api.bundle_align(pr["factors"], pr["priors"], pr["betweens"], list(pr["X0"]), 0, api_params(SHORT))
    assert e.value.code == -6


# ---- 3. the solve alone ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solve_exe(tmp_path_factory):
    return build_driver(tmp_path_factory, "graph_solve", "-Wno-unknown-pragmas")


@pytest.mark.parametrize("n", [198, 270, 1536])
def test_the_devices_solve_is_the_host_drivers_bit_for_bit(ctx, solve_exe, tmp_path, n):
    from glim_amd import api

    rng = np.random.default_rng(n)
    S = spd_system(rng, n)
    ref_ok, ok, same_L, same_y, same_delta, want = blocked_solve(solve_exe, tmp_path, S, n, 1e-5, 64)
    assert ref_ok and ok and same_L and same_y and same_delta  # the host driver is the serial rule
    got_ok, got = api.graph_solve_debug(blr.packed(S), n, 1e-5, ctx=ctx)
    assert got_ok and got.tobytes() == want.tobytes(), (n, np.abs(got - want).max())
    k = 64 + 32  # a pivot of an interior tile
    S["H"][k, :] = S["H"][:, k] = 0.0
    ref_ok, ok, _, _, same_delta, want = blocked_solve(solve_exe, tmp_path, S, n, 0.0, 64)
    assert not ref_ok and not ok and same_delta and not want.any()
    got_ok, got = api.graph_solve_debug(blr.packed(S), n, 0.0, ctx=ctx)
    assert not got_ok and got.tobytes() == want.tobytes()
    got_ok, got = api.graph_solve_debug(blr.packed(S), n, 1e-5, ctx=ctx)  # the next valid call still works
    assert got_ok and np.isfinite(got).all() and got[k] != 0.0


# ---- 4. the chunk length -----------------------------------------------------------------------------------------------------------------------
def test_the_chunk_length_moves_no_bit(orc, ctx):
    pr = graph_problem(orc, ctx, 33)
    kw = dict(max_iterations=3)
    a, rows_a, raw_a = run(pr, kw)
    b, rows_b, raw_b = run(pr, kw, rounds_per_chunk=1)
    c, rows_c, _ = run(pr, kw, rounds_per_chunk=64)  # longer than the loop: all rounds up front
    assert same_result(a, b) and same_rows(rows_a, rows_b) and same_result(a, c) and same_rows(rows_a, rows_c) and a.trials >= 2
    for x, y in zip(raw_a[:3], raw_b[:3]):
        assert np.array_equal(x, y)  # the rounds after the last are never written, whatever was enqueued


# ---- 5. untouched poses and a failed solve -----------------------------------------------------------------------------------------------------
def test_untouched_poses_keep_their_bits_and_a_failed_solve_is_a_rejected_trial(orc, ctx):
    lone = (20, 32)
    pr = graph_problem(orc, ctx, 33, lone=lone)
    assert all(k not in f for f in pr["pairs"] for k in lone) and all(b[0] not in lone and b[1] not in lone for b in pr["betweens"])
    a, rows, _ = run(pr, SHORT)
    teacher_forced(ctx, pr, a, rows, blr.params(**SHORT))
    assert a.iterations >= 1
    for k in lone:  # a block lambda I and a right-hand side +0.0: a zero step, the pose's bits unchanged in every candidate
        assert np.array_equal(a.poses[k], pr["X0"][k]) and all(np.array_equal(e["X"][k], pr["X0"][k]) for e in rows)
    # lambda_initial = 0: pose 20's first row (row 120, inside the second tile) has a zero pivot.  Every trial is then the kept poses again,
    # evaluated and rejected; lambda times its factor stays 0, so the loop runs into its trial budget -- as the host's step does
    kw = dict(lambda_initial=0.0, max_iterations=2, max_trials=3)
    b, rows_b, _ = run(pr, kw)
    s = teacher_forced(ctx, pr, b, rows_b, blr.params(**kw))
    assert [e["accepted"] for e in rows_b] == [True, False, False, False] and (b.status, b.iterations, b.trials) == (lmr.MAX_TRIALS, 0, 3) == (s["status"], s["iterations"], s["trials"])
    assert all(np.array_equal(e["X"], pr["X0"]) for e in rows_b) and np.array_equal(b.poses, pr["X0"]) and b.lam == 0.0
    c, rows_c, _ = run(pr, kw, one_thread=True)
    assert same_result(b, c) and same_rows(rows_b, rows_c)


# ---- 6. convergence against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pert,kw", [(PERT_A, dict(max_iterations=2)), (PERT_B, dict(max_iterations=3))])
def test_convergence_against_the_oracle_driven_loop(orc, ctx, pert, kw):
    """The decision sequence is equal; the final poses are within POSE_TOL (measured on an MI355X: 9.2e-6 and 2.3e-5)."""
    pr = graph_problem(orc, ctx, 45, pert)
    ref, trace = blr.run(oracle_linearize(orc, ctx, pr), pr["g"], pr["X0"], blr.params(**kw))
    print("oracle:", "".join("A" if e["accepted"] else "r" for e in trace), ["%.2e" % m for m in moves(trace)], ref["status"], ref["iterations"], ref["trials"])
    assert min(moves(trace)) > MOVES, moves(trace)  # the condition the case was chosen for, on this run's oracle
    assert (ref["status"], ref["iterations"]) == (lmr.MAX_ITERATIONS, kw["max_iterations"])
    dev, rows, _ = run(pr, kw)
    assert [e["accepted"] for e in rows] == [e["accepted"] for e in trace]
    assert (dev.status, dev.iterations, dev.trials) == (ref["status"], ref["iterations"], ref["trials"])
    d = np.abs(dev.poses - ref["X"]).max()
    print(f"|dX| {d:.3e}, cost {dev.cost}, the oracle's at its own poses {ref['sys']['cost']}")
    assert d <= POSE_TOL


# ---- 7. terms only -----------------------------------------------------------------------------------------------------------------------------
def test_terms_alone_at_64_poses_end_as_the_host_does(orc, ctx):
    from glim_amd import api, synth

    N = 64
    poses = synth.arc_trajectory(N, 0.6, 3.0)
    priors = [(0, poses[0], 1e4 * np.eye(6))]
    betweens = [(k, k + 1, np.linalg.inv(poses[k]) @ poses[k + 1], 1e2 * np.eye(6) + 10.0 * np.ones((6, 6))) for k in range(N - 1)]
    X0 = [poses[0] @ orc.se3_exp(np.array(PERT_A))] + [poses[k] @ orc.se3_exp(np.array(PERT_B) * (1 if k % 2 else -1)) for k in range(1, N)]
    r = api.graph_align([], priors, betweens, X0, ctx=ctx)
    ref, _ = blr.run(lambda Tf: [], blr.graph(N, [], priors, betweens), np.stack(X0), blr.params())
    print("terms alone:", r.status_name, r.iterations, r.trials, r.cost)
    assert ref["status"] != lmr.RUNNING and (r.status, r.iterations, r.trials) == (ref["status"], ref["iterations"], ref["trials"])
    assert r.factor_cost == 0.0 and r.num_inliers == 0 and r.cost < 1e-3 * blr.assemble(blr.graph(N, [], priors, betweens), np.stack(X0), [])["cost"]
    with pytest.raises(api.GlimAmdError) as e:  # neither factor nor term
        api.graph_align([], [], [], X0, ctx=ctx)
    assert e.value.code == -1
