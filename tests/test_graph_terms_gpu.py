"""Damping terms and Huber between terms on the device (include/glim_amd.h "Damping terms and Huber between terms"): glim_amd_bundle_align_terms
(one workgroup, the system in LDS) and glim_amd_graph_align_terms (launches, the systems in device memory).

Graphs with factors are those of tests/test_graph_align_gpu.py (clouds of 256 points, the factors (i, j) with 0 < j - i <= 2, a between chain
of precision 1e3) with the prior of pose 0 replaced by a damping of 1e6, chain between 10 falsified by Exp(0.1 FALSIFY) under a width of 1.0
(s is about 7 there) and chain between 20 under a width of 50 (never reached: the branch k > 0, s <= k).  The pose graphs are
tests/graph_terms_restatement.py's ring_scene; what a comparison with the restatement rests on -- no between within 1e-6 of its width at any
trial, cond(H) <= 1e9 at the kept systems -- is asserted on the restatement's own run."""
import ctypes as C

import numpy as np
import pytest

import graph_terms_restatement as gtr
import lm_restatement as lmr
from align_cases import PERT_A, ctx, same_result  # noqa: F401 (ctx: a fixture)
from test_bundle_align_gpu import api_params, caller_set, pose44, problem, same_lin
from test_gicp import POSE_TOL
from test_graph_align_gpu import SHORT, graph_problem, same_rows
from test_graph_terms import COND_MAX, WIDTH_MARGIN, check_weights

pytestmark = pytest.mark.gpu
BUNDLE_MAX_POSES = 32
INVALID = -1


def terms_problem(orc, ctx, N):
    pr = dict(graph_problem(orc, ctx, N))
    widths = {10: 1.0, 20: 50.0}
    pr["betweens"] = [(i, j, D @ lmr.expmap(0.1 * gtr.FALSIFY) if q == 10 else D, L) + ((widths[q],) if q in widths else ())
                      for q, (i, j, D, L) in enumerate(pr["betweens"])]
    pr["priors"], pr["dampings"] = [], [(0, 1e6)]
    pr["g"] = gtr.graph(N, pr["pairs"], [], pr["betweens"], pr["dampings"])
    return pr


def run(which, pr, kw, **more):
    from glim_amd import api

    fn = api.bundle_align_debug_trace if which == "bundle" else api.graph_align_debug_trace
    return fn(pr["factors"], pr["priors"], pr["betweens"], list(pr["X0"]), 0, api_params(kw), dampings=pr.get("dampings", ()), **more)


def same_all(a, b):
    """two results hold the same bits, the weights included"""
    return same_result(a, b) and a.between_weights is not None and np.array_equal(a.between_weights, b.between_weights)


def raw_terms_call(entry, pr, kw, more):
    """the `_terms` entry point itself, so that `more` can be NULL"""
    from glim_amd import _lib, api

    betweens = [tuple(b[:4]) for b in pr["betweens"]]
    c, fa, ta, keep = api._bundle_args(pr["factors"], pr["priors"], betweens, list(pr["X0"]), None)
    F, N = fa[-1], ta[-1]
    prm = api_params(kw)._c()
    X_out, compact, out, w = np.zeros((N, 12)), np.zeros((F, _lib.COMPACT_DOUBLES)), _lib.BundleResult(), np.full(len(betweens), np.nan)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    api.check(getattr(_lib.lib(), entry)(*fa, 0, *ta, C.byref(prm), dp(X_out), dp(compact), C.byref(out), more, dp(w)), entry)
    return api.BundleResult(out, api._poses44(X_out), compact, w)


# ---- 1. no new term ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,N", [("bundle", 4), ("graph", 33)])
def test_without_a_new_term_the_new_entry_points_return_the_old_bits(orc, ctx, which, N):
    from glim_amd import api

    pr = problem(orc, ctx, 4, 0.5, PERT_A, chain=1e3) if which == "bundle" else graph_problem(orc, ctx, 33)
    kw = dict(max_iterations=2)
    old = getattr(api, which + "_align")(pr["factors"], pr["priors"], pr["betweens"], list(pr["X0"]), 0, api_params(kw))
    assert old.between_weights is None and old.iterations >= 1
    null = raw_terms_call(f"glim_amd_{which}_align_terms", pr, kw, None)
    assert same_result(old, null) and np.array_equal(null.between_weights, np.ones(len(pr["betweens"])))
    zero = dict(pr, betweens=[b + (0.0,) for b in pr["betweens"]])  # no damping and a width array of zeros, through the mirror
    res, rows, _ = run(which, zero, kw)
    assert same_result(old, res) and np.array_equal(res.between_weights, np.ones(len(pr["betweens"])))
    _, rows_old, _ = run(which, pr, kw)
    assert same_rows(rows, rows_old)


# ---- 2. at the bundle's cap --------------------------------------------------------------------------------------------------------------------
def test_at_the_bundles_cap_the_two_paths_agree_bit_for_bit(orc, ctx):
    from glim_amd import api

    pr = terms_problem(orc, ctx, BUNDLE_MAX_POSES)
    kw = dict(max_iterations=2)
    a, rows_a, _ = run("bundle", pr, kw)
    b, rows_b, _ = run("graph", pr, kw)
    print("N", BUNDLE_MAX_POSES, b.status_name, b.iterations, b.trials, "cost", b.cost, "weights", b.between_weights[[10, 20]])
    assert same_all(a, b) and same_rows(rows_a, rows_b) and b.iterations >= 1 and b.num_inliers > 0
    assert b.between_weights[10] < 0.5 and np.count_nonzero(b.between_weights != 1.0) == 1
    args = (pr["factors"], [], pr["betweens"], list(pr["X0"]), 0, api_params(kw))
    assert same_all(api.bundle_align(*args, dampings=pr["dampings"]), a) and same_all(api.graph_align(*args, dampings=pr["dampings"]), a)  # the stable entries
    fset = caller_set(ctx, pr)
    values = {k: x for k, x in enumerate(pr["X0"])}
    got, res = fset.optimize_graph(values, [], pr["betweens"], api_params(kw), dampings=pr["dampings"])
    assert same_all(res, b) and all(np.array_equal(got[k], b.poses[k]) for k in values)  # the set's own entry is the same call
    fset.close()


# ---- 3. beyond the cap -------------------------------------------------------------------------------------------------------------------------
def teacher_forced(ctx, pr, res, rows, p):
    """tests/test_bundle_align_gpu.py's teacher_forced over the extended restatement: every trace record is the caller's set's at the traced
    T_f; the restatement, fed the device's records from the device's own previous state, decides the same and proposes the same candidates
    within pose_gate; no between is within WIDTH_MARGIN of its width at a traced evaluation"""
    from glim_amd import api

    g = pr["g"]
    fset = caller_set(ctx, pr)
    s = gtr.blr.new_state(pr["X0"], p)
    k_w = np.array(g["widths"])
    assert len(rows) == res.trials + 1
    for k, e in enumerate(rows):
        records = fset.linearize_poses(e["Tf"])
        mine = [api.expand_compact(c, Tf, api.FACTOR_BINARY) for c, Tf in zip(e["compact"], e["Tf"])]
        assert same_lin(mine, records), k
        assert e["lam"] == s["lam"], k
        if k == 0:
            assert np.array_equal(e["X"], pr["X0"])
        else:
            gate = lmr.pose_gate(s)
            assert np.abs(e["X"] - s["cand"]).max() <= gate, (k, np.abs(e["X"] - s["cand"]).max(), gate)
        s["cand"] = e["X"]  # teacher forcing: the device's poses are the ones the records belong to
        recs = [lmr.record_of_compact(c) for c in e["compact"]]
        s = gtr.step(p, g, s, recs)
        assert (e["accepted"], e["status"]) == (s["accepted"], s["status"]), k
        S = gtr.assemble(g, e["X"], recs)
        assert (np.abs(S["s"] - k_w)[k_w > 0] / k_w[k_w > 0]).min() > WIDTH_MARGIN and np.linalg.cond(s["sys"]["H"]) <= COND_MAX, k
        assert abs(e["cost"] - S["cost"]) <= 1e-9 * abs(S["cost"]), k
    fset.close()
    assert s["status"] != lmr.RUNNING and (res.status, res.iterations, res.trials) == (s["status"], s["iterations"], s["trials"])
    assert np.array_equal(res.poses, s["X"]) and res.lam == s["lam"]
    check_weights(res.between_weights, s["sys"]["weights"])
    assert abs(res.between_cost - s["sys"]["bcost"]) <= 1e-9 * s["sys"]["bcost"] and res.cost == (res.factor_cost + res.prior_cost) + res.between_cost
    return s


def test_beyond_the_cap_every_round_is_the_one_thread_round_and_the_hosts_decision(orc, ctx):
    pr = terms_problem(orc, ctx, 33)
    a, rows_a, _ = run("graph", pr, SHORT)
    b, rows_b, _ = run("graph", pr, SHORT, one_thread=True)
    print("N 33", a.status_name, a.iterations, a.trials, "inliers", a.num_inliers, "cost", a.cost, "weights", a.between_weights[[10, 20]])
    assert same_all(a, b) and same_rows(rows_a, rows_b) and a.iterations >= 1
    s = teacher_forced(ctx, pr, a, rows_a, gtr.params(**SHORT))
    assert s["iterations"] >= 1 and a.between_weights[10] < 0.5 and a.between_weights[20] == 1.0


# ---- 4. terms only -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,N", [("bundle", 8), ("graph", 33), ("graph", 64)])
def test_the_pose_graph_scene_ends_as_the_restatement_does(ctx, which, N):
    from glim_amd import api

    g, betweens, dampings, X0, _ = gtr.ring_scene(N)
    ref, trace = gtr.run(lambda Tf: [], g, X0)
    assert gtr.width_margin(g, trace) > WIDTH_MARGIN and all(np.linalg.cond(e["state"]["sys"]["H"]) <= COND_MAX for e in trace)
    r = getattr(api, which + "_align")([], [], betweens, list(X0), dampings=dampings, ctx=ctx)
    print("N", N, r.status_name, r.iterations, r.trials, "cost", r.cost, "weights", r.between_weights[N - 1:], "pose 0 moves", np.abs(r.poses[0] - X0[0]).max(),
          "|dX|", np.abs(r.poses - ref["X"]).max())
    assert ref["status"] == lmr.CONVERGED and (r.status, r.iterations, r.trials) == (ref["status"], ref["iterations"], ref["trials"])
    assert np.abs(r.poses - ref["X"]).max() <= POSE_TOL
    check_weights(r.between_weights, ref["sys"]["weights"])
    assert np.count_nonzero(r.between_weights != 1.0) == (2 if N == 64 else 1)
    at = gtr.assemble(g, r.poses, [])  # the restatement AT the device's poses
    gauss = gtr.assemble(dict(g, widths=[0.0] * len(betweens)), r.poses, [])
    assert abs(r.between_cost - at["bcost"]) <= 1e-9 * at["bcost"] and r.between_cost < 0.5 * gauss["bcost"]  # the robust cost, not r^T L r
    assert r.cost == (0.0 + 0.0) + r.between_cost and r.factor_cost == 0.0 and r.prior_cost == 0.0 and r.num_inliers == 0
    assert np.abs(r.poses[0] - X0[0]).max() < 1e-9


# ---- 5. kept weights ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,N,noise", [("bundle", 8, 1.0), ("graph", 33, 0.6)])
def test_after_a_rejected_last_trial_the_weights_are_those_of_the_kept_poses(ctx, which, N, noise):
    """the ring scene started far off (every pose but the first times Exp of noise of that size): the restatement's trials are A r r r r ...;
    with a budget of two trials the loop ends on a rejected one"""
    g, betweens, dampings, X0, _ = gtr.ring_scene(N)
    rng = np.random.default_rng(8)
    X0 = np.stack([X0[0]] + [x @ lmr.expmap(rng.normal(0, noise, 6)) for x in X0[1:]])
    kw = dict(max_trials=2)
    ref, trace = gtr.run(lambda Tf: [], g, X0, gtr.params(**kw))
    assert [e["accepted"] for e in trace] == [True, False, False] and ref["status"] == lmr.MAX_TRIALS
    assert gtr.width_margin(g, trace) > WIDTH_MARGIN and np.linalg.cond(ref["sys"]["H"]) <= COND_MAX
    assert min(abs(e["cost"] - trace[0]["cost"]) / trace[0]["cost"] for e in trace[1:]) > 0.5  # the rejections are no close calls
    pr = dict(factors=[], priors=[], betweens=betweens, dampings=dampings, X0=X0)
    a, rows_a, _ = run(which, pr, kw, ctx=ctx)
    b, rows_b, _ = run(which, pr, kw, ctx=ctx, one_thread=True)
    assert [e["accepted"] for e in rows_a] == [True, False, False] and (a.status, a.iterations, a.trials) == (lmr.MAX_TRIALS, 0, 2)
    assert same_all(a, b) and same_rows(rows_a, rows_b) and np.array_equal(a.poses, X0)
    kept, last = gtr.assemble(g, a.poses, [])["weights"], gtr.assemble(g, rows_a[-1]["X"], [])["weights"]
    assert np.abs(kept - last).max() > 1e-3  # the last evaluation's weights are others
    check_weights(a.between_weights, kept)


# ---- 6. a lone damped pose ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,N", [("bundle", 8), ("graph", 33)])
def test_a_pose_touched_only_by_a_damping_keeps_its_bits(orc, ctx, which, N):
    from glim_amd import api

    g, betweens, dampings, X0, _ = gtr.ring_scene(N)
    lone = X0[3] @ lmr.expmap(np.array([0.3, -0.2, 0.1, 5.0, -4.0, 3.0]))
    pr = dict(factors=[], priors=[], betweens=betweens, dampings=dampings + [(N, [5.0, 4.0, 3.0, 2.0, 1.0, 0.5])], X0=np.concatenate([X0, lone[None]]))
    kw = dict(max_iterations=3)
    a, rows, _ = run(which, pr, kw, ctx=ctx)
    want, _, _ = run(which, dict(pr, dampings=dampings, X0=X0), kw, ctx=ctx)
    assert a.iterations == 3 and np.array_equal(a.poses[N], lone) and all(np.array_equal(e["X"][N], lone) for e in rows)
    assert np.array_equal(a.poses[:N], want.poses) and np.array_equal(a.between_weights, want.between_weights) and a.cost == want.cost  # (block-diagonal: the same solve)
    for dampings_only in ([(0, 1.0)], [(0, 1.0), (N, 2.0)]):
        with pytest.raises(api.GlimAmdError) as e:  # nothing to optimise over
            getattr(api, which + "_align")([], [], [], list(pr["X0"]), dampings=dampings_only, ctx=ctx)
        assert e.value.code == INVALID
        again, _, _ = run(which, pr, kw, ctx=ctx)
        assert same_all(again, a)  # the next valid call still works


# ---- 7. the chunk length -----------------------------------------------------------------------------------------------------------------------
def test_the_chunk_length_moves_no_bit_with_the_terms(orc, ctx):
    pr = terms_problem(orc, ctx, 33)
    kw = dict(max_iterations=3)
    a, rows_a, raw_a = run("graph", pr, kw)
    b, rows_b, raw_b = run("graph", pr, kw, rounds_per_chunk=1)
    c, rows_c, _ = run("graph", pr, kw, rounds_per_chunk=64)  # longer than the loop: all rounds up front
    assert same_all(a, b) and same_rows(rows_a, rows_b) and same_all(a, c) and same_rows(rows_a, rows_c) and a.trials >= 2
    for x, y in zip(raw_a[:3], raw_b[:3]):
        assert np.array_equal(x, y)
