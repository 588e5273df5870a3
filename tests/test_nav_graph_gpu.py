"""Velocity and bias variables, vector priors, vector betweens and IMU terms on the device (include/glim_amd.h "Graph optimisation with velocity
and bias variables"; glim_amd_graph_align_nav): the workgroup form against the one-thread form, the trial records against a caller's factor
set, the device against the host header, the entry point without new terms against glim_amd_graph_align_terms, the chunk length, and a
velocity that overflows in the middle of a run.

The graphs are tests/nav_graph_restatement.py's.  Those with factors take the poses, the clouds of 256 points and the factors (i, j) with
0 < j - i <= 2 of tests/test_graph_align_gpu.py's problem at K frames; node 3k is frame k's pose."""
import numpy as np
import pytest

import nav_graph_restatement as nr
from align_cases import PERT_A, build_driver, ctx, same_result  # noqa: F401 (ctx: a fixture)
from test_bundle_align_gpu import api_params, caller_set, same_lin
from test_gicp import POSE_TOL
from test_graph_align_gpu import graph_problem, same_rows
from test_graph_terms_gpu import terms_problem
from test_nav_graph import cpp_step

pytestmark = pytest.mark.gpu
NUMERIC = 6
NAV_FIELDS = ("values12", "cost", "factor_cost", "prior_cost", "between_cost", "vector_prior_cost", "vector_between_cost", "imu_cost", "lam", "num_inliers",
              "iterations", "trials", "status", "compact", "between_weights")


def same_nav(a, b):
    """two results hold the same bits: nodes, the cost and its six parts, lambda, the counts, the status, the records and the weights"""
    return all(np.array_equal(np.asarray(getattr(a, f)), np.asarray(getattr(b, f))) for f in NAV_FIELDS)


def run(sc, kw, factors=(), **more):
    from glim_amd import api

    g = sc["g"]
    vp, vb, im = nr.api_terms(g)
    betweens = [b + (w,) for b, w in zip(g["betweens"], g["widths"])]
    return api.graph_align_nav_debug_trace(list(factors), g["priors"], betweens, nr.api_nodes(sc["kinds"], sc["X0"]), sc["kinds"], vp, vb, im, g["dampings"], 0,
                                           api_params(kw), **more)


def factor_scene(orc, ctx, K):
    """the sub-map shape over the K frames of graph_problem, with its factors on the pose nodes"""
    pr = graph_problem(orc, ctx, K)
    sc = nr.submap_scene(K, PERT_A, poses=pr["truth"], pairs=pr["pairs"])
    factors = [(vm, cloud, 3 * i, 3 * j) for vm, cloud, i, j in pr["factors"]]
    return pr, sc, factors


@pytest.fixture(scope="module")
def step_exe(tmp_path_factory):
    return build_driver(tmp_path_factory, "nav_graph_step", "-Wno-unknown-pragmas")


# ---- 8. the workgroup form against the one-thread form -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 20])  # 72 rows; 360 rows: six tiles, the last one ragged
def test_the_launches_return_the_one_thread_forms_bits_and_a_callers_records(orc, ctx, K):
    """Nodes, the cost and its parts, the trace and the weights; and every trial record is what NonlinearFactorSetGPU.linearize_poses returns
    for the same pairs at the traced relative poses, blocks included.  At most three rounds: the one-thread form takes about a second per
    round at 360 rows."""
    from glim_amd import api

    pr, sc, factors = factor_scene(orc, ctx, K)
    kw = dict(max_iterations=2, max_trials=2)
    a, rows_a, _ = run(sc, kw, factors)
    b, rows_b, _ = run(sc, kw, factors, one_thread=True)
    print("K", K, a.status_name, a.iterations, a.trials, "inliers", a.num_inliers, "cost", a.cost, "parts", a.factor_cost, a.prior_cost, a.between_cost,
          a.vector_prior_cost, a.vector_between_cost, a.imu_cost)
    assert same_nav(a, b) and same_rows(rows_a, rows_b) and a.iterations >= 1 and len(rows_a) == a.trials + 1
    assert a.imu_cost > 0 and a.vector_prior_cost > 0 and a.num_inliers > 10 * len(factors)
    assert a.cost == ((((a.factor_cost + a.prior_cost) + a.between_cost) + a.vector_prior_cost) + a.vector_between_cost) + a.imu_cost
    assert np.array_equal(a.between_weights, np.ones(len(sc["g"]["betweens"])))
    fset = caller_set(ctx, pr)
    for k, e in enumerate(rows_a):
        records = fset.linearize_poses(e["Tf"])
        mine = [api.expand_compact(c, Tf, api.FACTOR_BINARY) for c, Tf in zip(e["compact"], e["Tf"])]
        assert same_lin(mine, records), k
        want = np.stack([np.linalg.inv(nr.pose_of(e["X"][3 * i])) @ nr.pose_of(e["X"][3 * j]) for i, j in pr["pairs"]])
        assert np.abs(np.stack([nr.pose_of(Tf) for Tf in e["Tf"]]) - want).max() <= 1e-12, k
    fset.close()
    plain = api.graph_align_nav(factors, sc["g"]["priors"], [q + (0.0,) for q in sc["g"]["betweens"]], nr.api_nodes(sc["kinds"], sc["X0"]), sc["kinds"],
                                *nr.api_terms(sc["g"]), params=api_params(kw))
    assert same_nav(plain, a)  # the entry point without the trace
    if K == 4:  # a factor on a vector node is refused (it needs handles, so it is asked here)
        with pytest.raises(api.GlimAmdError) as err:
            run(sc, kw, [factors[0][:3] + (1,)] + factors[1:])
        assert err.value.code == -1


# ---- 9. the device against the host header -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,mode", [("sub-map 4", nr.TANGENT), ("sub-map 20", nr.MANIFOLD), ("global 5", nr.TANGENT), ("global 5", nr.MANIFOLD)])
def test_the_device_decides_as_the_host_header_and_ends_at_the_truth(ctx, step_exe, tmp_path, scene, mode):
    """The graphs of tests/test_nav_graph.py without factors, with its loop parameters (nr.LOOP): the same decisions, counts, statuses and
    lambda round by round as glim_amd/csrc/bundle_lm_step.hpp under a plain C++ compiler; the final nodes within POSE_TOL of the host's and
    of the truth (velocities in m/s and biases in their units by the same number)."""
    from test_nav_graph import SCENES

    sc = SCENES[scene](mode)
    res, rows, _ = run(sc, nr.LOOP)
    host = cpp_step(step_exe, tmp_path, nr.params(**nr.LOOP), sc["g"], sc["X0"], [[] for _ in rows])
    print(scene, res.status_name, res.iterations, res.trials, "cost", res.cost, "error", nr.node_error(sc["kinds"], res.values12, sc["truth"]))
    assert len(rows) == res.trials + 1 and res.status == nr.CONVERGED and res.iterations >= 2
    lam = [nr.params(**nr.LOOP)["lambda_initial"]] + [h["lam"] for h in host]  # a trace row carries the lambda its round began with
    for k, (d, h) in enumerate(zip(rows, host)):
        assert (d["accepted"], d["status"], d["lam"]) == (h["accepted"], h["status"], lam[k]), k
    assert res.lam == host[-1]["lam"]
    assert (res.iterations, res.trials, res.status) == (host[-1]["iterations"], host[-1]["trials"], host[-1]["status"])
    assert nr.node_error(sc["kinds"], res.values12, host[-1]["X"]) <= POSE_TOL and nr.node_error(sc["kinds"], res.values12, sc["truth"]) <= POSE_TOL
    assert abs(res.cost - host[-1]["cost"]) <= 1e-9 * max(host[0]["cost"], 1.0)
    tails = np.array([k != nr.POSE for k in sc["kinds"]])[:, None] & (np.arange(12)[None, :] >= np.array([nr.dim(k) for k in sc["kinds"]])[:, None])
    assert not res.values12[tails].any() and not np.signbit(res.values12[tails]).any()  # returned as +0.0
    assert isinstance(res.nodes[1], np.ndarray) and res.nodes[0].shape == (4, 4)


# ---- 10. without new terms ---------------------------------------------------------------------------------------------------------------------
def test_with_poses_alone_the_entry_point_returns_graph_align_terms_bits(orc, ctx):
    from glim_amd import api

    pr = terms_problem(orc, ctx, 12)
    kw = dict(max_iterations=3)
    old = api.graph_align(pr["factors"], pr["priors"], pr["betweens"], list(pr["X0"]), 0, api_params(kw), dampings=pr["dampings"])
    new = api.graph_align_nav(pr["factors"], pr["priors"], pr["betweens"], list(pr["X0"]), [nr.POSE] * 12, dampings=pr["dampings"], params=api_params(kw))
    print(old.status_name, old.iterations, old.trials, "cost", old.cost, "weights", old.between_weights[old.between_weights != 1.0])
    assert old.between_weights is not None and old.iterations >= 1 and (old.between_weights != 1.0).any()
    for f in ("cost", "factor_cost", "prior_cost", "between_cost", "lam", "num_inliers", "iterations", "trials", "status"):
        assert getattr(old, f) == getattr(new, f), f
    assert np.array_equal(old.compact, new.compact) and np.array_equal(old.between_weights, new.between_weights)
    assert np.array_equal(np.stack([x[:3].reshape(-1) for x in old.poses]), new.values12)
    assert (new.vector_prior_cost, new.vector_between_cost, new.imu_cost) == (0.0, 0.0, 0.0)
    old_t, rows_old, _ = api.graph_align_debug_trace(pr["factors"], pr["priors"], pr["betweens"], list(pr["X0"]), 0, api_params(kw), dampings=pr["dampings"])
    new_t, rows_new, _ = api.graph_align_nav_debug_trace(pr["factors"], pr["priors"], pr["betweens"], list(pr["X0"]), [nr.POSE] * 12, dampings=pr["dampings"],
                                                         params=api_params(kw))
    assert len(rows_old) == len(rows_new) and all(np.array_equal(np.stack([x[:3].reshape(-1) for x in a["X"]]), b["X"]) and np.array_equal(a["Tf"], b["Tf"]) and
                                                  np.array_equal(a["compact"], b["compact"]) and
                                                  (a["lam"], a["cost"], a["accepted"], a["status"]) == (b["lam"], b["cost"], b["accepted"], b["status"])
                                                  for a, b in zip(rows_old, rows_new))


# ---- 11. the chunk length ----------------------------------------------------------------------------------------------------------------------
def test_the_chunk_length_moves_no_bit(ctx):
    sc = nr.global_scene(5, PERT_A)
    ref, rows_ref, _ = run(sc, nr.LOOP)
    assert ref.iterations >= 2
    for chunk in (1, 4, 64):
        res, rows, _ = run(sc, nr.LOOP, rounds_per_chunk=chunk)
        assert same_nav(res, ref) and same_rows(rows, rows_ref), chunk


# ---- 12. a value that stops being finite in the middle of a run --------------------------------------------------------------------------------
def test_a_velocity_that_overflows_ends_numeric_with_the_kept_nodes(ctx, step_exe, tmp_path):
    """Two velocities at 1.7e308 m/s, a prior that holds the first and a between that asks the second to be 1e307 larger, informations 1e-310 so
    that the cost (1e304) is finite: round 0 is kept, its step is finite (1e307) and the retraction overflows.  GLIM_AMD_ALIGN_NUMERIC, and
    the nodes returned are the kept ones -- the initial ones, bit for bit; the host header does the same."""
    big, L = 1.7e308, 1e-310 * np.eye(3)
    kinds = [nr.VELOCITY, nr.VELOCITY]
    g = nr.graph(2, kinds, vpriors=[(0, [big, 0, 0], L)], vbetweens=[(0, 1, [1e307, 0, 0], L)])
    sc = {"g": g, "kinds": kinds, "X0": np.stack([nr.row_of(nr.VELOCITY, [big, 0, 0])] * 2)}
    kw = dict(lambda_initial=1e-320)
    host = cpp_step(step_exe, tmp_path, nr.params(**kw), g, sc["X0"], [[]] * 2)
    assert host[0]["accepted"] and host[0]["status"] == NUMERIC and 9e306 < host[0]["delta"][6] < 1.1e307 and np.isinf(host[0]["cand"][1, 0])
    for one_thread in (False, True):
        res, rows, _ = run(sc, kw, one_thread=one_thread)
        print(res.status_name, res.trials, res.cost, res.values12[:, 0])
        assert res.status == NUMERIC and res.trials == 0 and len(rows) == 1 and rows[0]["accepted"] and rows[0]["status"] == NUMERIC
        assert np.array_equal(res.values12, sc["X0"]) and res.cost == host[0]["cost"] and np.isfinite(res.cost)
