"""Min-cut segmentation on the device (glim_amd/csrc/min_cut.hip, map_edit.hip) against scipy's maximum flow and the NumPy restatement
(tests/min_cut_restatement.py).  Every comparison is an equality: capacities are integers, and the minimal source side of a minimum cut is the
same set for every maximum flow.

Scene: a post of 500 points on a jittered ground plane of 2 400, dealt over 3 clouds with poses whose translations are of order 20 m; cloud 1
is an FP32 cloud, the others keep FP64 points; the clouds with normals are FP32 clouds throughout.  Parameters: foreground radius 0.5,
background radius 2.0, weight 10, sigma_d 0.25, k 8.

Figures of the scene (computed by the tests on the CPU): 1 860 candidates, 8 817 edges, 310 foreground and 812 background points, maximum flow
822 027 units, segment 512 points (the post and a collar of ground), 64 push rounds in 2 chunks; smallest margins: weight 7.0e-5 of a unit
from a quantisation step's middle (required: > 1e-6), relative gap between a k-th and (k+1)-th neighbour distance 7.1e-5 (> 1e-5), qq 7.0e-5
relative from a squared radius (> 1e-9).
"""
import numpy as np
import pytest

import min_cut_restatement as M

R = M.R
pytestmark = pytest.mark.gpu

SCENE_SEED = 2
COUNT_KEYS = ("num_candidates", "num_edges", "num_foreground", "num_background")


@pytest.fixture(scope="module")
def ctx():
    from glim_amd import api

    return api.Context(0, 1)


def _params(api, p):
    return api.MinCutParams(**p)


@pytest.fixture(scope="module")
def scene(ctx):
    from glim_amd import api

    clouds, poses, _ = M.make_scene(SCENE_SEED)
    gpu = [api.PointCloudGPU.clone(p.astype(np.float32), ctx=ctx) if s == 1 else api.clone_exact(p, ctx=ctx) for s, p in enumerate(clouds)]
    want = M.min_cut(clouds, poses, M.CENTER)
    assert M.graph_margins_hold(want["graph"]["margins"]), want["graph"]["margins"]  # a condition on the scene, not a tolerance
    return {"clouds": clouds, "poses": poses, "gpu": gpu, "want": want}


@pytest.fixture(scope="module")
def normal_scene(ctx):
    from glim_amd import api

    clouds, poses, normals = M.make_scene(SCENE_SEED, fp32=True)
    gpu = [api.PointCloudGPU.clone(p.astype(np.float32), normals=n, ctx=ctx) for p, n in zip(clouds, normals)]
    return {"clouds": clouds, "poses": poses, "normals": normals, "gpu": gpu}


def _same_counts(got, want):
    for k in COUNT_KEYS + ("status",):
        assert got[k] == want[k], (k, got[k], want[k])


# ---- the solver alone ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.tiny_graphs()))
def test_the_solver_alone_equals_scipy(ctx, name):
    from glim_amd import api

    n, edges, cap, src, snk = M.tiny_graphs()[name]
    flow, flags = M.judge(n, edges, cap, src, snk)
    want = M.solve(n, edges, cap, src, snk)
    got = api.diag_max_flow(ctx, n, edges, cap, src, snk)
    print(name, "flow", got["flow"], "against", flow, "members", int(got["member"].sum()), "against", int(flags.sum()), "rounds", got["rounds"], "looks", got["looks"])
    assert got["status"] == "ok" and got["flow"] == flow
    np.testing.assert_array_equal(got["member"], flags)
    assert (got["rounds"], got["looks"]) == (want["rounds"], want["looks"])  # the restatement follows the device round for round
    again = api.diag_max_flow(ctx, n, edges, cap, src, snk)
    assert again["member"].tobytes() == got["member"].tobytes() and again["flow"] == got["flow"]


def test_the_grids_tell_the_minimal_from_the_maximal_cut_and_one_round_is_a_round_limit(ctx):
    from glim_amd import api

    differ = 0
    for seed in range(1, 7):
        n, edges, cap, src, snk = M.grid_graph(seed)
        assert (src > 0).sum() == 4 and (snk > 0).sum() == 6 and cap.min() == 0 and cap.max() == 3
        differ += int(M.judge(n, edges, cap, src, snk, maximal=True)[1].sum() > M.judge(n, edges, cap, src, snk)[1].sum())
    assert differ >= 2
    n, edges, cap, src, snk = M.long_chain()
    assert n == 2 * api.EDIT_ROUNDS_PER_LOOK + 5 and api.diag_max_flow(ctx, n, edges, cap, src, snk)["looks"] > 1
    cut = api.diag_max_flow(ctx, n, edges, cap, src, snk, max_rounds=1)
    assert cut["status"] == "round_limit" and cut["rounds"] == 1 and cut["flow"] == 0 and not cut["member"].any()
    # a loop, an endpoint out of range, a negative capacity: refused
    for bad_edges, bad_cap in (([(1, 1)], [1]), ([(0, 3)], [1]), ([(0, 1)], [-1])):
        with pytest.raises(api.GlimAmdError) as e:
            api.diag_max_flow(ctx, 3, bad_edges, bad_cap, [1, 0, 0], [0, 0, 1])
        assert e.value.code == -1
    empty = api.diag_max_flow(ctx, 0, [], [], [], [])
    assert empty["flow"] == 0 and empty["status"] == "ok" and len(empty["member"]) == 0


# ---- the graph -----------------------------------------------------------------------------------------------------------------------------------
def test_the_graph_equals_the_restatement_with_and_without_normals(scene, normal_scene):
    from glim_amd import api

    for sc, prm, normals in ((scene, M.PARAMS, None), (normal_scene, dict(M.PARAMS, use_normals=True), normal_scene["normals"])):
        want = M.graph(sc["clouds"], sc["poses"], M.CENTER, prm, normals)
        print("normals" if normals else "plain", {k: want[k] for k in COUNT_KEYS}, "margins", want["margins"])
        # conditions on the scene, asserted before anything is compared
        assert want["margins"]["weight"] > 1e-6 and want["margins"]["neighbour_gap"] > 1e-5 and want["margins"]["qq"] > 1e-9
        got = api.diag_edit_min_cut_graph(sc["gpu"], sc["poses"], M.CENTER, _params(api, prm))
        _same_counts(got, want)
        np.testing.assert_array_equal(got["candidates"], want["candidates"])
        np.testing.assert_array_equal(got["edges"], want["edges"])
        np.testing.assert_array_equal(got["edge_cap"], want["cap"])
        np.testing.assert_array_equal(got["source_cap"], want["src"])
        np.testing.assert_array_equal(got["sink_cap"], want["snk"])
        assert (got["edges"][:, 0] < got["edges"][:, 1]).all() and (np.diff(R.pack_ids(got["edges"]).astype(np.int64)) > 0).all()
    plain = M.graph(normal_scene["clouds"], normal_scene["poses"], M.CENTER)
    assert (want["cap"] < plain["cap"]).any()  # the normals change capacities


# ---- the whole call ------------------------------------------------------------------------------------------------------------------------------
def test_the_segment_equals_the_restatement_and_scipy_on_the_downloaded_graph(scene):
    from glim_amd import api

    gpu, poses, want = scene["gpu"], scene["poses"], scene["want"]
    prm = _params(api, M.PARAMS)
    got = api.edit_min_cut(gpu, poses, M.CENTER, prm)
    print({k: got[k] for k in COUNT_KEYS + ("count", "flow", "rounds", "looks", "status")})
    # the scene is not trivial
    assert want["flow"] > 0 and want["num_foreground"] < want["count"] < want["num_candidates"]
    _same_counts(got, want)
    assert got["count"] == want["count"] and got["flow"] == want["flow"]
    np.testing.assert_array_equal(got["pairs"], want["pairs"])
    assert (got["rounds"], got["looks"]) == (want["rounds"], want["looks"])
    # the judge on the graph the device built
    g = api.diag_edit_min_cut_graph(gpu, poses, M.CENTER, prm)
    flow, flags = M.judge(g["num_candidates"], g["edges"], g["edge_cap"], g["source_cap"], g["sink_cap"])
    assert got["flow"] == flow
    np.testing.assert_array_equal(got["pairs"], g["candidates"][flags == 1])
    # capacities below the count: the prefix, and the true count
    part = api.edit_min_cut(gpu, poses, M.CENTER, prm, capacity=37)
    assert part["count"] == want["count"] and part["flow"] == want["flow"]
    np.testing.assert_array_equal(part["pairs"], want["pairs"][:37])
    none = api.edit_min_cut(gpu, poses, M.CENTER, prm, capacity=0)
    assert none["count"] == want["count"] and len(none["pairs"]) == 0
    # two calls: the same bytes
    again = api.edit_min_cut(gpu, poses, M.CENTER, prm)
    assert again["pairs"].tobytes() == got["pairs"].tobytes() and again["flow"] == got["flow"] and again["count"] == got["count"]
    # too few rounds: a status, nothing selected
    assert M.min_cut(scene["clouds"], poses, M.CENTER, dict(M.PARAMS, max_rounds=3))["status"] == M.ROUND_LIMIT
    short = api.edit_min_cut(gpu, poses, M.CENTER, _params(api, dict(M.PARAMS, max_rounds=3)))
    assert short["status"] == "round_limit" and short["count"] == 0 and len(short["pairs"]) == 0 and short["rounds"] == 3


def test_statuses_and_refused_parameters(scene, normal_scene, ctx):
    from glim_amd import api

    gpu, poses, clouds = scene["gpu"], scene["poses"], scene["clouds"]
    prm = _params(api, M.PARAMS)
    # no sub-map
    none = api.edit_min_cut([], [], M.CENTER, prm, capacity=4)
    assert none["count"] == 0 and len(none["pairs"]) == 0 and none["status"] == "empty"
    # a window with no point
    empty = api.edit_min_cut(gpu, poses, [1000.0, 1000.0, 1000.0], prm)
    assert empty["status"] == "empty" and empty["count"] == 0 and empty["num_candidates"] == 0
    # fewer than k + 1 candidates
    few = R.CENTER + np.arange(5)[:, None] * np.array([0.1, 0.0, 0.0])
    got = api.edit_min_cut([api.clone_exact(few, ctx=ctx)], [np.eye(4)], R.CENTER, prm)
    assert M.min_cut([few], [np.eye(4)], R.CENTER)["status"] == M.FEW_POINTS
    assert got["status"] == "few_points" and got["count"] == 0 and got["num_candidates"] == 5
    # nothing inside the foreground radius of the picked point
    off = M.BASE + np.array([1.0, 1.0, 1.0])
    want = M.min_cut(clouds, poses, off)
    got = api.edit_min_cut(gpu, poses, off, prm)
    assert want["status"] == M.NO_SEED and want["num_candidates"] > 1000
    _same_counts(got, want)
    assert got["count"] == 0 and got["flow"] == 0 and len(got["pairs"]) == 0
    # use_normals on clouds without normals; with normals the call runs and equals the restatement
    with_normals = dict(M.PARAMS, use_normals=True)
    with pytest.raises(api.GlimAmdError) as e:
        api.edit_min_cut(gpu, poses, M.CENTER, _params(api, with_normals))
    assert e.value.code == -5
    ns = normal_scene
    want = M.min_cut(ns["clouds"], ns["poses"], M.CENTER, with_normals, ns["normals"])
    got = api.edit_min_cut(ns["gpu"], ns["poses"], M.CENTER, _params(api, with_normals))
    _same_counts(got, want)
    assert got["flow"] == want["flow"] and got["count"] == want["count"]
    np.testing.assert_array_equal(got["pairs"], want["pairs"])
    # each invalid parameter
    bad = [dict(distance_sigma=0.0), dict(distance_sigma=np.nan), dict(angle_sigma=-1.0), dict(angle_sigma=np.inf), dict(foreground_mask_radius=0.0),
           dict(foreground_mask_radius=2.0), dict(foreground_mask_radius=3.0), dict(background_mask_radius=np.inf), dict(foreground_weight=0.0),
           dict(foreground_weight=-1.0), dict(foreground_weight=np.nan), dict(background_weight=-1.0), dict(k_neighbors=0), dict(max_rounds=-1),
           dict(foreground_weight=32768.0), dict(background_weight=1e9)]
    for change in bad:
        with pytest.raises(api.GlimAmdError) as e:
            api.edit_min_cut(gpu, poses, M.CENTER, _params(api, dict(M.PARAMS, **change)))
        assert e.value.code == -1, change
    with pytest.raises(api.GlimAmdError) as e:
        api.edit_min_cut(gpu, poses, M.CENTER, _params(api, dict(M.PARAMS, k_neighbors=32)))
    assert e.value.code == -6
    assert api.edit_min_cut(gpu, poses, M.CENTER, _params(api, dict(M.PARAMS, k_neighbors=31)))["status"] == "ok"


def test_segment_remove_and_segment_again(scene):
    from glim_amd import api

    gpu, poses, clouds, first = scene["gpu"], scene["poses"], scene["clouds"], scene["want"]
    prm = _params(api, M.PARAMS)
    cut = api.edit_min_cut(gpu, poses, M.CENTER, prm)
    np.testing.assert_array_equal(cut["pairs"], first["pairs"])
    edited = api.edit_remove_selected(gpu, cut["pairs"])
    kept = [R.remove(clouds[s], cut["pairs"][cut["pairs"][:, 0] == s, 1]) for s in range(3)]
    for s in range(3):
        assert edited[s].size() == len(kept[s]) < len(clouds[s])
    # at the same point the post is gone: no seed
    want = M.min_cut(kept, poses, M.CENTER)
    got = api.edit_min_cut(edited, poses, M.CENTER, prm)
    assert want["status"] == M.NO_SEED and M.graph_margins_hold(want["graph"]["margins"])
    _same_counts(got, want)
    assert got["count"] == 0
    # a patch of ground beside it, with smaller radii
    point = M.BASE + np.array([1.5, -1.0, 0.0])
    small = dict(M.PARAMS, foreground_mask_radius=0.3, background_mask_radius=1.0)
    want = M.min_cut(kept, poses, point, small)
    print({k: want[k] for k in COUNT_KEYS + ("count", "flow", "rounds", "looks", "status")}, want["graph"]["margins"])
    assert want["status"] == M.OK and want["flow"] > 0 and 0 < want["count"] < want["num_candidates"] and M.graph_margins_hold(want["graph"]["margins"])
    got = api.edit_min_cut(edited, poses, point, _params(api, small))
    _same_counts(got, want)
    assert got["flow"] == want["flow"] and got["count"] == want["count"]
    np.testing.assert_array_equal(got["pairs"], want["pairs"])
