"""Map editing and the bundle-adjustment ball selection at map scale: the scenes of tests/map_scale_cases.py (whose docstring states their sizes
and what each is there to cross; tests/test_map_scale_cases.py holds those properties on the CPU) against tests/map_edit_restatement.py and
tests/plane_ba_restatement.py.  Selections, region growing and removal are compared by equality, the ball's sums by the two-order bound of
plane_ba_restatement.sum_bounds.
"""
import numpy as np
import pytest

import map_edit_restatement as R
import map_scale_cases as M
import plane_ba_restatement as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from glim_amd import api

    return api.Context(0, 1)


@pytest.fixture(scope="module")
def scene_a(ctx):
    """the 71 device clouds, built once"""
    from glim_amd import api

    sc = M.scene_a()
    sc["gpu"] = [api.clone_exact(p, ctx=ctx) if e else api.PointCloudGPU.clone(p.astype(np.float32), ctx=ctx) for p, e in zip(sc["clouds"], sc["exact"])]
    assert [g.size() for g in sc["gpu"]] == sc["sizes"]
    return sc


def _api_mode(api, mode):
    return {R.BOX: api.EDIT_BOX, R.SPHERE: api.EDIT_SPHERE, R.WINDOW: api.EDIT_WINDOW, R.WINDOW_BALL: api.EDIT_WINDOW_BALL}[mode]


# ---- scene A: selections ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.PREDICATES_A))
def test_each_mode_over_71_sub_maps_equals_the_restatement(scene_a, name):
    from glim_amd import api

    gpu, clouds, poses, total = scene_a["gpu"], scene_a["clouds"], scene_a["poses"], scene_a["total"]
    mode, kw, args = M.PREDICATES_A[name]
    if mode in (R.BOX, R.SPHERE):  # the restated matrices are the binding's
        for a, b in zip(M.local_matrices(R.MODEL, poses), api.edit_local_matrices(R.MODEL, poses)):
            assert a.tobytes() == b.tobytes()
    want, _ = R.select(clouds, M.matrices_a(mode, poses), *args)
    pairs, count = api.edit_select(gpu, poses, _api_mode(api, mode), **kw)
    print(name, "selected", count, "of", total)
    assert 0 < len(want) < total
    assert count == len(want)
    np.testing.assert_array_equal(pairs, want)
    assert np.isin(R.pack_ids(scene_a["forced"]), R.pack_ids(pairs)).all()
    cap = len(want) // 2 + 1  # a capacity below the count: the true count and the exact prefix
    part, count2 = api.edit_select(gpu, poses, _api_mode(api, mode), capacity=cap, **kw)
    assert count2 == count and len(part) == cap
    np.testing.assert_array_equal(part, want[:cap])


def test_everything_and_nothing_over_71_sub_maps(scene_a):
    from glim_amd import api

    gpu, poses, total = scene_a["gpu"], scene_a["poses"], scene_a["total"]
    mode, kw, _ = M.EVERYTHING
    one, count = api.edit_select(gpu, poses, _api_mode(api, mode), capacity=1, **kw)
    assert count == total and one.tolist() == [[1, 0]]  # sub-map 0 is empty
    pairs, count = api.edit_select(gpu, poses, _api_mode(api, mode), **kw)
    assert count == total and len(pairs) == total
    np.testing.assert_array_equal(pairs, M.all_pairs(scene_a["sizes"]))  # in order, the empty sub-maps skipped
    mode, kw, _ = M.NOTHING
    for cap in (None, 1):
        none, count = api.edit_select(gpu, poses, _api_mode(api, mode), capacity=cap, **kw)
        assert count == 0 and len(none) == 0


def test_ball_selection_and_statistics_over_71_sub_maps(scene_a):
    from glim_amd import api

    gpu, clouds, poses = scene_a["gpu"], scene_a["clouds"], scene_a["poses"]
    want, q = B.select(clouds, poses, M.CENTER, M.BALL_RADIUS)
    pairs, count = api.ba_ball_select(gpu, poses, M.CENTER, M.BALL_RADIUS)
    print("ball holds", count, "of", scene_a["total"])
    assert 0 < len(want) < scene_a["total"]
    assert count == len(want)
    np.testing.assert_array_equal(pairs, want)
    again, count2 = api.ba_ball_select(gpu, poses, M.CENTER, M.BALL_RADIUS)
    assert count2 == count and again.tobytes() == pairs.tobytes()
    cap = len(want) // 2 + 1
    part, count3 = api.ba_ball_select(gpu, poses, M.CENTER, M.BALL_RADIUS, capacity=cap)
    assert count3 == count and len(part) == cap
    np.testing.assert_array_equal(part, want[:cap])
    a = api.ba_ball_stats(gpu, poses, M.CENTER, M.BALL_RADIUS)
    b = api.ba_ball_stats(gpu, poses, M.CENTER, M.BALL_RADIUS)
    n, s, S = B.sums(q)
    bs, bS = B.sum_bounds(q)
    print("sum differences", np.abs(a["sum"] - s), "bounds", bs, "\ncross differences", np.abs(a["sum_cross"] - S).max(), "bound", bS.min())
    assert a["num_points"] == n
    assert (np.abs(a["sum"] - s) <= bs).all()
    assert (np.abs(a["sum_cross"] - S) <= bS).all()
    for k in ("sum", "sum_cross", "eigenvalues"):
        assert a[k].tobytes() == b[k].tobytes(), k


# ---- scene B: removal ------------------------------------------------------------------------------------------------------------------------
def test_removal_from_a_cloud_of_more_than_one_scan_chunk(ctx):
    from glim_amd import api

    sc = M.scene_b()
    n = M.N_B
    cloud = api.PointCloudGPU.clone(sc["points"], sc["covs"], sc["normals"], ctx=ctx)
    assert cloud.size() == n
    arrays = (sc["points"], sc["covs"], sc["normals"])
    idx = M.removal_indices_b()
    keep = np.ones(n, dtype=bool)
    keep[idx] = False
    new = api.edit_remove_points(cloud, idx)
    assert new.size() == keep.sum() and 0 < new.size() < M.CHUNK
    got = new.download()
    for g, old in zip(got, arrays):
        assert g.shape == old[keep].shape
        assert g.tobytes() == old[keep].tobytes()
    assert (got[0][:, 0] == np.nonzero(keep)[0]).all()  # (component 0 is the index: the survivors, in order)
    # a second removal, on the result: below one chunk
    m = new.size()
    idx2 = M.second_removal_indices_b(m)
    keep2 = np.ones(m, dtype=bool)
    keep2[idx2] = False
    newer = api.edit_remove_points(new, idx2)
    assert newer.size() == keep2.sum() and 0 < newer.size() < m
    for g, old in zip(newer.download(), arrays):
        assert g.tobytes() == old[keep][keep2].tobytes()
    for g, old in zip(cloud.download(), arrays):  # the input cloud is untouched
        assert g.tobytes() == old.tobytes()


# ---- scene C: region growing -------------------------------------------------------------------------------------------------------------------
def test_region_growing_over_more_than_256_seed_blocks(ctx):
    from glim_amd import api

    sc = M.scene_c()
    gpu = [api.clone_exact(p, ctx=ctx) for p in sc["clouds"]]
    prm = api.RegionGrowingParams(distance_threshold=M.THRESHOLD_C, dilation_radius=M.DILATION_C)
    want = R.region_grow(sc["clouds"], sc["poses"], M.CENTER, M.THRESHOLD_C, dilation_radius=M.DILATION_C)
    got = api.edit_region_grow(gpu, sc["poses"], M.CENTER, prm)
    print("candidates", got["num_candidates"], "cluster", got["count"], "rounds", got["rounds"], "seed", got["seed"])
    assert want["num_candidates"] > 65536 and want["seed"] == (0, sc["tie"][0])
    assert got["seed"] == (0, sc["tie"][0]) and got["seed_qq"] == M.TIE_QQ  # the lower index of the two tied candidates
    np.testing.assert_array_equal(got["pairs"], want["pairs"])
    np.testing.assert_array_equal(got["levels"], want["levels"])
    for k in ("count", "num_candidates", "seed", "seed_qq", "rounds", "status"):
        assert got[k] == want[k], k
    assert (got["pairs"][:, 0] == 0).all() and got["count"] == len(sc["clouds"][0])  # the second patch is excluded
    again = api.edit_region_grow(gpu, sc["poses"], M.CENTER, prm)
    assert again["pairs"].tobytes() == got["pairs"].tobytes() and again["levels"].tobytes() == got["levels"].tobytes()
