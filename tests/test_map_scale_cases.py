"""CPU checks of the map-scale scenes (tests/map_scale_cases.py): the properties that make tests/test_map_scale_gpu.py meaningful, so that nobody
can shrink the scenes unnoticed, and the restatements at these sizes -- NumPy only, no device."""
import time

import numpy as np
import pytest

import map_edit_restatement as R
import map_scale_cases as M
import plane_ba_restatement as B

_spent = {}


def _timed(name, fn, *a, **kw):
    t0 = time.perf_counter()
    out = fn(*a, **kw)
    _spent[name] = time.perf_counter() - t0
    print(f"{name}: {_spent[name]:.2f} s")
    assert _spent[name] < 20.0, name  # every restatement of a GPU check finishes well under a minute
    return out


@pytest.fixture(scope="module")
def scene_a():
    return _timed("scene A", M.scene_a)


@pytest.fixture(scope="module")
def grown_c():
    sc = _timed("scene C", M.scene_c)
    return sc, _timed("region growing on scene C", R.region_grow, sc["clouds"], sc["poses"], M.CENTER, M.THRESHOLD_C, dilation_radius=M.DILATION_C)


def _ids(pairs):
    return R.pack_ids(pairs)


def test_scene_a_is_just_past_one_scan_chunk_and_its_empty_sub_maps_sit_where_find_sub_can_trip(scene_a):
    sizes = scene_a["sizes"]
    assert sizes == [0, 1] + [65536] * 32 + [0, 0, 255] + [65536] * 32 + [4097, 0] and len(sizes) == 71
    assert scene_a["total"] == sum(sizes) == M.TOTAL_A == 4198657
    T = scene_a["total"] + 1  # the flag array of a selection
    tiles = (T + M.TILE - 1) // M.TILE
    assert tiles == 1026 and tiles > M.CHUNK_TILES and M.CHUNK == 4194304
    empty = [s for s, n in enumerate(sizes) if n == 0]
    assert empty == [0, 34, 35, 70]  # first, an adjacent pair in the middle, last
    assert [len(c) for c in scene_a["clouds"]] == sizes and len(scene_a["poses"]) == 71
    assert [s for s, e in enumerate(scene_a["exact"]) if e] == [36, 69] and sizes[36] == 255 and sizes[69] == 4097
    for s, c in enumerate(scene_a["clouds"]):  # the FP32 clouds hold FP32 values, the FP64 ones do not
        assert (c.astype(np.float32).astype(np.float64) == c).all() == (not scene_a["exact"][s] or len(c) == 0), s
    # the forced indices and their owners: the first point of all (behind an empty sub-map), both sides of a tile and of a chunk boundary, the last
    assert M.FORCED == (0, 4095, 4096, 4194303, 4194304, 4198656)
    assert scene_a["forced"].tolist() == [[1, 0], [2, 4094], [2, 4095], [68, 2096895 - 31 * 65536], [68, 2096896 - 31 * 65536], [69, 4096]]
    off = np.concatenate([[0], np.cumsum(sizes)])
    for i, (s, j) in zip(M.FORCED, scene_a["forced"]):
        assert off[s] + j == i and 0 <= j < sizes[s]
    # an index at the shared offset of the empty run belongs to the sub-map behind it
    assert M.owner(sizes, off[34]) == (36, 0) and M.owner(sizes, 0) == (1, 0)
    # the poses differ, with rotations of order 0.5 rad and translations of order 20 m
    t = np.array([np.linalg.norm(P[:3, 3]) for P in scene_a["poses"]])
    ang = np.array([np.arccos(np.clip((np.trace(P[:3, :3]) - 1) / 2, -1, 1)) for P in scene_a["poses"]])
    assert 10.0 < np.median(t) < 60.0 and 0.3 < np.median(ang) < 1.5 and len({P.tobytes() for P in scene_a["poses"]}) == 71


def test_every_predicate_selects_the_forced_points_and_a_proper_part_of_scene_a(scene_a):
    clouds, poses, total = scene_a["clouds"], scene_a["poses"], scene_a["total"]
    forced = _ids(scene_a["forced"])
    for name, (mode, _, args) in M.PREDICATES_A.items():
        want, _ = _timed("select " + name, R.select, clouds, M.matrices_a(mode, poses), *args)
        print(name, "selects", len(want), "of", total, f"({100.0 * len(want) / total:.2f} %)")
        assert 0 < len(want) < total
        assert 0.005 * total < len(want) < 0.12 * total  # "roughly 1 - 10 %"
        assert np.isin(forced, _ids(want)).all(), name
        assert len(set(want[:, 0].tolist())) == 67  # every non-empty sub-map contributes
    ball, _ = _timed("ball select", B.select, clouds, poses, M.CENTER, M.BALL_RADIUS)
    print("ball selects", len(ball), "of", total)
    assert 0.005 * total < len(ball) < 0.12 * total and np.isin(forced, _ids(ball)).all()
    mode, _, args = M.EVERYTHING
    every, _ = _timed("select everything", R.select, clouds, M.matrices_a(mode, poses), *args)
    assert len(every) == total
    np.testing.assert_array_equal(every, M.all_pairs(scene_a["sizes"]))
    assert not np.isin(every[:, 0], [0, 34, 35, 70]).any()
    mode, _, args = M.NOTHING
    none, _ = _timed("select nothing", R.select, clouds, M.matrices_a(mode, poses), *args)
    assert len(none) == 0


def test_scene_b_and_its_index_lists():
    n = M.N_B
    assert n == 4198657 and (n + 1 + M.TILE - 1) // M.TILE > M.CHUNK_TILES and n < 2**24
    idx = M.removal_indices_b()
    assert idx.dtype == np.int32 and idx.min() == 0 and idx.max() == n - 1
    have = set(idx.tolist())
    assert set(range(0, n, 3)) <= have and {0, 4095, 4096, M.CHUNK - 1, M.CHUNK, n - 1} <= have
    assert set(range(M.CHUNK - 2500, M.CHUNK + 2500)) <= have
    assert len(idx) > len(have) and (np.diff(idx) < 0).any()  # duplicates, and not ascending
    keep = np.ones(n, dtype=bool)
    keep[idx] = False
    kept = int(keep.sum())
    assert 0 < kept < M.CHUNK and kept + 1 > M.TILE  # the second removal runs below one chunk, on more than one tile
    idx2 = M.second_removal_indices_b(kept)
    assert idx2.min() == 0 and idx2.max() == kept - 1 and len(idx2) > len(set(idx2.tolist()))
    sc = M.scene_b()
    for k in ("points", "normals", "covs"):
        a = sc[k].reshape(n, -1)
        assert a.dtype == np.float32 and np.isfinite(a).all()
        assert (a[:, 0] == np.arange(n)).all()  # distinct per point, in every array
    assert (sc["covs"] == np.transpose(sc["covs"], (0, 2, 1))).all()
    out = _timed("removal", lambda: [R.remove(sc[k], idx) for k in ("points", "normals", "covs")])
    assert all(len(a) == kept for a in out)


def test_scene_c_has_more_than_256_seed_blocks_and_an_exact_tie_across_them(grown_c):
    sc, res = grown_c
    cand, w = R.select(sc["clouds"], sc["poses"], R.WINDOW, M.CENTER)
    m = len(cand)
    assert m == 70200 == sum(len(c) for c in sc["clouds"]) and m > 65536 and (m + 255) // 256 > 256
    a, b = sc["tie"]
    assert a // 256 == 0 and b // 256 == 256 and b // 256 % 256 == a // 256  # the same thread of the final kernel folds both blocks
    assert cand[a].tolist() == [0, 7] and cand[b].tolist() == [0, 65600]
    qq = R.center_qq(w, M.CENTER)
    assert qq[a].tobytes() == qq[b].tobytes() and qq[a] == M.TIE_QQ
    others = np.delete(qq, [a, b])
    assert others.min() > M.TIE_QQ
    # the lattice: spacing well below the threshold, the gap to the second patch wider than the threshold and the dilation radius
    assert M.SPACING_C * 2 < M.THRESHOLD_C
    gap = sc["clouds"][1][:, 0].min() - np.delete(sc["clouds"][0], [a, b], axis=0)[:, 0].max()
    assert gap > M.DILATION_C > M.THRESHOLD_C
    # the restatement: the seed is the lower of the two, the lattice is taken whole, the second patch not at all
    assert res["num_candidates"] == m and res["seed"] == (0, 7) and res["seed_qq"] == M.TIE_QQ
    assert res["count"] == len(sc["clouds"][0]) and (res["pairs"][:, 0] == 0).all()
    assert res["rounds"] > 40 and res["levels"][b] >= 1
    print("scene C: rounds", res["rounds"], "cluster", res["count"], "of", m)


def test_the_bucketed_neighbour_search_returns_the_pairs_of_the_distance_matrix():
    clouds, poses, normals = R.make_scene(fp32=True)
    cand, w = R.select(clouds, poses, R.WINDOW, R.CENTER)
    nw = np.concatenate([R.rotate(np.asarray(normals[s])[cand[cand[:, 0] == s, 1]], poses[s]) for s in range(len(clouds))]).reshape(-1, 3)
    cos10 = np.cos(np.deg2rad(10.0))
    for thr, n, c in ((0.15, None, None), (0.15, nw, cos10), (0.38, None, None), (1e-4, None, None), (3.0, None, None)):
        i, j = R.neighbor_edges(w, thr, n, c)
        di, dj = np.nonzero(R.adjacency(w, thr, n, c))
        np.testing.assert_array_equal(i, di)
        np.testing.assert_array_equal(j, dj)
        for seed, hops in ((0, 0), (len(w) // 2, 3)):
            np.testing.assert_array_equal(R.bfs_levels_edges(len(w), i, j, seed, hops), R.bfs_levels(R.adjacency(w, thr, n, c), seed, hops))
    # a lattice at exactly the threshold, and one place above it
    g = np.arange(4.0)
    p = np.array([20.0, -13.0, 3.0]) + np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    for thr in (1.0, np.nextafter(1.0, 2.0)):
        i, j = R.neighbor_edges(p, thr)
        di, dj = np.nonzero(R.adjacency(p, thr))
        np.testing.assert_array_equal(i, di)
        np.testing.assert_array_equal(j, dj)
