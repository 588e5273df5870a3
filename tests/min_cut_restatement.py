"""NumPy restatement of the map editor's min-cut segmentation (include/glim_amd.h "Map editing", min-cut; device: glim_amd/csrc/map_edit.hip
and min_cut.hip): the scene of the tests, the candidate / neighbour / edge / capacity construction term by term in the documented order, a
plain restatement of the round-based push-relabel, and the judge -- scipy.sparse.csgraph.maximum_flow on the (n + 2)-node integer graph,
which nobody here wrote.

Every comparison of tests/test_min_cut_gpu.py with this file is an equality.  The conditions on a scene are `graph_margins`: no weight within
1e-6 of a quantisation step's middle, no point whose k-th and (k+1)-th neighbour distances are within 1e-5 relative (the device orders
neighbours in FP32), no qq within 1e-9 relative of a squared radius.
"""
import numpy as np

import map_edit_restatement as R
from glim_amd.se3 import se3_exp

CAP_SCALE = 65536.0  # GLIM_AMD_EDIT_CAP_SCALE
ROUNDS_PER_LOOK = 32  # GLIM_AMD_EDIT_ROUNDS_PER_LOOK
MAX_ROUNDS = 65536  # GLIM_AMD_EDIT_MIN_CUT_MAX_ROUNDS
INF = np.iinfo(np.int32).max
OK, EMPTY, FEW_POINTS, NO_SEED, ROUND_LIMIT = "ok", "empty", "few_points", "no_seed", "round_limit"

BASE = np.array([20.5, -13.25, 2.2])  # foot of the post
CENTER = BASE + np.array([0.0, 0.0, 0.8])  # the picked point: mid-height of the post
PARAMS = dict(distance_sigma=0.25, angle_sigma=float(np.deg2rad(10.0)), foreground_mask_radius=0.5, background_mask_radius=2.0, foreground_weight=10.0,
              background_weight=0.0, k_neighbors=8, use_normals=False, max_rounds=0)
DEFAULTS = dict(distance_sigma=0.25, angle_sigma=float(np.deg2rad(10.0)), foreground_mask_radius=0.5, background_mask_radius=5.0, foreground_weight=10.0,
                background_weight=0.0, k_neighbors=20, use_normals=False, max_rounds=0)


# ---- the scene ---------------------------------------------------------------------------------------------------------------------------------
def make_scene(seed=1, fp32=False):
    """A post of 500 points (radius 8 cm, 1.6 m high) on a jittered ground plane of 2 400 points (6.7 m square), dealt over S = 3 clouds with
    poses whose translations are of order 20 m.  Cloud 1 is an FP32 cloud (its points are rounded here, as clone() rounds them); fp32=True
    rounds all of them (the clouds with normals are FP32 clouds).  -> (clouds, poses, normals): normals are FP32 values in the clouds' frames,
    the ground's up and the post's radial direction, perturbed, with random signs."""
    rng = np.random.default_rng(seed)
    ground = np.stack([rng.uniform(-3.35, 3.35, 2400), rng.uniform(-3.35, 3.35, 2400), rng.normal(0.0, 0.01, 2400)], axis=1)
    phi, rad = rng.uniform(0.0, 2.0 * np.pi, 500), 0.08 * np.sqrt(rng.uniform(0.0, 1.0, 500))
    post = np.stack([rad * np.cos(phi), rad * np.sin(phi), rng.uniform(0.0, 1.6, 500)], axis=1)
    w = BASE + np.concatenate([ground, post])
    nw = np.concatenate([np.tile([0.0, 0.0, 1.0], (2400, 1)), np.stack([np.cos(phi), np.sin(phi), np.zeros(500)], axis=1)])
    nw = (nw + 0.05 * rng.normal(size=nw.shape)) * rng.choice([-1.0, 1.0], size=(len(nw), 1))
    nw /= np.linalg.norm(nw, axis=1, keepdims=True)
    owner = rng.integers(0, 3, len(w))
    poses = [se3_exp([0.3, -0.2, 0.5, 18.0, -22.0, 4.0]), se3_exp([-0.4, 0.1, 1.2, -21.0, 15.0, -3.0]), se3_exp([0.1, 0.2, 0.3, 19.0, 20.0, 1.0])]
    clouds, normals = [], []
    for s, T in enumerate(poses):
        p = (w[owner == s] - T[:3, 3]) @ T[:3, :3]
        if s == 1 or fp32:
            p = p.astype(np.float32).astype(np.float64)
        clouds.append(p.reshape(-1, 3))
        normals.append((nw[owner == s] @ T[:3, :3]).astype(np.float32).reshape(-1, 3))
    return clouds, poses, normals


# ---- the graph -----------------------------------------------------------------------------------------------------------------------------------
def quantize(w):
    """(int32) floor(w * 65536 + 0.5)"""
    return np.floor(np.asarray(w, dtype=np.float64) * CAP_SCALE + 0.5).astype(np.int64)


def edge_weight(a, b, sigma_d, na=None, nb=None, sigma_a=None):
    """w = exp(-(dd / (sigma_d sigma_d))) [* exp(-((t t) / (sigma_a sigma_a))), t = acos(min(1, |n_i . n_j|))], every product and sum on its own"""
    dx, dy, dz = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1], a[:, 2] - b[:, 2]
    dd = (dx * dx + dy * dy) + dz * dz
    w = np.exp(-(dd / (np.float64(sigma_d) * np.float64(sigma_d))))
    if na is not None:
        d = np.abs((na[:, 0] * nb[:, 0] + na[:, 1] * nb[:, 1]) + na[:, 2] * nb[:, 2])
        t = np.arccos(np.minimum(1.0, d))
        w = w * np.exp(-((t * t) / (np.float64(sigma_a) * np.float64(sigma_a))))
    return w


def neighbours(w, k):
    """-> (n x k indices of the k nearest OTHER points, the smallest relative gap between a point's k-th and (k+1)-th neighbour distance):
    the K = k + 1 nearest with the query included, the query's own index dropped"""
    dx, dy, dz = (w[:, None, a] - w[None, :, a] for a in range(3))
    D = (dx * dx + dy * dy) + dz * dz
    np.fill_diagonal(D, -1.0)  # the query sorts first
    order = np.argsort(D, axis=1, kind="stable")
    assert (order[:, 0] == np.arange(len(w))).all()
    dk = np.sqrt(np.take_along_axis(D, order[:, k:k + 2], axis=1)) if len(w) > k + 1 else None
    gap = float(((dk[:, 1] - dk[:, 0]) / dk[:, 1]).min()) if dk is not None else np.inf
    return order[:, 1:k + 1], gap


def graph(clouds, poses, center, params=PARAMS, normals=None, resolution=R.RESOLUTION, window=R.WINDOW_CELLS):
    """-> {status, candidates, world, qq, edges (E x 2, i < j, ascending key), cap, src, snk, num_foreground, num_background, margins}"""
    p = dict(params)
    k = int(p["k_neighbors"])
    fg, bg = np.float64(p["foreground_mask_radius"]), np.float64(p["background_mask_radius"])
    ball = bg + np.float64(1.0)
    cand, w = R.select(clouds, poses, R.WINDOW_BALL, center, ball, resolution, window)
    m = len(cand)
    out = {"candidates": cand, "world": w, "num_candidates": m, "num_edges": 0, "num_foreground": 0, "num_background": 0}
    if m < k + 1:
        out["status"] = EMPTY if m == 0 else FEW_POINTS
        return out
    qq = R.center_qq(w, center)
    nb, gap = neighbours(w, k)
    i = np.repeat(np.arange(m), k)
    j = nb.reshape(-1)
    keys = np.unique((np.minimum(i, j).astype(np.uint64) << np.uint64(32)) | np.maximum(i, j).astype(np.uint64))  # sorted, duplicates merged
    edges = np.stack([(keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)], axis=1)
    nw = None
    if p.get("use_normals"):
        nw = np.concatenate([R.rotate(np.asarray(normals[s])[cand[cand[:, 0] == s, 1]], poses[s]) for s in range(len(clouds))]).reshape(-1, 3)
    wgt = edge_weight(w[edges[:, 0]], w[edges[:, 1]], p["distance_sigma"], None if nw is None else nw[edges[:, 0]], None if nw is None else nw[edges[:, 1]],
                      p["angle_sigma"])
    bw = p["background_weight"] if p["background_weight"] > 0.0 else p["foreground_weight"]
    is_fg, is_bg = qq < fg * fg, qq >= bg * bg
    src = np.where(is_fg, quantize(p["foreground_weight"]), 0).astype(np.int64)
    snk = np.where(is_bg, quantize(bw), 0).astype(np.int64)
    frac = wgt * CAP_SCALE - np.floor(wgt * CAP_SCALE)
    radii2 = np.array([fg * fg, bg * bg, ball * ball])
    out.update(status=OK if is_fg.any() else NO_SEED, qq=qq, edges=edges, cap=quantize(wgt), src=src, snk=snk, num_edges=len(edges),
               num_foreground=int(is_fg.sum()), num_background=int(is_bg.sum()),
               margins={"weight": float(np.abs(frac - 0.5).min()), "neighbour_gap": gap,
                        "qq": float((np.abs(qq[:, None] - radii2[None, :]) / radii2[None, :]).min())})
    return out


def graph_margins_hold(margins):
    return margins["weight"] > 1e-6 and margins["neighbour_gap"] > 1e-5 and margins["qq"] > 1e-9


# ---- the solver, restated ----------------------------------------------------------------------------------------------------------------------
def solve(n, edges, cap, src, snk, max_rounds=0):
    """The device's round-based push-relabel from the sink side (min_cut.hip), round for round.  -> {flags, flow, rounds, looks, status}"""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    cap, src, snk = (np.asarray(a, dtype=np.int64) for a in (cap, src, snk))
    limit = max_rounds if max_rounds > 0 else MAX_ROUNDS
    E = len(edges)
    A = 2 * E
    tail = np.empty(A, dtype=np.int64)
    head = np.empty(A, dtype=np.int64)
    tail[0::2], head[0::2], tail[1::2], head[1::2] = edges[:, 0], edges[:, 1], edges[:, 1], edges[:, 0]
    order = np.argsort(tail, kind="stable")  # slot -> arc: by tail, then by arc id
    pos = np.empty(A, dtype=np.int64)
    pos[order] = np.arange(A)
    nbr = np.concatenate([head[order], [0]])
    rev = pos[order ^ 1] if A else np.zeros(0, dtype=np.int64)
    res = np.concatenate([cap[order >> 1], [0]])  # slot A: a dummy without residual, for the padding
    rs = np.searchsorted(tail[order], np.arange(n), side="left")
    deg = np.searchsorted(tail[order], np.arange(n), side="right") - rs
    D = int(deg.max()) if n and A else 0
    t = np.arange(max(D, 1))[None, :]
    idx = np.where(t < deg[:, None], rs[:, None] + t, A)  # n x D slots
    t0 = np.minimum(src, snk)
    ex, ab = snk - t0, src - t0

    def relabel():
        h = np.where(ab > 0, 1, INF).astype(np.int64)
        rho = 2
        while True:
            hit = (h == INF) & ((res[idx] > 0) & (h[nbr[idx]] < rho)).any(axis=1)
            if not hit.any():
                return h
            h[hit] = rho
            rho += 1

    h = relabel()
    rounds = looks = 0
    while ((ex > 0) & (h < INF)).any() and rounds < limit:
        chunk = min(ROUNDS_PER_LOOK, limit - rounds)
        for _ in range(chunk):
            act = (ex > 0) & (h < INF)
            if not act.any():
                break  # the device's idle rounds return at once
            a = np.where(act, np.minimum(ex, ab), 0)
            ex, ab = ex - a, ab - a
            need = act & (ex > 0)
            H = np.where(res[idx] > 0, h[nbr[idx]], INF)
            smin = H.argmin(axis=1)  # the first slot of the lowest height
            hmin = H[np.arange(n), smin]
            none = hmin == INF
            push = need & ~none & (h > hmin)
            hn = h.copy()
            hn[need & none] = INF
            up = need & ~none & ~(h > hmin)
            hn[up] = hmin[up] + 1
            ps = idx[np.arange(n), smin][push]
            pa = np.minimum(ex[push], res[ps])
            res[ps] -= pa
            ex[push] -= pa
            np.add.at(res, rev[ps], pa)
            np.add.at(ex, nbr[ps], pa)
            h = hn
        rounds += chunk
        looks += 1
        h = relabel()
    assert (res[:A] >= 0).all() and (res[:A] + res[:A][rev] == 2 * cap[order >> 1]).all()
    if ((ex > 0) & (h < INF)).any():
        return {"flags": np.zeros(n, dtype=np.int32), "flow": 0, "rounds": rounds, "looks": looks, "status": ROUND_LIMIT}
    return {"flags": (h < INF).astype(np.int32), "flow": int((src - ab).sum()), "rounds": rounds, "looks": looks, "status": OK}


# ---- the judge -----------------------------------------------------------------------------------------------------------------------------------
def _reach(start, mat):
    from scipy.sparse.csgraph import breadth_first_order

    return breadth_first_order(mat, start, directed=True, return_predecessors=False)


def judge(n, edges, cap, src, snk, maximal=False, times=None):
    """scipy's maximum flow on the (n + 2)-node graph (source n, sink n + 1) -> (flow, flags): the nodes reachable from the source over
    positive residuals -- the minimal source side of a minimum cut; maximal=True: the nodes that do NOT reach the sink (the maximal one).
    times: a dict that receives the seconds spent inside maximum_flow itself."""
    import time

    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import maximum_flow

    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    cap, src, snk = (np.asarray(a, dtype=np.int64) for a in (cap, src, snk))
    S, T = n, n + 1
    v = np.arange(n)
    rows = np.concatenate([edges[:, 0], edges[:, 1], np.full(n, S), v])
    cols = np.concatenate([edges[:, 1], edges[:, 0], v, np.full(n, T)])
    vals = np.concatenate([cap, cap, src, snk])
    C = coo_matrix((vals, (rows, cols)), shape=(n + 2, n + 2)).tocsr().astype(np.int32)  # parallel edges add up
    C.eliminate_zeros()
    t0 = time.perf_counter()
    r = maximum_flow(C, S, T)
    if times is not None:
        times["maximum_flow_s"] = time.perf_counter() - t0
    F = r.flow if hasattr(r, "flow") else C - r.residual
    resid = (C - F).tocsr()  # c(u, v) - f(u, v); f is antisymmetric, so a reverse arc without capacity has residual f(v, u)
    resid.data[resid.data < 0] = 0
    resid.eliminate_zeros()
    flags = np.zeros(n + 2, dtype=np.int32)
    if maximal:
        flags[:] = 1
        flags[_reach(T, resid.T.tocsr())] = 0
    else:
        flags[_reach(S, resid)] = 1
    return int(r.flow_value), flags[:n]


# ---- the whole call ------------------------------------------------------------------------------------------------------------------------------
def min_cut(clouds, poses, center, params=PARAMS, normals=None, resolution=R.RESOLUTION, window=R.WINDOW_CELLS):
    """-> {pairs, count, num_candidates, num_edges, num_foreground, num_background, flow, rounds, looks, status, graph}"""
    g = graph(clouds, poses, center, params, normals, resolution, window)
    out = {"pairs": np.zeros((0, 2), dtype=np.int32), "count": 0, "flow": 0, "rounds": 0, "looks": 0, "status": g["status"], "graph": g}
    for key in ("num_candidates", "num_edges", "num_foreground", "num_background"):
        out[key] = g[key]
    if g["status"] != OK:
        return out
    s = solve(g["num_candidates"], g["edges"], g["cap"], g["src"], g["snk"], int(dict(params)["max_rounds"]))
    out.update(flow=s["flow"], rounds=s["rounds"], looks=s["looks"], status=s["status"])
    if s["status"] == OK:
        out["pairs"] = g["candidates"][s["flags"] == 1]
        out["count"] = int(s["flags"].sum())
    return out


# ---- the tiny graphs of the solver's tests -------------------------------------------------------------------------------------------------------
def _g(n, edges, cap, src, snk):
    s, t = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    for v, c in src.items():
        s[v] = c
    for v, c in snk.items():
        t[v] = c
    return n, np.array(edges, dtype=np.int32).reshape(-1, 2), np.array(cap, dtype=np.int32), s, t


def grid_graph(seed, side=8):
    """a side x side 4-neighbour grid with capacities 0...3, 4 source and 6 sink nodes (distinct), tied with 3"""
    rng = np.random.default_rng(seed)
    node = np.arange(side * side).reshape(side, side)
    edges = np.concatenate([np.stack([node[:, :-1].ravel(), node[:, 1:].ravel()], axis=1), np.stack([node[:-1, :].ravel(), node[1:, :].ravel()], axis=1)])
    cap = rng.integers(0, 4, len(edges))
    ends = rng.choice(side * side, 10, replace=False)
    return _g(side * side, edges, cap, {int(v): 3 for v in ends[:4]}, {int(v): 3 for v in ends[4:]})


def long_chain():
    """2 x 32 + 5 nodes in a row, the source at one end and the sink at the other, the bottleneck in the middle"""
    n = 2 * ROUNDS_PER_LOOK + 5
    cap = np.full(n - 1, 9)
    cap[n // 2] = 4
    return _g(n, [(i, i + 1) for i in range(n - 1)], cap, {0: 20}, {n - 1: 20})


def tiny_graphs():
    """name -> (n, edges, cap, src, snk)"""
    out = {
        "one node, both terminals, source larger": _g(1, [], [], {0: 7}, {0: 3}),
        "one node, both terminals, sink larger": _g(1, [], [], {0: 3}, {0: 7}),
        "chain s-5-a-5-b-5-t, all saturated": _g(2, [(0, 1)], [5], {0: 5}, {1: 5}),
        "two parallel paths, different bottlenecks": _g(4, [(0, 1), (2, 3)], [2, 9], {0: 6, 2: 6}, {1: 6, 3: 6}),
        "a greedy path must be undone": _g(4, [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)], [4, 4, 4, 4, 4], {0: 8}, {3: 8}),
        "the diamond with a cross arc": _g(4, [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)], [3, 2, 5, 2, 3], {0: 9}, {3: 9}),
        "two components, one touches the sink": _g(5, [(0, 1), (1, 2), (3, 4)], [3, 1, 2], {0: 4, 3: 4}, {2: 4}),
        "edges of capacity 0": _g(4, [(0, 1), (1, 2), (2, 3), (0, 3)], [0, 5, 0, 2], {0: 6}, {3: 6, 2: 1}),
        "an isolated source node": _g(3, [(1, 2)], [3], {0: 5, 1: 2}, {2: 9}),
        "the long chain": long_chain(),
    }
    for seed in range(1, 7):
        out[f"8 x 8 grid, seed {seed}"] = grid_graph(seed)
    return out
