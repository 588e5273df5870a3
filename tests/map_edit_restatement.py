"""NumPy (FP64) restatement of the map editor's device side (include/glim_amd.h "Map editing"; reference:
src/glim/viewer/editor/points_selector.cpp): the four selection predicates in the device's documented operation order -- every product and
sum written out term by term, so that each boolean is reproduced bit for bit --, the outlier rule over oracle.find_inliers, region growing as
a breadth-first search over the edge list of a grid-bucketed neighbour search (`neighbor_edges`: the same ordered pairs as the brute-force distance
matrix `adjacency`, which tests/test_map_scale_cases.py holds it against, without the m x m memory), and removal as boolean indexing.

All comparisons of tests/test_map_edit_gpu.py with this file are equalities.  The one condition on a scene is the outlier test's: the device
adds the mean neighbour distances d_i in block order and the oracle adds them sequentially, so the two thresholds may differ in their last
places; `outlier_margin` returns the smallest |d_i - threshold| / threshold of a scene and the test requires it to exceed 1e-9 before it
compares anything.
"""
import numpy as np

from glim_amd.se3 import se3_exp

BOX, SPHERE, WINDOW, WINDOW_BALL = 0, 1, 2, 3
CENTER = np.array([20.5, -13.25, 3.0])
RESOLUTION, WINDOW_CELLS = 2.0, 5  # points_selector.cpp:22-23


# ---- predicates ------------------------------------------------------------------------------------------------------------------------------
def transform(points, M):
    """v_k = ((M_k0 p_x + M_k1 p_y) + M_k2 p_z) + M_k3"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    M = np.asarray(M, dtype=np.float64)
    v = np.empty_like(p)
    for k in range(3):
        v[:, k] = ((M[k, 0] * p[:, 0] + M[k, 1] * p[:, 1]) + M[k, 2] * p[:, 2]) + M[k, 3]
    return v


def rotate(normals, M):
    n = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    M = np.asarray(M, dtype=np.float64)
    v = np.empty_like(n)
    for k in range(3):
        v[:, k] = (M[k, 0] * n[:, 0] + M[k, 1] * n[:, 1]) + M[k, 2] * n[:, 2]
    return v


def sq3(v):
    return (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]


def center_qq(v, center):
    c = np.asarray(center, dtype=np.float64)
    e = np.stack([v[:, 0] - c[0], v[:, 1] - c[1], v[:, 2] - c[2]], axis=1)
    return sq3(e)


def in_window(v, center, resolution=RESOLUTION, window=WINDOW_CELLS):
    """cell = floor(v_k * (1 / resolution)) -- a product, :177 --; centre cell = floor(c_k / resolution) -- a division, :87"""
    inv = np.float64(1.0) / np.float64(resolution)
    keep = np.ones(len(v), dtype=bool)
    for k in range(3):
        cell = np.floor(v[:, k] * inv)
        c = np.floor(np.float64(center[k]) / np.float64(resolution))
        keep &= (cell >= c - window) & (cell <= c + window)
    return keep


def predicate(mode, v, center=None, radius=0.0, resolution=RESOLUTION, window=WINDOW_CELLS):
    if mode == BOX:
        return (v[:, 0] > -0.5) & (v[:, 0] < 0.5) & (v[:, 1] > -0.5) & (v[:, 1] < 0.5) & (v[:, 2] > -0.5) & (v[:, 2] < 0.5)
    if mode == SPHERE:
        return sq3(v) < 1.0
    keep = in_window(v, center, resolution, window)
    if mode == WINDOW_BALL:
        keep &= center_qq(v, center) < np.float64(radius) * np.float64(radius)
    return keep


def select(clouds, matrices, mode, center=None, radius=0.0, resolution=RESOLUTION, window=WINDOW_CELLS):
    """-> (pairs n x 2 int32 ascending in (sub-map, point), the n transformed points).  matrices: T_local_submap for BOX / SPHERE,
    T_world_submap otherwise."""
    pairs, vs = [np.zeros((0, 2), dtype=np.int64)], [np.zeros((0, 3))]
    for s, (p, M) in enumerate(zip(clouds, matrices)):
        v = transform(p, M)
        idx = np.nonzero(predicate(mode, v, center, radius, resolution, window))[0]
        pairs.append(np.stack([np.full(len(idx), s), idx], axis=1))
        vs.append(v[idx])
    return np.concatenate(pairs).astype(np.int32).reshape(-1, 2), np.concatenate(vs).reshape(-1, 3)


# ---- outliers in a radius (:703-759) -----------------------------------------------------------------------------------------------------------
def outlier_statistic(w, k):
    """d_i = mean distance of point i to its k nearest neighbours, itself included (brute force)"""
    dx, dy, dz = (w[:, None, a] - w[None, :, a] for a in range(3))
    D = np.sqrt((dx * dx + dy * dy) + dz * dz)
    return np.sort(D, axis=1)[:, :k].sum(axis=1) / k


def outlier_margin(w, k, thresh):
    """smallest |d_i - threshold| / threshold: how far the scene is from a decision that the order of a sum could turn"""
    d = outlier_statistic(w, k)
    mean = d.mean()
    var = (d * d).mean() - mean * mean
    t = mean + thresh * np.sqrt(max(var, 0.0))
    return np.abs(d - t).min() / t


def select_outliers(orc, clouds, poses, center, radius, radius_offset=1.0, k=10, thresh=2.0, resolution=RESOLUTION, window=WINDOW_CELLS):
    """-> (pairs, status, the candidates' world points)"""
    pairs, w = select(clouds, poses, WINDOW_BALL, center, np.float64(radius) + np.float64(radius_offset), resolution, window)
    if len(pairs) < k:
        return np.zeros((0, 2), dtype=np.int32), "few_points", w
    outlier = np.ones(len(pairs), dtype=bool)
    outlier[orc.find_inliers(w, k, thresh)] = False
    keep = outlier & (center_qq(w, center) < np.float64(radius) * np.float64(radius))
    return pairs[keep], "ok", w


# ---- region growing ------------------------------------------------------------------------------------------------------------------------------
def adjacency(w, distance_threshold, normals=None, cos_angle=None):
    dx, dy, dz = (w[:, None, a] - w[None, :, a] for a in range(3))
    adj = ((dx * dx + dy * dy) + dz * dz) < np.float64(distance_threshold) * np.float64(distance_threshold)
    if normals is not None:
        n = normals
        dot = (n[:, None, 0] * n[None, :, 0] + n[:, None, 1] * n[None, :, 1]) + n[:, None, 2] * n[None, :, 2]
        adj &= np.abs(dot) >= cos_angle
    return adj


def bfs_levels(adj, seed, max_hops=0):
    """hop count from the seed over the boolean adjacency matrix; -1 where unreached (or beyond max_hops)"""
    level = np.full(len(adj), -1, dtype=np.int32)
    level[seed] = 0
    rho = 0
    while max_hops == 0 or rho < max_hops:
        frontier = level == rho
        new = (level < 0) & adj[:, frontier].any(axis=1)
        if not new.any():
            break
        rho += 1
        level[new] = rho
    return level


def neighbor_edges(w, distance_threshold, normals=None, cos_angle=None):
    """np.nonzero(adjacency(...)) without the m x m matrix: -> (i, j), every ordered pair with an edge (i == j included), ascending in (i, j).
    The points are bucketed into cells a hair wider than the threshold, so that two points closer than it lie in the same or in adjacent
    cells; the pairs of the 27 cell neighbourhoods are then tested with adjacency's own expressions, term by term."""
    w = np.asarray(w, dtype=np.float64).reshape(-1, 3)
    m = len(w)
    if m == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    h = np.float64(distance_threshold) * 1.001
    cell = np.floor((w - w.min(axis=0)) / h).astype(np.int64) + 1  # >= 1: a neighbour's coordinate is never negative
    dim = cell.max(axis=0) + 2
    key = (cell[:, 2] * dim[1] + cell[:, 1]) * dim[0] + cell[:, 0]
    order = np.argsort(key, kind="stable")
    skey = key[order]
    thr2 = np.float64(distance_threshold) * np.float64(distance_threshold)
    src, dst = [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                nk = key + (dz * dim[1] + dy) * dim[0] + dx
                lo, hi = np.searchsorted(skey, nk, side="left"), np.searchsorted(skey, nk, side="right")
                cnt = hi - lo
                i = np.repeat(np.arange(m), cnt)
                j = order[np.repeat(lo, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))]
                ex, ey, ez = (w[i, a] - w[j, a] for a in range(3))
                keep = ((ex * ex + ey * ey) + ez * ez) < thr2
                if normals is not None:
                    n = normals
                    dot = (n[i, 0] * n[j, 0] + n[i, 1] * n[j, 1]) + n[i, 2] * n[j, 2]
                    keep &= np.abs(dot) >= cos_angle
                src.append(i[keep])
                dst.append(j[keep])
    src, dst = np.concatenate(src), np.concatenate(dst)
    o = np.lexsort((dst, src))
    return src[o], dst[o]


def bfs_levels_edges(m, src, dst, seed, max_hops=0):
    """bfs_levels over the edge list of neighbor_edges"""
    level = np.full(m, -1, dtype=np.int32)
    level[seed] = 0
    rho = 0
    while max_hops == 0 or rho < max_hops:
        hit = np.zeros(m, dtype=bool)
        hit[src[level[dst] == rho]] = True
        new = (level < 0) & hit
        if not new.any():
            break
        rho += 1
        level[new] = rho
    return level


def region_grow(clouds, poses, center, distance_threshold=0.5, cos_angle=None, normals=None, dilation_radius=0.5, max_hops=0, resolution=RESOLUTION,
                window=WINDOW_CELLS):
    """normals: None, or one N x 3 array per cloud (cloud-local; rotated to world here).  -> {pairs, levels, count, num_candidates, seed,
    seed_qq, rounds, status}"""
    cand, w = select(clouds, poses, WINDOW, center, 0.0, resolution, window)
    m = len(cand)
    if m == 0:
        return {"pairs": cand, "levels": np.zeros(0, dtype=np.int32), "count": 0, "num_candidates": 0, "seed": (-1, -1), "seed_qq": 0.0, "rounds": 0,
                "status": "empty"}
    nw = None
    if normals is not None:
        nw = np.concatenate([rotate(np.asarray(normals[s])[cand[cand[:, 0] == s, 1]], poses[s]) for s in range(len(clouds))]).reshape(-1, 3)
    qq = center_qq(w, center)
    seed = int(np.lexsort((np.arange(m), qq))[0])  # the smallest qq, ties to the smaller pair
    level = bfs_levels_edges(m, *neighbor_edges(w, distance_threshold, nw, cos_angle), seed, max_hops)
    rounds = int(level.max())
    if dilation_radius > 0.0:
        i, j = neighbor_edges(w, dilation_radius)
        near = np.zeros(m, dtype=bool)
        near[i[level[j] >= 0]] = True
        level[(level < 0) & near] = rounds + 1
    keep = level >= 0
    return {"pairs": cand[keep], "levels": level[keep], "count": int(keep.sum()), "num_candidates": m, "seed": (int(cand[seed, 0]), int(cand[seed, 1])),
            "seed_qq": float(qq[seed]), "rounds": rounds, "status": "ok", "all_levels": level, "candidates": cand, "world": w}


# ---- removal ---------------------------------------------------------------------------------------------------------------------------------------
def remove(array, indices):
    keep = np.ones(len(array), dtype=bool)
    keep[np.asarray(indices, dtype=np.int64)] = False
    return array[keep]


def pack_ids(pairs):
    """the reference's point ids (:84): (sub-map << 32) | point"""
    p = np.asarray(pairs, dtype=np.uint64).reshape(-1, 2)
    return (p[:, 0] << np.uint64(32)) | p[:, 1]


# ---- the scene of the tests ----------------------------------------------------------------------------------------------------------------------
def make_scene(seed=11, fp32=False):
    """S = 4 clouds of 1, 257, 1000 and 0 points (a single point, a block boundary, more than one block, an empty cloud) from a 2 cm slab
    through CENTER plus clutter, poses with translations of order 20 m.  Cloud 2 is an FP32 cloud (its points are rounded here, as clone()
    rounds them), the others keep FP64 points; fp32=True rounds all of them (the clouds with normals are FP32 clouds).
    -> (clouds, poses, normals): normals are FP32 values, the slab's normal tilted by some degrees (more than 10 for a part), random signs."""
    rng = np.random.default_rng(seed)
    n = np.array([0.3, -0.2, 0.93])
    n /= np.linalg.norm(n)
    e1 = np.cross(n, [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(n, e1)
    sizes = [1, 257, 1000, 0]
    poses = [se3_exp([0.3, -0.2, 0.5, 18.0, -22.0, 4.0]), np.eye(4), se3_exp([-0.4, 0.1, 1.2, -21.0, 15.0, -3.0]), se3_exp([0.1, 0.2, 0.3, 19.0, 20.0, 1.0])]
    clouds, normals = [], []
    for s, (k, T) in enumerate(zip(sizes, poses)):
        ab = rng.uniform(-1.3, 1.3, size=(k, 2))
        z = rng.uniform(-0.01, 0.01, size=k)
        w = CENTER + ab[:, :1] * e1 + ab[:, 1:] * e2 + z[:, None] * n
        clutter = rng.random(k) < 0.1
        w[clutter] = CENTER + rng.uniform(-1.3, 1.3, size=(int(clutter.sum()), 3))
        if s == 0:
            w = CENTER + np.array([[0.25, 0.125, 0.0]])
        p = (w - T[:3, 3]) @ T[:3, :3]
        if s == 2 or fp32:
            p = p.astype(np.float32).astype(np.float64)
        clouds.append(p.reshape(-1, 3))
        nl = (n + 0.08 * rng.normal(size=(k, 3))) * rng.choice([-1.0, 1.0], size=(k, 1))
        nl /= np.linalg.norm(nl, axis=1, keepdims=True)
        normals.append((nl @ T[:3, :3]).astype(np.float32).reshape(-1, 3))
    return clouds, poses, normals


MODEL = np.array([[1.6, 0.3, 0.0, 20.4], [-0.2, 1.9, 0.1, -13.0], [0.0, -0.1, 1.2, 3.1], [0.0, 0.0, 0.0, 1.0]])  # a gizmo: scale, shear, offset
