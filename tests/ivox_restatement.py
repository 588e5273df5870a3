"""FP64 restatement of the device iVox (include/glim_amd.h "device iVox") in NumPy / pure Python: the SEQUENTIAL insert of
gtsam_points::IncrementalVoxelMap<FlatContainer>, its LRU eviction, its bounded nearest-neighbour search, and the GICP / continuous-time
GICP factors over it.  tests/test_ivox.py checks the device against this; nothing here touches the library.

Storage is the library's documented choice: FP32 points and covariances; an insert with a pose forms x' = ((R00 x + R01 y) + R02 z) + tx in
FP64 with separate roundings, rounds to FP32, and the voxel / the min_dist test use the stored value."""
import numpy as np

from ct_restatement import hat

KEY_RANGE = 1048576.0  # voxel coordinates live in [-2^20, 2^20)

OFFSETS7 = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
OFFSETS19 = OFFSETS7 + [(1, 1, 0), (1, -1, 0), (-1, 1, 0), (-1, -1, 0), (1, 0, 1), (1, 0, -1), (-1, 0, 1), (-1, 0, -1), (0, 1, 1), (0, 1, -1), (0, -1, 1),
                        (0, -1, -1)]
OFFSETS27 = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
OFFSETS = {1: OFFSETS7[:1], 7: OFFSETS7, 19: OFFSETS19, 27: OFFSETS27}


def transform_points(p32, T):
    """stored points of insert(cloud, T): FP64 products and sums with separate roundings, then FP32"""
    p = np.asarray(p32, dtype=np.float32).astype(np.float64)
    if T is None:
        return np.asarray(p32, dtype=np.float32).copy()
    T = np.asarray(T, dtype=np.float64)
    out = np.empty_like(p)
    for r in range(3):
        out[:, r] = ((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3]
    return out.astype(np.float32)


def transform_covs(c32, T):
    """R C R^T with the FP32 image of R (the device sums in FP32, in another order: compared at 1e-6)"""
    c = np.asarray(c32, dtype=np.float32)
    if T is None:
        return c.copy()
    R = np.asarray(T, dtype=np.float64)[:3, :3].astype(np.float32).astype(np.float64)
    return np.einsum("ab,nbc,dc->nad", R, c.astype(np.float64), R).astype(np.float32)


def voxel_coords(p32, leaf):
    """floor(p * (1 / leaf)) in FP64 on the stored point; valid = finite and inside the key range"""
    t = np.asarray(p32, dtype=np.float32).astype(np.float64) * (1.0 / leaf)
    with np.errstate(invalid="ignore"):
        valid = np.all((t >= -KEY_RANGE) & (t < KEY_RANGE), axis=1)
    c = np.zeros(t.shape, dtype=np.int64)
    c[valid] = np.floor(t[valid]).astype(np.int64)
    return c, valid


def sqdist(a, b):
    """(dx^2 + dy^2) + dz^2 with separate roundings (sqdist_nc of gicp.hip); a: (3,), b: (m, 3)"""
    d = b - a
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


class Voxel:
    __slots__ = ("coord", "pts", "covs", "count", "lru")

    def __init__(self, coord, cap, lru):
        self.coord = coord
        self.pts = np.zeros((cap, 3), dtype=np.float32)
        self.covs = np.zeros((cap, 3, 3), dtype=np.float32)
        self.count = 0
        self.lru = lru


class IVox:
    """IncrementalVoxelMap<FlatContainer>(leaf) with upstream's defaults"""

    def __init__(self, leaf, min_dist=0.1, max_points=20, lru_horizon=10, lru_clear_cycle=10, mode=7):
        self.leaf = float(leaf)
        self.min_sq = float(min_dist) * float(min_dist)
        self.cap = int(max_points)
        self.lru_horizon, self.lru_clear_cycle, self.lru_counter = int(lru_horizon), int(lru_clear_cycle), 0
        self.mode = int(mode)
        self.voxels = []  # first-seen order
        self.index = {}   # coord -> position in self.voxels

    def insert(self, points32, covs32, T=None):
        p = transform_points(points32, T)
        c = transform_covs(covs32, T)
        coords, valid = voxel_coords(p, self.leaf)
        p64 = p.astype(np.float64)
        for i in range(len(p)):
            if not valid[i]:
                continue
            key = (int(coords[i, 0]), int(coords[i, 1]), int(coords[i, 2]))
            k = self.index.get(key)
            if k is None:
                k = len(self.voxels)
                self.index[key] = k
                self.voxels.append(Voxel(key, self.cap, self.lru_counter))
            v = self.voxels[k]
            v.lru = self.lru_counter
            # FlatContainer::add
            if v.count >= self.cap:
                continue
            if v.count and np.any(sqdist(p64[i], v.pts[: v.count].astype(np.float64)) < self.min_sq):
                continue
            v.pts[v.count] = p[i]
            v.covs[v.count] = c[i]
            v.count += 1
        self.lru_counter += 1
        if self.lru_counter % self.lru_clear_cycle == 0:
            self.voxels = [v for v in self.voxels if not (v.lru + self.lru_horizon < self.lru_counter)]
            self.index = {v.coord: k for k, v in enumerate(self.voxels)}
        return self

    # ---- views ----
    def num_voxels(self):
        return len(self.voxels)

    def num_points(self):
        return sum(v.count for v in self.voxels)

    def voxel_points(self):
        if not self.voxels:
            return np.zeros((0, 3))
        return np.concatenate([v.pts[: v.count] for v in self.voxels]).astype(np.float64)

    def as_dict(self):
        return {v.coord: v for v in self.voxels}

    # ---- search ----
    def nearest(self, q, max_d, detail=False):
        """(coord, place, d^2) of the nearest stored point among the voxels of the neighbour mode, or None.  detail: also the second-best
        distance over all candidates (inf when there is none), whatever the radius."""
        q = np.asarray(q, dtype=np.float64)
        t = q * (1.0 / self.leaf)
        best, best_d, second = None, np.inf, np.inf
        if np.all((t >= -KEY_RANGE) & (t < KEY_RANGE)):
            c = np.floor(t).astype(np.int64)
            for off in OFFSETS[self.mode]:
                k = self.index.get((int(c[0]) + off[0], int(c[1]) + off[1], int(c[2]) + off[2]))
                if k is None:
                    continue
                v = self.voxels[k]
                d = sqdist(q, v.pts[: v.count].astype(np.float64))
                for place in range(v.count):
                    if d[place] < best_d:  # a later candidate replaces the best only when strictly smaller
                        second = best_d
                        best, best_d = (v.coord, place), d[place]
                    elif d[place] < second:
                        second = d[place]
        hit = None if best is None or not (best_d <= max_d * max_d) else (best[0], best[1], best_d)
        return (hit, best_d, second) if detail else hit

    def face_distance(self, q):
        """distance of q to the nearest voxel face (a q this close to a face may fall into the other voxel under another rounding)"""
        t = np.asarray(q, dtype=np.float64) / self.leaf
        return float(np.min(np.abs(t - np.round(t))) * self.leaf)


def transform_q(T, p):
    T = np.asarray(T, dtype=np.float64)
    return np.asarray(p, dtype=np.float64) @ T[:3, :3].T + T[:3, 3]


def search_all(ivox, q, max_d):
    """per query: (coord, place) or None, plus the fragile set: queries whose best and second-best candidate distances differ by less than 1e-12
    relative, or that lie within 1e-9 of a voxel face"""
    hits, fragile = [], []
    for i in range(len(q)):
        hit, best_d, second = ivox.nearest(q[i], max_d, detail=True)
        hits.append(None if hit is None else (hit[0], hit[1]))
        close = np.isfinite(second) and (second - best_d) <= 1e-12 * max(second, 1e-300)
        if close or ivox.face_distance(q[i]) < 1e-9:
            fragile.append(i)
    return hits, fragile


def gicp_on_hits(ivox, hits, sp, sc, T):
    """IntegratedGICPFactor_<iVox, PointCloud>::linearize at T given the correspondences: per point M = (C_B + R C_A R^T)^-1, r = b - q,
    J_s = [R hat(p) | -R]; error = sum r^T M r (no 1/2), H_ss = sum J_s^T M J_s, b_s = sum J_s^T M r."""
    T = np.asarray(T, dtype=np.float64)
    R = T[:3, :3]
    vox = ivox.as_dict()
    out = dict(num_inliers=0, error=0.0, H_ss=np.zeros((6, 6)), b_s=np.zeros(6))
    q = transform_q(T, sp)
    for i, h in enumerate(hits):
        if h is None:
            continue
        v = vox[h[0]]
        b = v.pts[h[1]].astype(np.float64)
        CB = v.covs[h[1]].astype(np.float64)
        M = np.linalg.inv(CB + R @ sc[i] @ R.T)
        r = b - q[i]
        J = np.hstack([R @ hat(sp[i]), -R])
        out["num_inliers"] += 1
        out["error"] += r @ M @ r
        out["H_ss"] += J.T @ M @ J
        out["b_s"] += J.T @ M @ r
    return out


def ct_on_ivox(ivox, sp, sc, idx, poses, max_d):
    """IntegratedCT_GICPFactor_<iVox, PointCloud>::linearize: point i moves with T[idx[i]]; per bucket the rigid system above, then the chain
    rule [D0 | D1] (tests/ct_restatement.py np_ct_linearize, with the map's search in place of the exact one).  Returns the record, the hits and
    the fragile set."""
    T, D0, D1 = poses
    out = dict(num_inliers=0, error=0.0, H_00=np.zeros((6, 6)), H_01=np.zeros((6, 6)), H_11=np.zeros((6, 6)), b_0=np.zeros(6), b_1=np.zeros(6))
    hits, fragile = [None] * len(sp), []
    for k in range(len(T)):
        sel = np.flatnonzero(idx == k)
        if len(sel) == 0:
            continue
        h, fr = search_all(ivox, transform_q(T[k], sp[sel]), max_d)
        fragile += [int(sel[j]) for j in fr]
        for j, i in enumerate(sel):
            hits[i] = h[j]
        L = gicp_on_hits(ivox, h, sp[sel], sc[sel], T[k])
        out["num_inliers"] += L["num_inliers"]
        out["error"] += L["error"]
        out["H_00"] += D0[k].T @ L["H_ss"] @ D0[k]
        out["H_01"] += D0[k].T @ L["H_ss"] @ D1[k]
        out["H_11"] += D1[k].T @ L["H_ss"] @ D1[k]
        out["b_0"] += D0[k].T @ L["b_s"]
        out["b_1"] += D1[k].T @ L["b_s"]
    return out, hits, fragile
