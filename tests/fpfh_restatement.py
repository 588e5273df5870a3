"""FP64 restatement in NumPy of the FPFH descriptor and of nearest-descriptor matching as include/glim_amd.h ("FPFH") states them, written from
that text and vectorised over all pairs.  tests/test_fpfh*.py check the device against this; nothing here touches the library.

Besides the values it returns how close every decision came to going the other way, so that a test can state the condition under which the
device -- whose FP64 features differ from NumPy's by ~1e-15 -- must take the same decisions:
  bin margin    distance of 11 * (normalised feature) to the nearest bin edge that separates two bins (edges 1..10; for f1, which is an angle,
                also the seam at -pi / +pi, i.e. edges 0 and 11)
  swap margin   | |a1| - |a2| | of the pairs whose two values are not identical (identical inputs give identical values on any machine)
  match gap     second-best minus best squared distance of every query"""
import numpy as np

FPFH_DIM = 33


def _sq3(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def neighbour_pairs(points32, radius, chunk=512):
    """(i, j, d2) of every ordered pair with 0 < d2 <= r^2, d2 = (dx^2 + dy^2) + dz^2 in FP64 from the FP32 coordinates (dp = p_j - p_i);
    rows with a non-finite coordinate take no part"""
    p = np.asarray(points32, dtype=np.float32).astype(np.float64)[:, :3]
    n = len(p)
    ok = np.all(np.isfinite(p), axis=1)
    r2 = float(radius) * float(radius)
    I, J, D = [], [], []
    for a in range(0, n, chunk):
        d = p[None, :, :] - p[a:a + chunk, None, :]
        with np.errstate(invalid="ignore"):
            d2 = _sq3(d)
            m = (d2 > 0.0) & (d2 <= r2) & ok[None, :] & ok[a:a + chunk, None]
        ii, jj = np.nonzero(m)
        I.append(ii + a)
        J.append(jj)
        D.append(d2[ii, jj])
    return np.concatenate(I), np.concatenate(J), np.concatenate(D)


def pair_features(points32, normals32, i, j, d2):
    """per pair: bins (m x 3, -1 in every column of a skipped pair), skipped (|v| = 0), bin margin (m x 3), swap margin (m; inf where a1 and a2
    are identical)"""
    p = np.asarray(points32, dtype=np.float32).astype(np.float64)[:, :3]
    nr = np.asarray(normals32, dtype=np.float32).astype(np.float64)[:, :3]
    dp = p[j] - p[i]
    ni, nj = nr[i], nr[j]
    f4 = np.sqrt(d2)
    a1 = np.sum(ni * dp, axis=1) / f4
    a2 = np.sum(nj * dp, axis=1) / f4
    swap = np.abs(a1) < np.abs(a2)
    n1 = np.where(swap[:, None], nj, ni)
    n2 = np.where(swap[:, None], ni, nj)
    dp = np.where(swap[:, None], -dp, dp)
    f3 = np.where(swap, -a2, a1)
    v = np.cross(dp, n1)
    vn = np.sqrt(np.sum(v * v, axis=1))
    skipped = vn == 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        v = v / vn[:, None]
    w = np.cross(n1, v)
    f2 = np.sum(v * n2, axis=1)
    f1 = np.arctan2(np.sum(w * n2, axis=1), np.sum(n1 * n2, axis=1))
    t = np.stack([11.0 * (f1 + np.pi) / (2.0 * np.pi), 11.0 * (f2 + 1.0) / 2.0, 11.0 * (f3 + 1.0) / 2.0], axis=1)
    t[skipped] = 5.5
    bins = np.clip(np.floor(t), 0, 10).astype(np.int64)
    # nearest deciding edge: 1..10 for every feature, 0 and 11 too for the angle
    inner = np.clip(np.round(t), 1, 10)
    margin = np.abs(t - inner)
    seam = np.minimum(np.abs(t[:, 0]), np.abs(t[:, 0] - 11.0))
    margin[:, 0] = np.minimum(margin[:, 0], seam)
    margin[skipped] = np.inf
    bins[skipped] = -1
    swap_margin = np.abs(np.abs(a1) - np.abs(a2))
    swap_margin[a1 == a2] = np.inf
    return bins, skipped, margin, swap_margin


def spfh(points32, normals32, radius):
    """S (n x 33, count * 100 / k), k (n), the pair list and the margins"""
    n = len(points32)
    i, j, d2 = neighbour_pairs(points32, radius)
    bins, skipped, margin, swap_margin = pair_features(points32, normals32, i, j, d2)
    k = np.bincount(i, minlength=n)
    counts = np.zeros((n, FPFH_DIM), dtype=np.int64)
    keep = ~skipped
    for f in range(3):
        np.add.at(counts, (i[keep], 11 * f + bins[keep, f]), 1)
    S = np.zeros((n, FPFH_DIM))
    nz = k > 0
    S[nz] = (counts[nz] * 100) / k[nz, None].astype(np.float64)
    return {"S": S, "k": k, "counts": counts, "i": i, "j": j, "d2": d2, "bins": bins, "skipped": skipped, "bin_margin": margin, "swap_margin": swap_margin}


def fpfh(points32, normals32, radius):
    """the descriptors in FP64 (n x 33, before the one rounding to FP32) plus everything spfh() returns"""
    r = spfh(points32, normals32, radius)
    n = len(points32)
    F = np.zeros((n, FPFH_DIM))
    np.add.at(F, r["i"], r["S"][r["j"]] * (1.0 / r["d2"])[:, None])
    for b in range(3):
        blk = F[:, 11 * b:11 * b + 11]
        s = blk.sum(axis=1)
        nz = s != 0.0
        blk[nz] *= (100.0 / s[nz])[:, None]
    r["F"] = F
    return r


def sqdist_matrix(source, target):
    a = np.asarray(source, dtype=np.float64)
    b = np.asarray(target, dtype=np.float64)
    d = a[:, None, :] - b[None, :, :]
    return np.sum(d * d, axis=2)


def match(target, source):
    """per source row: nearest target row (ties to the smaller index; -1 for an empty target), its squared distance, and the second best
    squared distance (inf when the target has one row)"""
    ns, nt = len(source), len(target)
    if nt == 0:
        return np.full(ns, -1, dtype=np.int64), np.full(ns, np.inf), np.full(ns, np.inf)
    D = sqdist_matrix(source, target)
    best = np.argmin(D, axis=1)  # first occurrence = smaller index
    rows = np.arange(ns)
    d1 = D[rows, best]
    D2 = D.copy()
    D2[rows, best] = np.inf
    d2 = D2.min(axis=1) if nt > 1 else np.full(ns, np.inf)
    return best, d1, d2


def match_reciprocal(target, source):
    """forward match with -1 where source i is not the nearest source of its target; also the backward (best, d1, d2) per target row"""
    best, d1, d2 = match(target, source)
    back, e1, e2 = match(source, target)
    keep = (best >= 0) & (back[np.clip(best, 0, None)] == np.arange(len(source))) if len(target) else np.zeros(len(source), dtype=bool)
    return np.where(keep, best, -1), (best, d1, d2), (back, e1, e2)


def fp32_bound(source, target_rows):
    """e = 36 * 2^-24 * (|a|^2 + |b|^2) per (source row, its given target row)"""
    a = np.asarray(source, dtype=np.float64)
    b = np.asarray(target_rows, dtype=np.float64)
    return 36.0 * 2.0 ** -24 * (np.sum(a * a, axis=1) + np.sum(b * b, axis=1))
