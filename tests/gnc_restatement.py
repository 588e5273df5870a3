"""FP64 restatement in NumPy of the GNC global registration as include/glim_amd.h ("GNC") states it, independent in method: the same integer
draws, the weighted pose by SVD (Kabsch) instead of Horn's quaternion + Jacobi, the occupancy as a Python set (ransac_restatement's).
tests/test_gnc*.py check the library against this; nothing here touches the library.

Gates of ONE step (they follow from the arithmetic; n = list length, GATE_C = 64 and EPS = 2^-52 are ransac_restatement's): a sum of n FP64
terms is off by at most n * 2^-53 * sum |term| in any order, so Horn's matrix N(H) moves by at most ~ n * EPS * S, S = sum w |p| |q|, and by
Davis-Kahan its leading eigenvector -- the rotation -- by at most that over gap = lambda_1 - lambda_2:
  rotation      GATE_C * n * EPS * S / gap                                       [rad]
  translation   that angle * max |p| + GATE_C * n * EPS * max |q|
  W             GATE_C * n * EPS * W                                             (all terms are >= 0: the sum itself)
  cost          GATE_C * n * EPS * (cost + 2 sum w sum_axis |d| m),  m = |t| + |R| |s| + |t0| per axis
                (the terms w r^2 are >= 0 too; the second part is the first-order term of the residual's own rounding: d = t - (R s + t0) is a
                sum of five terms of size m per axis, so it is off by ~ EPS m and r^2 by 2 |d| EPS m -- negligible where outliers dominate the
                cost, the whole error where the pose fits and d is micrometres between coordinates of metres)
For dof 4 the rotation is the direction of (C, S_yaw), which moves by at most |delta (C, S_yaw)| / |(C, S_yaw)|: gap = |(C, S_yaw)| there.
The comparison is conditional on S / gap <= 100 at every step (a condition on the input, asserted on this module's numbers)."""
import numpy as np

import ransac_restatement as R

GATE_C = R.GATE_C
EPS = R.EPS
LANES = 512      # the solve block: lane l takes the entries l, l + 512, ..
MAX_TRIALS = 1 << 22


def hashes(seed, index):
    """ransac_restatement.sample_hash over an array of indices (uint64 arithmetic wraps as the device's does)"""
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & R.MASK) + (np.asarray(index, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _f64(p32):
    return np.asarray(p32, dtype=np.float32).astype(np.float64)[:, :3]


def select(target32, source32, nearest, seed, max_init_samples):
    """step 1: the list as an (C, 2) array of (source index, target index), ascending in the source index"""
    sp, tp, near = _f64(source32), _f64(target32), np.asarray(nearest, dtype=np.int64)
    n = len(sp)
    if n == 0:
        return np.zeros((0, 2), dtype=np.int32)
    if max_init_samples >= n:
        cand = np.arange(n)
    else:
        cand = np.unique((hashes(seed, np.arange(max_init_samples)) % np.uint64(n)).astype(np.int64))
    cand = cand[near[cand] >= 0]
    ok = np.all(np.isfinite(sp[cand]), axis=1) & np.all(np.isfinite(tp[near[cand]]), axis=1) if len(cand) else np.zeros(0, dtype=bool)
    cand = cand[ok]
    return np.stack([cand, near[cand]], axis=1).astype(np.int32)


def _edge(a, b):
    d = a - b
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def tuples(lst, target32, source32, seed, tuple_thresh, max_num_tuples):
    """step 2: (the new list, number of tuples kept, number of passing trials, smallest margin |lo / hi - thresh| over the decided edges)"""
    C = len(lst)
    if C < 3:
        return np.zeros((0, 2), dtype=np.int32), 0, 0, np.inf
    sp, tp = _f64(source32), _f64(target32)
    trials = min(100 * C, MAX_TRIALS)
    c = (hashes((int(seed) + 1) & R.MASK, np.arange(3 * trials)) % np.uint64(C)).astype(np.int64).reshape(trials, 3)
    ok = (c[:, 0] != c[:, 1]) & (c[:, 1] != c[:, 2]) & (c[:, 0] != c[:, 2])
    margin = np.inf
    for a, b in ((0, 1), (1, 2), (2, 0)):
        ds = _edge(sp[lst[c[:, a], 0]], sp[lst[c[:, b], 0]])
        dt = _edge(tp[lst[c[:, a], 1]], tp[lst[c[:, b], 1]])
        lo, hi = np.minimum(ds, dt), np.maximum(ds, dt)
        ok &= (hi > 0) & (lo >= tuple_thresh * hi)
        with np.errstate(invalid="ignore", divide="ignore"):
            m = np.abs(lo / hi - tuple_thresh)
        distinct = (c[:, 0] != c[:, 1]) & (c[:, 1] != c[:, 2]) & (c[:, 0] != c[:, 2]) & (hi > 0)
        if distinct.any():
            margin = min(margin, float(m[distinct].min()))
    passing = np.nonzero(ok)[0]
    kept = passing[:max_num_tuples]
    return lst[c[kept].ravel()].astype(np.int32), len(kept), len(passing), margin


def tree_sum(x):
    """sum over axis 0 of x (n, m) in the documented tree: per lane in ascending order, xor-butterfly over the 64 lanes of a wavefront
    (offsets 32 .. 1), the wavefront sums in wavefront order"""
    x = np.asarray(x, dtype=np.float64)
    n, m = x.shape
    rows = (n + LANES - 1) // LANES
    acc = np.zeros((LANES, m))
    for r in range(rows):
        chunk = x[r * LANES:(r + 1) * LANES]
        acc[:len(chunk)] = acc[:len(chunk)] + chunk
    acc = acc.reshape(LANES // 64, 64, m)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ off]
    total = acc[0, 0].copy()
    for w in range(1, LANES // 64):
        total = total + acc[w, 0]
    return total


def points_of(lst, target32, source32):
    return _f64(source32)[lst[:, 0]], _f64(target32)[lst[:, 1]]


def frame(P, Q):
    """step 4: c_s, c_t (the documented tree, so bitwise the device's), D2, mu_0 and mu_min's default"""
    n = float(len(P))
    c_s, c_t = tree_sum(P) / n, tree_sum(Q) / n
    ds, dt = P.max(axis=0) - P.min(axis=0), Q.max(axis=0) - Q.min(axis=0)
    D2 = max((ds[0] * ds[0] + ds[1] * ds[1]) + ds[2] * ds[2], (dt[0] * dt[0] + dt[1] * dt[1]) + dt[2] * dt[2])
    return c_s, c_t, float(D2)


def mu_min_of(D2, max_corr_dist):
    if max_corr_dist > 0:
        return max_corr_dist * max_corr_dist
    m = 0.025 * np.sqrt(D2)
    return m * m


def horn_matrix(H):
    return np.array([[H[0, 0] + H[1, 1] + H[2, 2], H[1, 2] - H[2, 1], H[2, 0] - H[0, 2], H[0, 1] - H[1, 0]],
                     [H[1, 2] - H[2, 1], H[0, 0] - H[1, 1] - H[2, 2], H[0, 1] + H[1, 0], H[2, 0] + H[0, 2]],
                     [H[2, 0] - H[0, 2], H[0, 1] + H[1, 0], H[1, 1] - H[0, 0] - H[2, 2], H[1, 2] + H[2, 1]],
                     [H[0, 1] - H[1, 0], H[2, 0] + H[0, 2], H[1, 2] + H[2, 1], H[2, 2] - H[0, 0] - H[1, 1]]])


def pose_of_weights(P, Q, w, dof):
    """the weighted least-squares pose (Kabsch by SVD; dof 4: yaw by atan2) and the conditioning figures of the module docstring"""
    W = float(w.sum())
    ps, qs = (w[:, None] * P).sum(axis=0) / W, (w[:, None] * Q).sum(axis=0) / W
    A, B = P - ps, Q - qs
    H = (w[:, None] * A).T @ B
    if dof == 4:
        S, Cc = H[0, 1] - H[1, 0], H[0, 0] + H[1, 1]
        yaw = np.arctan2(S, Cc)
        Rm = np.array([[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
        gap = float(np.hypot(S, Cc))
    else:
        U, _, Vt = np.linalg.svd(H)
        d = np.sign(np.linalg.det(Vt.T @ U.T))
        Rm = Vt.T @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ U.T
        ev = np.linalg.eigvalsh(horn_matrix(H))
        gap = float(ev[-1] - ev[-2])
    T = np.eye(4)
    T[:3, :3] = Rm
    T[:3, 3] = qs - Rm @ ps
    return T, W, H, gap


def step(P, Q, T_in, mu, dof):
    """one iteration of step 5 from the pose T_in (3 x 4 or 4 x 4) at `mu`: dict(T 4 x 4, W, cost, cost_abs, w, gap, S, far_p, far_q, moments)"""
    T_in = np.asarray(T_in, dtype=np.float64)
    d = Q - (P @ T_in[:3, :3].T + T_in[:3, 3])
    m = np.abs(Q) + np.abs(P) @ np.abs(T_in[:3, :3]).T + np.abs(T_in[:3, 3])
    r2 = np.sum(d ** 2, axis=1)
    w = (mu / (mu + r2)) ** 2
    T, W, H, gap = pose_of_weights(P, Q, w, dof)
    c_s, c_t = P.mean(axis=0), Q.mean(axis=0)
    p, q = P - c_s, Q - c_t
    np_, nq = np.linalg.norm(p, axis=1), np.linalg.norm(q, axis=1)
    moments = {"W": W, "a": (w[:, None] * p).sum(axis=0), "b": (w[:, None] * q).sum(axis=0), "M": (w[:, None] * p).T @ q, "c_s": c_s, "c_t": c_t}
    return {"T": T, "W": W, "cost": float(np.sum(w * r2)), "w": w, "gap": gap, "S": float(np.sum(w * np_ * nq)), "far_p": float(np_.max()),
            "far_q": float(nq.max()), "moments": moments, "cost_abs": float(np.sum(w * (r2 + 2.0 * np.sum(np.abs(d) * m, axis=1))))}


def step_gates(st, n):
    """(rotation gate [rad], translation gate, gate of W, gate of cost) of one step over n list entries"""
    rot = GATE_C * n * EPS * st["S"] / st["gap"]
    return rot, rot * st["far_p"] + GATE_C * n * EPS * st["far_q"], GATE_C * n * EPS * st["W"], GATE_C * n * EPS * st["cost_abs"]


def run(P, Q, dof, max_iterations=64, div_factor=1.4, max_corr_dist=0.0):
    """free-running steps 4 and 5: dict(T, iterations_run, mu (per iteration), mu_final, W, cost)"""
    _, _, D2 = frame(P, Q)
    mu, mu_min = D2, mu_min_of(D2, max_corr_dist)
    T = np.eye(4)
    out = {"T": T, "iterations_run": 0, "mu": [], "mu_final": mu, "W": 0.0, "cost": 0.0}
    for k in range(max_iterations):
        with np.errstate(all="ignore"):
            try:
                st = step(P, Q, T, mu, dof)
            except np.linalg.LinAlgError:
                break
        if not (np.isfinite(st["W"]) and np.all(np.isfinite(st["T"]))):
            break
        T = st["T"]
        out.update(T=T, iterations_run=k + 1, mu_final=mu, W=st["W"], cost=st["cost"])
        out["mu"].append(mu)
        if k % 4 == 3 and mu > mu_min:
            mu = max(mu / div_factor, mu_min)
    return out


def inliers(T, target32, source32, res, delta):
    """(count, ambiguous) of RANSAC's rule for pose T over all finite source points"""
    sp = _f64(source32)
    finite = np.all(np.isfinite(sp), axis=1)
    return R.score(T, sp, finite, R._occ_keys(R.occupancy(target32, res)), res, delta)
