"""FP64 restatement in NumPy of the RANSAC global registration as include/glim_amd.h ("RANSAC") states it, independent in method: the same
integer draws, the pose by SVD (Kabsch) instead of Horn's quaternion + Jacobi, the occupancy as a Python set of integer triples.
tests/test_ransac*.py check the library against this; nothing here touches the library.

Per hypothesis it also returns how close each decision came to going the other way and how well conditioned the pose is:
  cond          sigma_1 / sigma_2 of the centred source triangle (inf when sigma_2 = 0)
  edge_margin   min over the three edges of | min(d_s, d_t) / max(d_s, d_t) - (1 - thresh) |
  col_margin    | sigma_2 / sigma_1 - 1e-6 |
  ambiguous     source points for which some axis of (R p + t) / res lies within delta / res of an integer, delta the position gate

Gates (they follow from the arithmetic): the rotation between two correct FP64 solutions of one triangle differs by an angle of at most
GATE_C * 2^-52 * cond^2 -- Horn's matrix has eigen-gap ~ 2 sigma_2(H) and norm ~ sigma_1(H), and the sigma(H) scale as the triangle's squared;
GATE_C = 64 is slack for the Jacobi sweeps and the SVD side.  Translation: that angle * (largest source-point norm) + GATE_C * 2^-52 * (largest
target-point norm).  Position gate delta: the same bound with the farthest source point of the cloud."""
import numpy as np

MASK = (1 << 64) - 1
GATE_C = 64.0
EPS = 2.0 ** -52
COLLINEAR_RATIO = 1e-6
KEY_LIMIT = float(1 << 20)


def sample_hash(seed, index):
    """splitmix64 of seed + (index + 1) * golden (glim_amd_preprocess's counter-based generator)"""
    z = (int(seed) + (int(index) + 1) * 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def draw(seed, it, n_source):
    return [sample_hash(seed, 3 * it + k) % n_source for k in range(3)]


def _norm3(d):
    return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def rotation_angle(Ra, Rb):
    """angle of Ra^T Rb, from the skew part and the trace (accurate near 0)"""
    D = Ra.T @ Rb
    s = 0.5 * np.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2)
    c = 0.5 * (np.trace(D) - 1.0)
    return float(np.arctan2(s, c))


def solve(s, t, thresh, dof):
    """s, t: 3 x 3 FP64 (rows = points).  Returns dict(status 0 | 3 | 4, T 4 x 4, cond, edge_margin, col_margin)."""
    out = {"status": 0, "T": np.eye(4), "cond": np.inf, "edge_margin": np.inf, "col_margin": np.inf}
    if not (np.all(np.isfinite(s)) and np.all(np.isfinite(t))):
        out["status"] = 4
        return out
    ok = True
    for a, b in ((0, 1), (1, 2), (2, 0)):
        ds, dt = _norm3(s[a] - s[b]), _norm3(t[a] - t[b])
        lo, hi = min(ds, dt), max(ds, dt)
        ok = ok and lo >= (1.0 - thresh) * hi
        if hi > 0:
            out["edge_margin"] = min(out["edge_margin"], abs(lo / hi - (1.0 - thresh)))
        else:
            out["edge_margin"] = 0.0
    if not ok:
        out["status"] = 3
        return out
    cs, ct = s.mean(axis=0), t.mean(axis=0)
    A, B = s - cs, t - ct
    sv = np.linalg.svd(A, compute_uv=False)
    if sv[0] > 0:
        out["cond"] = sv[0] / sv[1] if sv[1] > 0 else np.inf
        out["col_margin"] = abs(sv[1] / sv[0] - COLLINEAR_RATIO)
    else:
        out["col_margin"] = 0.0
    if sv[0] == 0 or sv[1] < COLLINEAR_RATIO * sv[0]:
        out["status"] = 4
        return out
    if dof == 4:
        S = np.sum(A[:, 0] * B[:, 1] - A[:, 1] * B[:, 0])
        Cc = np.sum(A[:, 0] * B[:, 0] + A[:, 1] * B[:, 1])
        yaw = np.arctan2(S, Cc)
        R = np.array([[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
    else:
        U, _, Vt = np.linalg.svd(A.T @ B)  # H = sum a b^T; R = V diag(1, 1, det) U^T
        d = np.sign(np.linalg.det(Vt.T @ U.T))
        R = Vt.T @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ U.T
    out["T"][:3, :3] = R
    out["T"][:3, 3] = ct - R @ cs
    return out


def occupancy(target32, res):
    """set of integer voxel triples of the finite, in-range target points"""
    p = np.asarray(target32, dtype=np.float32).astype(np.float64)[:, :3]
    with np.errstate(invalid="ignore", over="ignore"):
        v = p * (1.0 / res)
        ok = np.all(np.isfinite(v), axis=1) & np.all((v >= -KEY_LIMIT) & (v < KEY_LIMIT), axis=1)
    c = np.floor(v[ok]).astype(np.int64)
    return set(map(tuple, c))


def _occ_keys(occ):
    if not occ:
        return np.zeros(0, dtype=np.int64)
    c = np.array(sorted(occ), dtype=np.int64) + (1 << 20)
    return np.sort((c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2])


def score(T, source64, finite, occ_keys, res, delta):
    """(inliers, ambiguous) of pose T over the source points (FP64 n x 3; `finite` marks the rows that take part)"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = (source64 @ T[:3, :3].T + T[:3, 3]) * (1.0 / res)
        ok = finite & np.all(np.isfinite(v), axis=1) & np.all((v >= -KEY_LIMIT) & (v < KEY_LIMIT), axis=1)
        fl = np.floor(v)
        near = np.abs(v - np.rint(v)) <= delta / res
        surely_out = np.any(~np.isfinite(v) | (np.abs(v) > KEY_LIMIT + 1.0), axis=1)  # some axis decides "no inlier" whatever the rounding
    ambiguous = int(np.sum(finite & ~surely_out & np.any(near, axis=1)))
    c = fl[ok].astype(np.int64) + (1 << 20)
    keys = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    if len(occ_keys) == 0 or len(keys) == 0:
        return 0, ambiguous
    pos = np.searchsorted(occ_keys, keys)
    pos[pos == len(occ_keys)] = 0
    return int(np.sum(occ_keys[pos] == keys)), ambiguous


def pose_gates(cond, source_norm, target_norm):
    """(rotation gate [rad], translation gate) of a hypothesis of condition `cond`"""
    ang = GATE_C * EPS * cond * cond
    return ang, ang * source_norm + GATE_C * EPS * target_norm


def hypotheses(target32, source32, nearest, seed, thresh, res, dof, first, count, score_them=True):
    """every hypothesis of [first, first + count): dict of arrays samples, status, T (count x 4 x 4), inliers, cond, edge_margin, col_margin,
    ambiguous (0 where status != 0)"""
    tp = np.asarray(target32, dtype=np.float32).astype(np.float64)[:, :3]
    sp = np.asarray(source32, dtype=np.float32).astype(np.float64)[:, :3]
    n = len(sp)
    finite = np.all(np.isfinite(sp), axis=1)
    occ_keys = _occ_keys(occupancy(target32, res)) if score_them else None
    far_s = float(np.max(np.linalg.norm(sp[finite], axis=1))) if finite.any() else 0.0
    tfin = np.all(np.isfinite(tp), axis=1)
    far_t = float(np.max(np.linalg.norm(tp[tfin], axis=1))) if tfin.any() else 0.0
    out = {"samples": np.zeros((count, 3), dtype=np.int32), "status": np.zeros(count, dtype=np.int32), "T": np.tile(np.eye(4), (count, 1, 1)),
           "inliers": np.zeros(count, dtype=np.int64), "cond": np.full(count, np.inf), "edge_margin": np.full(count, np.inf),
           "col_margin": np.full(count, np.inf), "ambiguous": np.zeros(count, dtype=np.int64), "far_source": far_s, "far_target": far_t}
    near = np.asarray(nearest)
    for j in range(count):
        s = draw(seed, first + j, n)
        out["samples"][j] = s
        t = [int(near[k]) for k in s]
        if min(t) < 0:
            out["status"][j] = 1
            continue
        if len(set(s)) < 3 or len(set(t)) < 3:
            out["status"][j] = 2
            continue
        r = solve(sp[s], tp[t], thresh, dof)
        for k in ("status", "cond", "edge_margin", "col_margin"):
            out[k][j] = r[k]
        if r["status"] != 0:
            continue
        out["T"][j] = r["T"]
        if score_them:
            _, delta = pose_gates(min(r["cond"], 1e8), far_s, far_t)
            out["inliers"][j], out["ambiguous"][j] = score(r["T"], sp, finite, occ_keys, res, delta)
    return out


def sequential_result(status, inliers, n_source, early_stop_inlier_rate, max_iterations):
    """the result rule applied to per-hypothesis records (arrays over it = 0 .. max_iterations - 1): (best_iteration, num_inliers, iterations_run)"""
    thr = early_stop_inlier_rate * float(n_source)
    best, best_count = -1, -1
    for it in range(max_iterations):
        if status[it] != 0:
            continue
        c = int(inliers[it])
        if float(c) >= thr:
            return it, c, it + 1
        if c > best_count:
            best, best_count = it, c
    return best, max(best_count, 0), max_iterations
