"""The 28 sums of a factor record, point by point, and the gate each of them is held to.  A plain module (NumPy only): it holds no tests.

The factor kernels -- accumulate_point (vgicp.hip), gicp_point (gicp_factor.hpp), icp_point (icp_factor.hpp) -- add 28 FP32 terms per matched point
(device_math.hpp "record math"):

    0..5   Hww = hat(l)^T M hat(l)  (00 01 02 11 12 22)      6..14  G = hat(l) M  (row-major)      15..20  M  (00 01 02 11 12 22)
    21..23 u x l                                              24..26 u = M r                        27      e = r . u

with the lever arm l = q' = R p and M, r in the TARGET frame for VGICP, l = p and M, r in the SOURCE frame for GICP and ICP.  Every function
below returns these terms as an n x 28 array, one row per matched pair, in the dtype asked for:

  float64   the reference: every stage in FP64.
  float32   what is formed in which precision follows the kernel stage for stage -- q = T p and what is subtracted from it in FP64 and then
            rounded, the rotation, the covariance sandwich, the inverse and everything after them in FP32 -- but NOT its order of operations,
            its fused multiply-adds or its reciprocal-plus-Newton step: the products are NumPy's, the division is a division.  The ALGEBRAIC
            form of the inverse is the kernel's (adjugate over determinant, _inv; Sherman-Morrison in the plane form), because its
            conditioning is part of what FP32 costs there.  An independent evaluation in the same precision, whose distance from the
            reference measures what FP32 costs at this point, with this conditioning.

gate():  with c64, c32 the two arrays,  S_j = sum c64[:, j],  P_j = sum |c32[:, j] - c64[:, j]|,  Q_j = sum |c64[:, j]|,

    gate_j = m P_j + s 2^-24 Q_j + 64 2^-53 max|block of S that holds j|

  m P_j          the device's per-point rounding is another draw from the distribution the FP32 restatement drew from, and P_j adds absolute values
                 (no cancellation between points is assumed); m = 2 by default, never above 8 (M_MAX)
  s 2^-24 Q_j    the FP32 additions a term passes through on its way to the block's partial row: at most ppt in its thread, six DPP steps
                 across the wavefront, then (w0 + w1) + (w2 + w3) -- s = ppt + 8 (additions()).  The rows are added in FP64.
  the last term  the FP64 rotation of the finaliser and its inverse here (sums_of_record): some 30 operations on the entries of one block

Slots whose terms are all integers computed without rounding (the zeros and counts of point-to-point ICP) are exact(): compared with ==.

The continuous-time factor (the last section): the same 28 terms per point, at the pose of the point's time bucket (ct_terms); the 92 entries
of its record from the bucket sums through the chain rule [D0_k | D1_k] (ct_record); the gate of each entry propagated from the buckets'
gates with no cancellation assumed (ct_gate); and ct_error_kernel's one term per kept pair with its gate (ct_frozen_terms, error_gate).
"""
import numpy as np

NSLOTS = 28
M_DEFAULT = 2.0
M_MAX = 8.0
BLOCKS = (slice(0, 6), slice(6, 15), slice(15, 21), slice(21, 24), slice(24, 27), slice(27, 28))
SLOT_NAMES = (["Hww00", "Hww01", "Hww02", "Hww11", "Hww12", "Hww22"] + [f"G{r}{c}" for r in range(3) for c in range(3)]
              + ["M00", "M01", "M02", "M11", "M12", "M22", "bw0", "bw1", "bw2", "u0", "u1", "u2", "e"])
_UR, _UC = np.array([0, 0, 0, 1, 1, 2]), np.array([0, 1, 2, 1, 2, 2])
MEAN_SCALE = 2.0 ** 28  # voxelmap.hip: the fixed-point unit of a voxel's coordinate sums


def hat(v):
    """n x 3 -> n x 3 x 3, hat(a) b = a x b, in v's dtype"""
    o = np.zeros((len(v), 3, 3), dtype=v.dtype)
    o[:, 0, 1], o[:, 0, 2] = -v[:, 2], v[:, 1]
    o[:, 1, 0], o[:, 1, 2] = v[:, 2], -v[:, 0]
    o[:, 2, 0], o[:, 2, 1] = -v[:, 1], v[:, 0]
    return o


def rodrigues(w):
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    K = hat(w[None] / th)[0]
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * K @ K


def perturbed(delta, w=(0.006, -0.005, 0.0062), v=(0.03, -0.028, 0.029)):
    """delta times a rigid perturbation of 0.01 rad / 0.05 m"""
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = rodrigues(w), v
    return np.asarray(delta, dtype=np.float64) @ P


def transform(T, p):
    """q = T p in FP64, n x 3; T: one pose (4 x 4) or one per point (n x 4 x 4)"""
    T, p = np.asarray(T, dtype=np.float64), np.asarray(p, dtype=np.float64)
    if T.ndim == 3:
        return np.einsum("nij,nj->ni", T[:, :3, :3], p) + T[:, :3, 3]
    return p @ T[:3, :3].T + T[:3, 3]


def _terms(M, r, lever):
    """the 28 terms from the metric M (n x 3 x 3), the residual r and the lever arm (n x 3), all of one dtype"""
    dt = M.dtype
    assert r.dtype == dt and lever.dtype == dt
    H = hat(lever)
    G = H @ M
    Hww = -(G @ H)
    u = np.einsum("nij,nj->ni", M, r)
    c = np.zeros((len(M), NSLOTS), dtype=dt)
    c[:, 0:6] = Hww[:, _UR, _UC]
    c[:, 6:15] = G.reshape(-1, 9)
    c[:, 15:21] = M[:, _UR, _UC]
    c[:, 21:24] = np.cross(u, lever)
    c[:, 24:27] = u
    c[:, 27] = np.einsum("ni,ni->n", r, u)
    assert c.dtype == dt
    return c


def _inv(S):
    """FP64: LAPACK's inverse.  FP32: the adjugate over the determinant, the algebraic form of the kernels' general path (accumulate_point,
    gicp_point) -- in NumPy's own order of operations, with a true division and no fused multiply-add.  The form is part of the stage: the
    determinant of S = C_B + R C_A R^T cancels (eigenvalues 0.02, 2, 2 here), and an LU inverse in FP32 does not show that error -- with
    LAPACK's inverse in this place the device stood 12.4 P_j from the reference on G00 of a one-point GICP factor and 4.2 P_j on Hww01 of a
    33-point VGICP factor, inside the gate only through its other terms (one run on an MI355X)."""
    if len(S) == 0:
        return S.copy()
    if S.dtype == np.float64:
        return np.linalg.inv(S)
    a, b, c, d, e, f = S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]
    k = [d * f - e * e, c * e - b * f, b * e - c * d, a * f - c * c, b * c - a * e, a * d - b * b]
    det = (c * k[2] + b * k[1]) + a * k[0]
    M = np.empty_like(S)
    M[:, _UR, _UC] = M[:, _UC, _UR] = np.stack(k, axis=1) / det[:, None]
    assert M.dtype == S.dtype
    return M


# the six ways to relabel the coordinate axes that keep a right-handed frame (signed permutations of determinant +1): the identity, the two
# cyclic ones, and the three swaps with the third axis reversed
_AXES = np.array([[[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, 1, 0], [0, 0, 1], [1, 0, 0]], [[0, 0, 1], [1, 0, 0], [0, 1, 0]],
                  [[0, 1, 0], [1, 0, 0], [0, 0, -1]], [[1, 0, 0], [0, 0, 1], [0, -1, 0]], [[0, 0, 1], [0, -1, 0], [1, 0, 0]]], dtype=np.float64)
assert all(abs(np.linalg.det(A) - 1.0) < 1e-15 for A in _AXES)


def _sym(u):
    A = np.zeros((len(u), 3, 3), dtype=u.dtype)
    A[:, _UR, _UC] = A[:, _UC, _UR] = u
    return A


def _mv(A, v):
    """A v per row: (n | 1) x 3 x 3 times n x 3"""
    return (A @ v[:, :, None])[:, :, 0]


def _t(A):
    return A.transpose(0, 2, 1)


def _finish(axes, build, *parts):
    """the terms of (M, r, lever) = build(*parts); parts: n x 3 vectors and (n | 1) x 3 x 3 matrices of one dtype -- everything the kernel
    forms in FP32 is formed inside build.  axes = 1..5: the same evaluation in relabelled axes -- v' = A v, C' = A C A^T with A = _AXES[axes]
    before build, the terms carried back after; products with 0 and +-1 are exact, so this is the same mathematics to the last sign with
    other roundings: further FP32 draws of every term (draws())."""
    if axes == 0:
        return _terms(*build(*parts))
    A = _AXES[axes].astype(parts[0].dtype)
    c = _terms(*build(*[x @ A.T if x.ndim == 2 else A @ x @ A.T for x in parts]))
    back = lambda X: A.T @ X @ A  # noqa: E731
    out = np.empty_like(c)
    out[:, 0:6], out[:, 15:21] = back(_sym(c[:, 0:6]))[:, _UR, _UC], back(_sym(c[:, 15:21]))[:, _UR, _UC]
    out[:, 6:15] = back(c[:, 6:15].reshape(-1, 3, 3)).reshape(-1, 9)
    out[:, 21:24], out[:, 24:27], out[:, 27] = c[:, 21:24] @ A, c[:, 24:27] @ A, c[:, 27]
    assert out.dtype == c.dtype
    return out


def _vgicp_frame(p, coord, mu_rel, T, res, dt, T_eval):
    """the VGICP stages that do not depend on the form: (R in dt, 1 x 3 x 3; r = mu - q relative to the voxel centre in dt; q' = R p in dt).
    Linearising call: the in-voxel fraction q / res - coord is formed in FP64 and rounded; FP32 from there.  Frozen call (T_eval: the error
    at another pose over the same voxels): T_eval p minus the voxel centre in FP64, rounded.  q' = q - t in FP64, rounded."""
    T = np.asarray(T, dtype=np.float64)
    q = transform(T, p)
    coord = np.asarray(coord, dtype=np.float64)
    if T_eval is not None:
        qr = (transform(T_eval, p) - (coord + 0.5) * res).astype(dt)
    elif dt == np.float64:
        qr = q - (coord + 0.5) * res
    else:
        qr = ((q * (1.0 / res) - coord).astype(dt) - dt(0.5)) * dt(res)
    r = np.asarray(mu_rel).astype(dt) - qr
    return T[None, :3, :3].astype(dt), r, (q - T[:3, 3]).astype(dt)


def vgicp_general(p, CA, coord, mu_rel, CB, T, res, dtype, T_eval=None, axes=0):
    """accumulate_point, general form.  p, CA: the matched source points (FP32 values) and their covariances; coord, mu_rel, CB: per pair the
    integer coordinate of its voxel, the voxel's mean relative to the voxel centre and its covariance (FP32 values, as the table holds
    them); T: the linearisation pose.  M = (C_B + R C_A R^T)^-1."""
    dt = np.dtype(dtype).type
    R, r, lever = _vgicp_frame(p, coord, mu_rel, T, res, dt, T_eval)
    return _finish(axes, lambda CB, CA, R, r, lever: (_inv(CB + R @ CA @ _t(R)), r, lever), np.asarray(CB).astype(dt), np.asarray(CA).astype(dt), R, r, lever)


def plane_view(CB):
    """A_B = (C_B + I)^-1 of the table's FP32 covariances, inverted in FP64 and stored in FP32 (voxelmap.hip plane_record)"""
    return _inv(np.asarray(CB, dtype=np.float32).astype(np.float64) + np.eye(3)).astype(np.float32)


def vgicp_plane(p, nrm, coord, mu_rel, AB, T, res, dtype, T_eval=None, w=0.999, axes=0):
    """accumulate_point, plane form: the source covariance is I - 0.999 n n^T (nrm: the FP32 normals the cloud streams), the table's plane
    view holds A_B = (C_B + I)^-1, and M = (C_B + I - 0.999 m m^T)^-1 = A_B + c v v^T by Sherman-Morrison: m = R n, v = A_B m,
    c = 0.999 / (1 - 0.999 m . v).  (w: the constant, for the mutation tests.)"""
    dt = np.dtype(dtype).type
    R, r, lever = _vgicp_frame(p, coord, mu_rel, T, res, dt, T_eval)

    def sherman_morrison(AB, R, n, r, lever):
        m = _mv(R, n)
        v = _mv(AB, m)
        c = dt(w) / (dt(1.0) - dt(w) * np.einsum("ni,ni->n", m, v))
        return AB + c[:, None, None] * v[:, :, None] * v[:, None, :], r, lever

    return _finish(axes, sherman_morrison, np.asarray(AB).astype(dt), R, np.asarray(nrm).astype(dt), r, lever)


def _source_frame(p, b, T, dt):
    """the GICP / ICP stages in front of the FP32 algebra: (R in dt, (1 | n) x 3 x 3; r = b - q formed in FP64 and rounded; the lever arm p).
    T: one pose, or one per point (the continuous-time factor: the pose of the point's bucket)"""
    T = np.asarray(T, dtype=np.float64)
    R = T[:, :3, :3] if T.ndim == 3 else T[None, :3, :3]
    return R.astype(dt), (np.asarray(b, dtype=np.float64) - transform(T, p)).astype(dt), np.asarray(p).astype(dt)


def gicp(p, CA, b, CB, T, dtype, transpose=False, axes=0):
    """gicp_point.  p, CA: matched source points and covariances; b, CB: their target points and covariances.  M = (R^T C_B R + C_A)^-1 and
    r_s = R^T r, in the source frame.  (transpose: R C_B R^T in its place, for the mutation tests.)"""
    dt = np.dtype(dtype).type
    R, r, lever = _source_frame(p, b, T, dt)

    def build(CB, CA, R, r, lever):
        Rm = _t(R) if transpose else R
        return _inv(_t(Rm) @ CB @ Rm + CA), _mv(_t(R), r), lever

    return _finish(axes, build, np.asarray(CB).astype(dt), np.asarray(CA).astype(dt), R, r, lever)


def icp_point(p, b, T, dtype, axes=0):
    """icp_point, point-to-point: M = I"""
    dt = np.dtype(dtype).type
    R, r, lever = _source_frame(p, b, T, dt)
    eye = np.broadcast_to(np.eye(3, dtype=dt), (len(lever), 3, 3)).copy()
    return _finish(axes, lambda R, r, lever: (eye, _mv(_t(R), r), lever), R, r, lever)


def icp_plane(p, b, nrm, T, dtype, axes=0):
    """icp_point, point-to-plane: M = R^T diag(n^2) R with n the target normal of the pair"""
    dt = np.dtype(dtype).type
    R, r, lever = _source_frame(p, b, T, dt)
    n = np.asarray(nrm).astype(dt)
    N = np.zeros((len(n), 3, 3), dtype=dt)
    N[:, [0, 1, 2], [0, 1, 2]] = n * n
    return _finish(axes, lambda N, R, r, lever: (_t(R) @ N @ R, _mv(_t(R), r), lever), N, R, r, lever)


# ---- the gate ---------------------------------------------------------------------------------------------------------------------------
def additions(ppt):
    """FP32 additions between a term and the block's partial row: ppt in the thread, six across the wavefront, two across the four wavefronts"""
    return ppt + 6 + 2


def block_max(S):
    out = np.zeros(NSLOTS)
    for b in BLOCKS:
        out[b] = np.abs(S[b]).max()
    return out


def exact(c32, c64):
    """slots whose terms are integers that both precisions form without rounding"""
    return np.all(c64 == np.rint(c64), axis=0) & np.all(c32.astype(np.float64) == c64, axis=0) & (np.abs(c64).sum(axis=0) < 2.0 ** 24)


def draws(terms):
    """terms: axes -> the FP32 terms.  The six draws of the FP32 restatement, K x n x 28; [0] is the restatement as it stands"""
    return np.stack([terms(axes) for axes in range(len(_AXES))])


def gate(c32, c64, s, m=M_DEFAULT):
    """-> dict S (reference sums), P, Q, gate (28 each), exact (28 booleans).  c32: the FP32 terms, or draws() of them: P_j then takes, point
    by point, the largest |c32 - c64| of the draws.  One draw is one rounding error per term, and the ratio of two such errors (the device's
    over the restatement's) has no bound worth the name when a factor has one point or a few: with single draws the device stood 23 P_j
    from the reference on slot 27 of a one-point GICP factor whose restated term happened to be right to a quarter of an FP32 step, and 8.2 P_j
    on G10 of a one-point point-to-plane factor -- inside the gate through its other terms (one run on an MI355X)."""
    c32 = c32[None] if c32.ndim == 2 else c32
    assert c32.dtype == np.float32 and c64.dtype == np.float64 and c32.shape[1:] == c64.shape and 0 < m <= M_MAX
    S, Q = c64.sum(axis=0), np.abs(c64).sum(axis=0)
    P = np.abs(c32.astype(np.float64) - c64).max(axis=0).sum(axis=0)
    ex = np.all([exact(c, c64) for c in c32], axis=0)
    return dict(S=S, P=P, Q=Q, exact=ex, gate=m * P + s * 2.0 ** -24 * Q + 64 * 2.0 ** -53 * block_max(S))


def old_gate(S):
    """what the suite's 2e-4-of-the-largest-entry rule allows each of the 28 sums: 2e-4 max|H| on 0..20, 2e-4 max|b| + 1e-6 max|H| on 21..26,
    2e-4 |e| on 27.  (A rotation does not change the size of the largest entry by more than sqrt(3).)"""
    out = np.zeros(NSLOTS)
    out[:21] = 2e-4 * np.abs(S[:21]).max()
    out[21:27] = 2e-4 * np.abs(S[21:27]).max() + 1e-6 * np.abs(S[:21]).max()
    out[27] = 2e-4 * abs(S[27])
    return out


def check(sums, g, label=""):
    """asserts the device's 28 sums against a gate() result; returns the ratios |sums - S| / P (nan where P = 0) for the record"""
    sums = np.asarray(sums, dtype=np.float64)
    err = np.abs(sums - g["S"])
    ex = g["exact"]
    bad_exact = [SLOT_NAMES[j] for j in np.flatnonzero(ex) if sums[j] != g["S"][j]]
    assert not bad_exact, f"{label}: exact slots differ: {bad_exact}"
    over = [(j, SLOT_NAMES[j], err[j] / g["gate"][j]) for j in np.flatnonzero(~ex) if not err[j] <= g["gate"][j]]
    assert not over, f"{label}: slots beyond their gate (slot, name, error / gate): {over}"
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(~ex & (g["P"] > 0), err / g["P"], np.nan)


# ---- compact record <-> the 28 sums -----------------------------------------------------------------------------------------------------
def _D(T):
    D = np.eye(6)
    if T is not None:
        R = np.asarray(T, dtype=np.float64)[:3, :3]
        D[:3, :3] = D[3:, 3:] = R
    return D


def sums_of_record(L, T=None):
    """the 28 accumulated sums behind a record (dict with H_ss, b_s, error), in FP64.  VGICP (T: the factor's pose): the finaliser stored
    H_ss = D^T H' D, b_s = D^T b' with D = diag(R, R) (device_math.hpp rotate_part), so H' = D H_ss D^T, b' = D b_s.  GICP and ICP (T = None):
    their finaliser (gicp_factor.hpp compact_entry) rotates nothing -- the sums are already source-frame -- so D = I.  Both store
    b_s = [sums 21..23, -sums 24..26] and the 21 upper entries of H' row-major."""
    D = _D(T)
    H, b = D @ np.asarray(L["H_ss"], dtype=np.float64) @ D.T, D @ np.asarray(L["b_s"], dtype=np.float64)
    out = np.zeros(NSLOTS)
    out[0:6], out[6:15], out[15:21] = H[:3, :3][_UR, _UC], H[:3, 3:].reshape(9), H[3:, 3:][_UR, _UC]
    out[21:24], out[24:27], out[27] = b[:3], -b[3:], L["error"]
    return out


def record_of_sums(S, T=None, num_inliers=0):
    """the record the finalisers make of 28 sums: the inverse of sums_of_record"""
    D = _D(T)
    H = np.zeros((6, 6))
    H[:3, :3][_UR, _UC], H[3:, 3:][_UR, _UC] = S[0:6], S[15:21]
    H[:3, :3][_UC, _UR], H[3:, 3:][_UC, _UR] = S[0:6], S[15:21]
    H[:3, 3:] = np.reshape(S[6:15], (3, 3))
    H[3:, :3] = H[:3, 3:].T
    b = np.concatenate([S[21:24], -np.asarray(S[24:27])])
    return dict(H_ss=D.T @ H @ D, b_s=D.T @ b, error=float(S[27]), num_inliers=int(num_inliers))


def adjoint(T):
    """Adjoint(T^-1) in [omega; v] order (record_expand.hpp binary_adjoint): H_tt = Ad^T H_ss Ad, H_ts = -Ad^T H_ss, b_t = -Ad^T b_s"""
    T = np.asarray(T, dtype=np.float64)
    R, t = T[:3, :3], T[:3, 3]
    Ad = np.zeros((6, 6))
    Ad[:3, :3] = Ad[3:, 3:] = R.T
    Ad[3:, :3] = -R.T @ hat(t[None])[0]
    return Ad


# ---- teacher-forced inputs --------------------------------------------------------------------------------------------------------------
def voxel_coords(points, res):
    """floor(p * (1 / res)) per axis in FP64: the voxel of a point (the same expression on the same operands as the map's insert)"""
    return np.floor(np.asarray(points, dtype=np.float64)[:, :3] * (1.0 / res)).astype(np.int64)


def voxel_table(points, covs, res):
    """The records of a voxel map built by ONE insert of (points, covs), restated: {(cx, cy, cz): (count, mean relative to the voxel centre as
    FP32, mean covariance as FP32)}.  The map adds every coordinate as the integer rint(p 2^28) and stores
    (float)(sum (1 / n / 2^28) - (c + 0.5) res) (voxelmap.hip finalize_slot): integers, so the sum has no order and this is the record's value.
    The table keeps the mean RELATIVE to the centre -- 24 bits of a number below res / 2 -- which a download of absolute FP32 means (at 30 m:
    2e-6 m a step) no longer shows; absolute_means() is what such a download must give, and the GPU tests assert that it does.
    The covariances here are the FP64 means rounded once (CPU tests); the GPU tests take the table's own from the download, which is exact."""
    p = np.asarray(points, dtype=np.float32).astype(np.float64)[:, :3]
    c = voxel_coords(p, res)
    uniq, inv = np.unique(c, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    cnt = np.bincount(inv, minlength=len(uniq))
    fixed = np.zeros((len(uniq), 3), dtype=np.int64)
    np.add.at(fixed, inv, np.rint(p * MEAN_SCALE).astype(np.int64))
    csum = np.zeros((len(uniq), 3, 3))
    np.add.at(csum, inv, np.asarray(covs, dtype=np.float64)[:, :3, :3])
    inv_n = 1.0 / cnt.astype(np.float64)
    rel = (fixed.astype(np.float64) * (inv_n / MEAN_SCALE)[:, None] - (uniq + 0.5) * res).astype(np.float32)
    C = (csum * inv_n[:, None, None]).astype(np.float32)
    return {tuple(int(x) for x in u): (int(k), m, S) for u, k, m, S in zip(uniq, cnt, rel, C)}


def absolute_means(coords, rel, res):
    """the absolute FP32 mean a download forms from a record (glim_amd_voxelmap_download)"""
    return (np.asarray(rel, dtype=np.float32).astype(np.float64) + (np.asarray(coords, dtype=np.float64) + 0.5) * res).astype(np.float32)


def lookup(table, coords):
    """per row of coords: (hit, count, mu_rel, C_B) from a voxel_table; rows without a voxel are zero"""
    n = len(coords)
    hit, mu, CB = np.zeros(n, dtype=bool), np.zeros((n, 3), dtype=np.float32), np.zeros((n, 3, 3), dtype=np.float32)
    for i, row in enumerate(np.asarray(coords)):
        v = table.get(tuple(int(x) for x in row))
        if v is not None:
            hit[i], mu[i], CB[i] = True, v[1], v[2]
    return hit, mu, CB


def nearest(tp, q, max_d, chunk=256):
    """exact nearest target point of every q within max_d (FP64 (dx^2 + dy^2) + dz^2, the smaller index among equals), -1 without one"""
    tp = np.asarray(tp, dtype=np.float64)
    j = np.full(len(q), -1, dtype=np.int64)
    for a in range(0, len(q), chunk):
        d = q[a:a + chunk, None, :] - tp[None]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        k = np.argmin(d2, axis=1)
        j[a:a + chunk] = np.where(d2[np.arange(len(k)), k] <= max_d * max_d, k, -1)
    return j


# ---- the scenes the CPU and the GPU tests share (pair: the suite's small_pair) ------------------------------------------------------------
SHIFT = np.array([200.0, -200.0, 0.0])
GENERAL = 0.01  # added to the diagonal of the scan's covariances: "general" ones, as test_small_cloud_host_pack_equals_the_device_pack makes them


def c33(c):
    return np.asarray(c, dtype=np.float64)[:, :3, :3]


def vgicp_scene(pair, plane, shift=False, n=None):
    """target map input and source cloud of a VGICP case, every array holding FP32 values: plane = the scan's own covariances (the cloud is in
    plane form, its normals streamed), else covariances + 0.01 I.  shift: map and pose moved by 200 m.  n: the first n source points."""
    t, s = pair["target"], pair["source"]
    off = SHIFT if shift else np.zeros(3)
    T = perturbed(pair["delta"])
    T[:3, 3] += off
    sc = c33(s["covs"]) if plane else (c33(s["covs"]) + GENERAL * np.eye(3)).astype(np.float32).astype(np.float64)
    n = len(s["points"]) if n is None else n
    return dict(tp=(t["points"].astype(np.float64) + off).astype(np.float32), tc=c33(t["covs"]), sp=s["points"][:n].astype(np.float32), sc=sc[:n],
                sn=s["normals"][:n].astype(np.float32), T=T, plane=plane)


def vgicp_matched(scene, res, table, coords=None):
    """the matched pairs of a VGICP scene over a voxel table ({coord: (count, mu_rel, C_B)}).  coords: the voxel of every source point as the
    device reports it, else computed here"""
    if coords is None:
        coords = voxel_coords(transform(scene["T"], scene["sp"]), res)
    hit, mu, CB = lookup(table, coords)
    i = np.flatnonzero(hit)
    return dict(idx=i, p=scene["sp"][i], CA=scene["sc"][i], nrm=scene["sn"][i], coord=np.asarray(coords)[i], mu_rel=mu[i], CB=CB[i], AB=plane_view(CB[i]), res=res,
                n=len(scene["sp"]))


def vgicp_terms(scene, m, dtype, T=None, T_eval=None, **kw):
    T = scene["T"] if T is None else T
    if scene["plane"]:
        return vgicp_plane(m["p"], m["nrm"], m["coord"], m["mu_rel"], m["AB"], T, m["res"], dtype, T_eval=T_eval, **kw)
    return vgicp_general(m["p"], m["CA"], m["coord"], m["mu_rel"], m["CB"], T, m["res"], dtype, T_eval=T_eval, **kw)


def vgicp_draws(scene, m, T=None, T_eval=None):
    return draws(lambda axes: vgicp_terms(scene, m, np.float32, T=T, T_eval=T_eval, axes=axes))


def gicp_scene(pair, n=None):
    """target and source of a GICP / ICP case: covariances + 0.01 I on both sides, the target's normals for point-to-plane; FP32 values"""
    t, s = pair["target"], pair["source"]
    n = len(s["points"]) if n is None else n
    gen = lambda c: (c33(c) + GENERAL * np.eye(3)).astype(np.float32).astype(np.float64)  # noqa: E731
    return dict(tp=t["points"].astype(np.float32), tc=gen(t["covs"]), tn=t["normals"].astype(np.float32), sp=s["points"][:n].astype(np.float32),
                sc=gen(s["covs"])[:n], T=perturbed(pair["delta"]))


def gicp_matched(scene, corr):
    """corr: per source point the index of its target point, or -1"""
    i = np.flatnonzero(np.asarray(corr) >= 0)
    j = np.asarray(corr)[i]
    return dict(idx=i, p=scene["sp"][i], CA=scene["sc"][i], b=scene["tp"][j], CB=scene["tc"][j], nrm=scene["tn"][j], n=len(scene["sp"]))


def gicp_terms(scene, m, kind, dtype, T=None, **kw):
    T = scene["T"] if T is None else T
    if kind == "gicp":
        return gicp(m["p"], m["CA"], m["b"], m["CB"], T, dtype, **kw)
    if kind == "icp_point":
        return icp_point(m["p"], m["b"], T, dtype, **kw)
    assert kind == "icp_plane"
    return icp_plane(m["p"], m["b"], m["nrm"], T, dtype, **kw)


def gicp_draws(scene, m, kind, T=None):
    return draws(lambda axes: gicp_terms(scene, m, kind, np.float32, T=T, axes=axes))


def device_sum(c32, idx, n, ppt):
    """The 28 sums of the FP32 terms added in the SHAPE of the device's reduction (not its assignment of points to lanes): blocks of 256 ppt
    consecutive points; a thread adds its ppt points in FP32; a wavefront adds its 64 lanes as a binary tree of six levels; the block adds
    (w0 + w1) + (w2 + w3); the blocks are added in FP64.  c32: the terms of the matched points, idx: their positions among the n points."""
    nb = max(1, -(-n // (256 * ppt)))
    full = np.zeros((nb * ppt * 256, NSLOTS), dtype=np.float32)
    full[idx] = c32
    x = full.reshape(nb, ppt, 256, NSLOTS)
    acc = np.zeros((nb, 256, NSLOTS), dtype=np.float32)
    for it in range(ppt):
        acc = acc + x[:, it]
    w = acc.reshape(nb, 4, 64, NSLOTS)
    while w.shape[2] > 1:
        w = w[:, :, 0::2] + w[:, :, 1::2]
    w = w[:, :, 0]
    assert w.dtype == np.float32
    rows = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    return rows.astype(np.float64).sum(axis=0)


# ---- the continuous-time factor (ct_factor.hpp; ct_gicp_kernel, ct_bucket_kernel, ct_sum_kernel, ct_error_kernel of gicp.hip) -----------------
CT_ROW = 92  # the record ct_expand_record reads: count, error, the 78 upper entries of the 12 x 12 H (row-major), the 12 of b
_U12 = np.triu_indices(12)
CT_NAMES = ["count", "error"] + [f"H{r}_{c}" for r, c in zip(*_U12)] + [f"b{r}" for r in range(12)]
CT_BLOCK = 256


def points_per_thread(n, num_cus=256):
    """gicp_factor.hpp points_per_thread, restated: the points a thread takes so that the cloud makes at least four blocks of 256 threads per
    compute unit.  1 up to 262 144 points on a part with 256 compute units; the CT blocks are cut by it (BLOCK * ppt points each)."""
    target_blocks = max(1, 4 * num_cus)
    return max(1, min(64, -(-n // (CT_BLOCK * target_blocks))))


def ct_matched(scene, corr, bucket):
    """corr: per source point the index of its target point, or -1; bucket: the time bucket of every source point"""
    i = np.flatnonzero(np.asarray(corr) >= 0)
    j = np.asarray(corr)[i]
    return dict(idx=i, p=scene["sp"][i], CA=scene["sc"][i], b=scene["tp"][j], CB=scene["tc"][j], bucket=np.asarray(bucket)[i], n=len(scene["sp"]),
                all_buckets=np.asarray(bucket))


def ct_terms(scene, m, dtype, poses, axes=0):
    """ct_gicp_block: the 28 source-frame terms of every matched point -- gicp_point, at the pose T[k] of the point's bucket.  poses: T, nbk x 4 x 4
    (scene is not read: the matched set carries the points; kept for the signature the other *_terms share)"""
    return gicp(m["p"], m["CA"], m["b"], m["CB"], np.asarray(poses, dtype=np.float64)[m["bucket"]], dtype, axes=axes)


def ct_draws(scene, m, poses):
    return draws(lambda axes: ct_terms(scene, m, np.float32, poses, axes=axes))


def _arrange(S):
    """the 6 x 6 and the 6 the finalisers make of 28 numbers WITHOUT the sign of b's second half: for gates and absolute sums"""
    r = record_of_sums(np.abs(S))
    return r["H_ss"], np.abs(r["b_s"])


def bucket_sums(c, bucket, nbk):
    """nbk x 28: the terms of every bucket added in FP64"""
    S = np.zeros((nbk, NSLOTS))
    np.add.at(S, np.asarray(bucket), np.asarray(c, dtype=np.float64))
    return S


def ct_record_of_bucket_sums(S, count, D0, D1):
    """ct_bucket_block and ct_sum_rows in FP64: per bucket (H_k, b_k) = record_of_sums(S_k) -- the compact record's convention,
    b = [sums 21..23, -sums 24..26] -- and J_k = [D0_k | D1_k]; the record is sum_k J_k^T H_k J_k, sum_k J_k^T b_k, sum_k S_k[27], the count"""
    H, b, e = np.zeros((12, 12)), np.zeros(12), 0.0
    for k in range(len(S)):
        r = record_of_sums(S[k])
        J = np.hstack([D0[k], D1[k]])
        H += J.T @ r["H_ss"] @ J
        b += J.T @ r["b_s"]
        e += r["error"]
    return np.concatenate([[float(count), e], H[_U12], b])


def ct_record(c, bucket_of_point, D0, D1):
    """the 92 entries of the CT record from the terms c (one row per matched point) and the bucket of each of these points"""
    return ct_record_of_bucket_sums(bucket_sums(c, bucket_of_point, len(D0)), len(c), D0, D1)


def ct_record_of(L):
    """the 92 entries behind a linearisation as the API hands it out (H_00, H_01, H_11, b_0, b_1): ct_expand_record undone"""
    H = np.block([[L["H_00"], L["H_01"]], [L["H_01"].T, L["H_11"]]])
    return np.concatenate([[float(L["num_inliers"]), L["error"]], H[_U12], L["b_0"], L["b_1"]])


def ct_dict(rec):
    """ct_expand_record: the API's dict of a 92-entry record"""
    H = np.zeros((12, 12))
    H[_U12] = rec[2:80]
    H = H + np.triu(H, 1).T
    return dict(num_inliers=int(round(rec[0])), error=float(rec[1]), H_00=H[:6, :6], H_01=H[:6, 6:], H_11=H[6:, 6:], b_0=rec[80:86].copy(), b_1=rec[86:92].copy())


def ct_gate(c32_draws, c64, bucket_of_point, D0, D1, s, m=M_DEFAULT):
    """The gate of each of the 92 entries.  -> dict S (the FP64 record), P, gate (92 each).

    Per bucket k the 28 sums S^k_j have the gate gate^k_j of gate() over that bucket's points (s = additions(1) = 9: a CT block takes one point
    per thread).  Every record entry is linear in the bucket sums, E = sum_k sum_j a^k_Ej S^k_j with the a made of entries of J_k = [D0_k | D1_k],
    and no cancellation between buckets or slots is assumed: gate_E = sum_k sum_j |a^k_Ej| gate^k_j -- for H, |J_k|^T G_k |J_k| with G_k the
    6 x 6 arrangement of the 21 gates; for b, |J_k|^T g_k; for the error, sum_k gate^k_27.  P_E is propagated the same way from the P^k_j.
    (gate^k_j carries 64 2^-53 of the bucket's block maxima: here it stands for the FP64 additions of the bucket's partial rows, at most 64.)

    On top, the device's own FP64 arithmetic: in ct_bucket_block an entry of W = H_k J_k is a 6-term dot product (6 roundings at most on any
    term: its product and five additions) and the entry of J_k^T W another one (6 more); ct_sum_rows then adds the nbk bucket rows (at most
    nbk additions on any term, in whatever grouping).  count = 6 + 6 + nbk roundings, and the gate takes TWICE count 2^-53 of the
    absolute-value sum sum_k |J_k|^T |H_k| |J_k| (|J_k|^T |b_k|, sum_k |e_k|).  Entry 0, the count, is exact: compared with ==."""
    c32 = c32_draws[None] if c32_draws.ndim == 2 else c32_draws
    nbk = len(D0)
    bucket = np.asarray(bucket_of_point)
    out = {k: np.zeros(CT_ROW) for k in ("P", "gate", "A")}
    for k in np.unique(bucket):
        sel = bucket == k
        g = gate(c32[:, sel], c64[sel], s, m)
        aJ = np.abs(np.hstack([D0[k], D1[k]]))
        for key, v in (("P", g["P"]), ("gate", g["gate"]), ("A", g["S"])):
            H6, b6 = _arrange(v)
            out[key][2:80] += (aJ.T @ H6 @ aJ)[_U12]
            out[key][80:92] += aJ.T @ b6
            out[key][1] += abs(v[27])
    fp64 = 2.0 * (6 + 6 + nbk) * 2.0 ** -53 * out["A"]
    S = ct_record(c64, bucket, D0, D1)
    return dict(S=S, P=out["P"], gate=out["gate"] + fp64, fp64=fp64)


def ct_check(rec, g, label=""):
    """asserts a device record (92 entries) against a ct_gate() result; returns |rec - S| / P per entry (nan for the count and where P = 0)"""
    rec = np.asarray(rec, dtype=np.float64)
    assert rec[0] == g["S"][0], f"{label}: count {rec[0]} != {g['S'][0]}"
    err = np.abs(rec - g["S"])
    over = [(CT_NAMES[j], err[j] / g["gate"][j]) for j in range(1, CT_ROW) if not err[j] <= g["gate"][j]]
    assert not over, f"{label}: entries beyond their gate (name, error / gate): {over}"
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(g["P"] > 0, err / g["P"], np.nan)
    r[0] = np.nan
    return r


def ct_device_sums(c32, m, ppt=1):
    """nbk x 28: the FP32 terms added in the shape of the CT factor's reduction -- every bucket's index run cut into blocks of 256 ppt points
    (device_sum per bucket: FP32 inside a block, FP64 across the blocks of the bucket)"""
    allb = m["all_buckets"]
    nbk = int(allb.max()) + 1 if len(allb) else 0
    S = np.zeros((nbk, NSLOTS))
    for k in range(nbk):
        run = np.flatnonzero(allb == k)
        assert len(run) and np.all(np.diff(run) == 1)  # a bucket is one contiguous index run (the time table never goes back)
        sel = m["bucket"] == k
        S[k] = device_sum(c32[sel], m["idx"][sel] - run[0], len(run), ppt)
    return S


def ct_frozen_terms(m, T_lin, T_eval, dtype, axes=0, rotate=True, R_from_eval=False):
    """ct_error_kernel after a linearising ct_gicp_block: per kept pair e = r . (M r) with M = R A R^T the kept target-frame metric,
    A = (R^T C_B R + C_A)^-1 by _inv, R the rotation of the LINEARISATION pose of the pair's bucket (FP32 in the FP32 form), and
    r = b - T_eval,k p formed in FP64 and rounded.  M is formed as the kernel forms it, W = R A and then W R^T, in NumPy's own order of
    operations.  T_lin, T_eval: nbk x 4 x 4.  -> n values.  (rotate = False: A left in the source frame; R_from_eval: the evaluation pose's
    rotation in M -- the mutation tests.)"""
    dt = np.dtype(dtype).type
    Tl, Te = np.asarray(T_lin, dtype=np.float64)[m["bucket"]], np.asarray(T_eval, dtype=np.float64)[m["bucket"]]
    R = (Te if R_from_eval else Tl)[:, :3, :3].astype(dt)
    r = (np.asarray(m["b"], dtype=np.float64) - transform(Te, m["p"])).astype(dt)

    def build(CB, CA, R, r, lever):
        A = _inv(_t(R) @ CB @ R + CA)
        return ((R @ A) @ _t(R) if rotate else A), r, lever

    return _finish(axes, build, np.asarray(m["CB"]).astype(dt), np.asarray(m["CA"]).astype(dt), R, r, np.asarray(m["p"]).astype(dt))[:, 27]


def ct_frozen_draws(m, T_lin, T_eval):
    return np.stack([ct_frozen_terms(m, T_lin, T_eval, np.float32, axes=a) for a in range(len(_AXES))])


def error_gate(e32_draws, e64, s, m=M_DEFAULT):
    """slot 27's gate for a kernel that adds one term per pair (ct_error_kernel): dict of the scalars S, P, Q, gate"""
    pad = lambda e: np.concatenate([np.zeros(e.shape + (NSLOTS - 1,), dtype=e.dtype), e[..., None]], axis=-1)  # noqa: E731
    g = gate(pad(e32_draws), pad(e64), s, m)
    return {k: float(g[k][27]) for k in ("S", "P", "Q", "gate")}
