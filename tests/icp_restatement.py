"""NumPy FP64 restatement of the ICP factors (include/glim_amd.h "ICP factors"): gtsam_points::IntegratedICPFactor (point-to-point) and
IntegratedPointToPlaneICPFactor (residual and Jacobian weighted elementwise by the target normal).  Brute-force exact nearest neighbour, ties
to the smaller index; the record dict the other restatements return (num_inliers, error, H_ss, b_s, corr).  A plain module: it holds no tests."""
from fractions import Fraction

import numpy as np


def hat_all(p):
    """hat(p_i) of every row: n x 3 x 3"""
    H = np.zeros((len(p), 3, 3))
    H[:, 0, 1], H[:, 0, 2] = -p[:, 2], p[:, 1]
    H[:, 1, 0], H[:, 1, 2] = p[:, 2], -p[:, 0]
    H[:, 2, 0], H[:, 2, 1] = -p[:, 1], p[:, 0]
    return H


def _fma(a, b, c):
    """a * b + c with one rounding (NumPy has no fused multiply-add): exact rationals, then the correctly rounded double"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def transform(sp, T):
    """q = T p as the factors form it (device_math.hpp transform_point_d, the oracle's order): fma(T0, x, fma(T1, y, fma(T2, z, t))) per row.
    The search compares FP64 distances from q, so q is restated to the bit."""
    T = [[float(v) for v in row] for row in np.asarray(T, dtype=np.float64)[:3]]
    q = np.zeros((len(sp), 3))
    for i, (x, y, z) in enumerate(np.asarray(sp, dtype=np.float64).tolist()):
        for r in range(3):
            q[i, r] = _fma(T[r][0], x, _fma(T[r][1], y, _fma(T[r][2], z, T[r][3])))
    return q


def nearest(tp, q, chunk=256):
    """exact nearest target point of every q: squared distance (dx^2 + dy^2) + dz^2 in FP64, the first (smallest) index among equals
    -> (index, squared distance); (-1, inf) over an empty target"""
    j, d2 = np.full(len(q), -1, dtype=np.int64), np.full(len(q), np.inf)
    if len(tp) == 0:
        return j, d2
    tx, ty, tz = (np.ascontiguousarray(tp[:, k]) for k in range(3))
    for a in range(0, len(q), chunk):
        dx, dy, dz = q[a:a + chunk, 0:1] - tx, q[a:a + chunk, 1:2] - ty, q[a:a + chunk, 2:3] - tz
        d = (dx * dx + dy * dy) + dz * dz
        k = np.argmin(d, axis=1)  # the first occurrence of the minimum: the smaller index
        j[a:a + chunk], d2[a:a + chunk] = k, d[np.arange(len(k)), k]
    return j, d2


def correspondences(nn, max_d):
    j, d2 = nn
    return np.where(d2 <= max_d * max_d, j, -1)


def icp_linearize(tp, sp, T, max_d, normals=None, corr=None, q=None):
    """the record at T.  normals: the target's, n x 3 -> point-to-plane; None -> point-to-point.  corr: frozen correspondences, or None: the
    exact nearest neighbours within max_d.  q: transform(sp, T) when the caller has it"""
    tp, sp, T = np.asarray(tp, dtype=np.float64), np.asarray(sp, dtype=np.float64), np.asarray(T, dtype=np.float64)
    R = T[:3, :3]
    if q is None:
        q = transform(sp, T)
    if corr is None:
        corr = correspondences(nearest(tp, q), max_d)
    ok = np.flatnonzero(corr >= 0)
    r = tp[corr[ok]] - q[ok]                                                     # m x 3
    J = np.concatenate([R @ hat_all(sp[ok]), np.broadcast_to(-R, (len(ok), 3, 3))], axis=2)  # m x 3 x 6: [R hat(p) | -R]
    if normals is not None:
        n = np.asarray(normals, dtype=np.float64)[corr[ok]]
        r, J = n * r, n[:, :, None] * J
    H = np.einsum("mki,mkj->ij", J, J)
    b = np.einsum("mki,mk->i", J, r)
    return dict(H_ss=H, b_s=b, error=float(np.sum(r * r)), num_inliers=int(len(ok)), corr=corr)
