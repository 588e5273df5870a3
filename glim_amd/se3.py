"""Host-side SE(3) helpers (numpy): gtsam::Pose3 conventions, tangent [omega; v], T (+) xi = T @ exp(xi)."""
import numpy as np


SERIES = 0.02    # below: Taylor series of the coefficients whose numerators cancel (csrc/ct_se3.hpp CT_SERIES)
LOG_SYM = 0.3    # se3_log: sin(th) below which, past a quarter turn, the axis comes from the symmetric part (csrc/ct_se3.hpp CT_LOG_SYM)


def hat(a):
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


def se3_exp(xi):
    xi = np.asarray(xi, dtype=np.float64).reshape(6)
    w, v = xi[:3], xi[3:]
    th2 = float(w @ w)
    th = np.sqrt(th2)
    W = hat(w)
    W2 = W @ W
    if th < SERIES:  # the closed forms cancel: (1 - cos th) / th^2 is off by 2e-8 of itself at 1e-4 (csrc/ct_se3.hpp switches here too)
        a, b, c = 1.0 - th2 / 6.0 + th2 * th2 / 120.0, 0.5 - th2 / 24.0 + th2 * th2 / 720.0, 1.0 / 6.0 - th2 / 120.0 + th2 * th2 / 5040.0
    else:
        a, b, c = np.sin(th) / th, (1.0 - np.cos(th)) / th2, (th - np.sin(th)) / (th2 * th)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * W + b * W2
    T[:3, 3] = (np.eye(3) + b * W + c * W2) @ v
    return T


def solve_damped(H, b, lam=0.0):
    """Gauss-Newton / LM step: (H + lam I) x = -b."""
    return np.linalg.solve(np.asarray(H) + lam * np.eye(6), -np.asarray(b))


def se3_log(T):
    """gtsam::Pose3::Logmap: [omega; v] with exp(se3_log(T)) == T, up to and including the half turn (csrc/ct_se3.hpp se3_log: the axis from
    R - R^T, and near pi, where that vanishes, from the symmetric part (R + R^T) / 2 - cos(th) I = (1 - cos th) n n^T)."""
    T = np.asarray(T, dtype=np.float64)
    R = T[:3, :3]
    vee = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, cth = np.linalg.norm(vee), 0.5 * (np.trace(R) - 1.0)
    th = np.arctan2(s, cth)
    if cth < 0.0 and s < LOG_SYM:
        j = int(np.argmax(np.diag(R)))
        n = 0.5 * (R[:, j] + R[j, :])
        n[j] -= cth
        d = n @ vee
        if d < 0.0 or (d == 0.0 and n[np.flatnonzero(n)[0]] < 0.0):
            n = -n
        w = th * n / np.linalg.norm(n)
    else:
        f = 1.0 + th * th / 6.0 + 7.0 * th**4 / 360.0 + 31.0 * th**6 / 15120.0 if th < SERIES else th / np.sin(th)
        w = f * vee
    W = hat(w)
    if th < SERIES:
        b, c = 0.5 - th**2 / 24.0 + th**4 / 720.0, 1.0 / 6.0 - th**2 / 120.0 + th**4 / 5040.0
    else:
        b, c = (1.0 - np.cos(th)) / th**2, (th - np.sin(th)) / th**3
    V = np.eye(3) + b * W + c * W @ W
    return np.concatenate([w, np.linalg.solve(V, T[:3, 3])])
