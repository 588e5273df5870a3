"""Host-side SE(3) helpers (numpy): gtsam::Pose3 conventions, tangent [omega; v], T (+) xi = T @ exp(xi)."""
import numpy as np


def hat(a):
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


def se3_exp(xi):
    xi = np.asarray(xi, dtype=np.float64).reshape(6)
    w, v = xi[:3], xi[3:]
    th2 = float(w @ w)
    th = np.sqrt(th2)
    W = hat(w)
    W2 = W @ W
    if th < 1e-8:
        a, b, c = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
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
    """gtsam::Pose3::Logmap: [omega; v] with exp(se3_log(T)) == T (rotation angle < pi)."""
    T = np.asarray(T, dtype=np.float64)
    R = T[:3, :3]
    vee = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    th = np.arctan2(np.linalg.norm(vee), 0.5 * (np.trace(R) - 1.0))
    f = 1.0 + th * th / 6.0 + 7.0 * th**4 / 360.0 if th < 0.02 else th / np.sin(th)
    w = f * vee
    W = hat(w)
    if th < 0.02:
        b, c = 0.5 - th**2 / 24.0 + th**4 / 720.0, 1.0 / 6.0 - th**2 / 120.0 + th**4 / 5040.0
    else:
        b, c = (1.0 - np.cos(th)) / th**2, (th - np.sin(th)) / th**3
    V = np.eye(3) + b * W + c * W @ W
    return np.concatenate([w, np.linalg.solve(V, T[:3, 3])])
