"""FP64 NumPy restatement of the continuous-time GICP factor (gtsam_points::IntegratedCT_GICPFactor, odometry_estimation_ct.cpp:158-183) for
tests/test_ct_gicp.py, tests/test_ivox.py, tests/ivox_restatement.py and the timing tools: gtsam::Pose3 with right-perturbation Jacobians, the
time table, the bucket poses T_k with D0_k / D1_k, the oracle's per-bucket GICP terms through the chain rule, the comparison of two records,
and the moving-sensor scenes.  A plain module: it holds no tests."""
import numpy as np

POSE_TOL = 1e-4
SERIES = 0.02
Q_SERIES = 1.0  # csrc/ct_se3.hpp CT_Q_SERIES: the coefficients of Q are their series below this



def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def so3_coeffs(th):
    if th < SERIES:
        return 0.5 - th**2 / 24 + th**4 / 720, 1 / 6 - th**2 / 120 + th**4 / 5040
    return (1 - np.cos(th)) / th**2, (th - np.sin(th)) / th**3


def alt_series(t2, k0):
    """sum_k (-1)^k t2^k / (2 k + k0)!, ten terms nested (csrc/ct_se3.hpp alt_series)"""
    s = 1.0
    for k in range(9, 0, -1):
        s = 1.0 - s * t2 / ((2 * k + k0 - 1) * (2 * k + k0))
    return s / float(np.prod(np.arange(2, k0 + 1)))


def expmap(xi):
    w, v = np.asarray(xi[:3], float), np.asarray(xi[3:], float)
    th = np.linalg.norm(w)
    W = hat(w)
    a = 1 - th**2 / 6 + th**4 / 120 if th < SERIES else np.sin(th) / th
    b, c = so3_coeffs(th)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * W + b * W @ W
    T[:3, 3] = (np.eye(3) + b * W + c * W @ W) @ v
    return T


def logmap(T):
    from glim_amd.se3 import se3_log

    return se3_log(T)


def adjoint(T):
    R, t = T[:3, :3], T[:3, 3]
    A = np.zeros((6, 6))
    A[:3, :3] = A[3:, 3:] = R
    A[3:, :3] = hat(t) @ R
    return A


def expmap_derivative(xi):
    """Pose3::ExpmapDerivative: [[Jw, 0], [Q, Jw]] (gtsam computeQforExpmapDerivative)."""
    w, rho = np.asarray(xi[:3], float), np.asarray(xi[3:], float)
    th = np.linalg.norm(w)
    W, V = hat(w), hat(rho)
    b, c = so3_coeffs(th)
    Jw = np.eye(3) - b * W + c * W @ W
    if th < Q_SERIES:
        ca, cb = alt_series(th**2, 3), -alt_series(th**2, 4)
        cc = -0.5 * (cb + 3 * alt_series(th**2, 5))
    else:
        ca, cb = (th - np.sin(th)) / th**3, (1 - th**2 / 2 - np.cos(th)) / th**4
        cc = -0.5 * (cb - 3 * (th - np.sin(th) - th**3 / 6) / th**5)
    Q = -0.5 * V + ca * (W @ V + V @ W - W @ V @ W) + cb * (W @ W @ V + V @ W @ W - 3 * W @ V @ W) + cc * (W @ V @ W @ W + W @ W @ V @ W)
    J = np.zeros((6, 6))
    J[:3, :3] = J[3:, 3:] = Jw
    J[3:, :3] = Q
    return J


def time_table(times):
    """IntegratedCT_ICPFactor's constructor: a new bucket when t - table.back() > 1e-3, entries / max(1e-9, table.back())."""
    table, idx = [], np.zeros(len(times), dtype=np.int32)
    for i, t in enumerate(times):
        if not table or t - table[-1] > 1e-3:
            table.append(float(t))
        idx[i] = len(table) - 1
    table = np.array(table)
    if len(table):
        table = table / max(1e-9, table[-1])
    return table, idx


def ct_poses(table, X, Y):
    """T_k = X Exp(t_k Log(X^-1 Y)); D0 = H_c1 + H_c2 H_exp t_k H_log H_b1, D1 = H_c2 H_exp t_k H_log H_b2."""
    delta = np.linalg.inv(X) @ Y
    vel = logmap(delta)
    H_log = np.linalg.inv(expmap_derivative(vel))
    H_b1 = -adjoint(np.linalg.inv(delta))
    Ts, D0s, D1s = [], [], []
    for t in table:
        E = expmap(t * vel)
        G = expmap_derivative(t * vel) @ (t * H_log)
        Ts.append(X @ E)
        D0s.append(adjoint(np.linalg.inv(E)) + G @ H_b1)
        D1s.append(G)
    return np.array(Ts).reshape(-1, 4, 4), np.array(D0s).reshape(-1, 6, 6), np.array(D1s).reshape(-1, 6, 6)


def np_ct_linearize(orc, tp, tc, sp, sc, times, X, Y, max_d, poses=None):
    """The factor at (X, Y): per bucket, the oracle's GICP linearisation at T_k, then the chain rule in FP64.  poses: (T, D0, D1) to use
    instead of the restatement's own (the library's, so that correspondences can be compared bit for bit)."""
    table, idx = time_table(times)
    T, D0, D1 = poses if poses is not None else ct_poses(table, X, Y)
    out = dict(num_inliers=0, error=0.0, H_00=np.zeros((6, 6)), H_01=np.zeros((6, 6)), H_11=np.zeros((6, 6)), b_0=np.zeros(6), b_1=np.zeros(6))
    corr = np.full(len(sp), -1, dtype=np.int32)
    if len(sp) == 0 or len(tp) == 0:
        out["corr"] = corr
        return out
    for k in range(len(table)):
        sel = np.flatnonzero(idx == k)
        L = orc.gicp_linearize(tp, tc, sp[sel], sc[sel], T[k], max_d, want_corr=True)
        corr[sel] = L["corr"]
        out["num_inliers"] += L["num_inliers"]
        out["error"] += L["error"]
        out["H_00"] += D0[k].T @ L["H_ss"] @ D0[k]
        out["H_01"] += D0[k].T @ L["H_ss"] @ D1[k]
        out["H_11"] += D1[k].T @ L["H_ss"] @ D1[k]
        out["b_0"] += D0[k].T @ L["b_s"]
        out["b_1"] += D1[k].T @ L["b_s"]
    out["corr"] = corr
    return out


def frozen_error(tp, tc, sp, sc, times, corr, X_lin, Y_lin, X, Y):
    """error() after linearize() at (X_lin, Y_lin): the correspondences and M of the linearisation point, residuals at (X, Y)."""
    table, idx = time_table(times)
    Tl, _, _ = ct_poses(table, X_lin, Y_lin)
    Te, _, _ = ct_poses(table, X, Y)
    e = 0.0
    for i in np.flatnonzero(corr >= 0):
        k, j = idx[i], corr[i]
        R = Tl[k][:3, :3]
        M = np.linalg.inv(tc[j] + R @ sc[i] @ R.T)
        r = tp[j] - (Te[k][:3, :3] @ sp[i] + Te[k][:3, 3])
        e += r @ M @ r
    return e


def full_system(L):
    H = np.block([[L["H_00"], L["H_01"]], [L["H_01"].T, L["H_11"]]])
    return H, np.concatenate([L["b_0"], L["b_1"]])


def gn_step(L, lam=0.0):  # of a record of either size: the rigid (H_ss, b_s) or the CT factor's 12-dof system
    H, b = (L["H_ss"], L["b_s"]) if "H_ss" in L else full_system(L)
    return np.linalg.solve(H + lam * np.eye(len(b)), -b)


def _check_record(got, ref, step=True):
    """step = False: without the Gauss-Newton step, for a system so short of pairs that the damping decides the step"""
    assert got["num_inliers"] == ref["num_inliers"] > 0
    np.testing.assert_allclose(got["error"], ref["error"], rtol=2e-4)
    Hg, bg = full_system(got)
    Hr, br = full_system(ref)
    scale = np.abs(Hr).max()
    np.testing.assert_allclose(Hg, Hr, rtol=0, atol=2e-4 * scale)
    np.testing.assert_allclose(bg, br, rtol=0, atol=2e-4 * np.abs(br).max() + 1e-6 * scale)
    lam = 1e-6 * np.trace(Hr) / 12
    assert not step or np.abs(gn_step(got, lam) - gn_step(ref, lam)).max() < POSE_TOL


def _prior(T, T0, prec):
    xi = logmap(np.linalg.inv(T0) @ T)
    J = np.linalg.inv(expmap_derivative(xi))
    return prec * J.T @ J, prec * J.T @ xi, prec * xi @ xi


# ---- workloads ------------------------------------------------------------------------------------------------------------------------
T_BEGIN_ARGS = (-10.0, -6.0, 1.8, np.radians(10.0))


def sweep_poses():
    """a 0.1 s sweep moving ~1 m forward and yawing 5 degrees"""
    from glim_amd import synth

    x, y, z, yaw = T_BEGIN_ARGS
    T0 = synth.pose(x, y, z, yaw)
    T1 = synth.pose(x + 1.0 * np.cos(yaw), y + 1.0 * np.sin(yaw), z + 0.02, yaw + np.radians(5.0), pitch=0.005)
    return T0, T1


def static_map(rings, az):
    """the target: two static scans around the sweep, in the world frame (float32 like every cloud)"""
    from glim_amd import synth

    scene = synth.Scene.default()
    dirs = synth.lidar_directions(rings, az)
    T0, T1 = sweep_poses()
    pts = []
    for i, T in enumerate((synth.pose(-10.5, -6.3, 1.7, 0.1), synth.pose(-9.0, -5.5, 1.9, 0.3))):
        p = synth.scan(scene, T, dirs, frame_id=10 + i).astype(np.float64)
        pts.append(p @ T[:3, :3].T + T[:3, 3])
    return np.concatenate(pts).astype(np.float32).astype(np.float64)


def moving_source(rings, az):
    from glim_amd import synth

    T0, T1 = sweep_poses()
    p, t = synth.moving_scan(synth.Scene.default(), T0, T1, rings, az, duration=0.1, frame_id=3)
    return p.astype(np.float64), t


# the scenes as device clouds
def _target(api, ctx, rings, az):
    tp = static_map(rings, az)
    tg = api.PointCloudGPU.clone(tp, ctx=ctx)
    tg.find_neighbors(10, download=False)
    tg.estimate_covariances(10)
    _, tc, _ = tg.download(covs=True, normals=False)
    return tp, tc.astype(np.float64), tg


def _source(api, ctx, kind):
    """'pre10k': a 64 x 1024 sweep through the shipped preprocessing (random grid, ~10 000 points, times kept on the device);
    'raw131k': a 128 x 1024 sweep uploaded as it is, times handed to the factor."""
    if kind == "pre10k":
        p, t = moving_source(64, 1024)
        sg = api.PointCloudGPU.preprocess(p, t, None, ctx=ctx)
        sg.estimate_covariances(10)
        times = sg.download_frame()["times"]
        pass_times = None
    else:
        p, t = moving_source(128, 1024)
        sg = api.PointCloudGPU.clone(p, ctx=ctx)
        sg.find_neighbors(10, download=False)
        sg.estimate_covariances(10)
        times = pass_times = t
    sp, sc, _ = sg.download(covs=True, normals=False)
    return sp.astype(np.float64), sc.astype(np.float64), times, pass_times, sg
