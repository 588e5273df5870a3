"""Deskewing: oracle pins on CPU (analytic cases + an independent scipy restatement of
src/glim/common/cloud_deskewing.cpp), HIP parity on the GPU."""
import numpy as np
import pytest


def make_case(seed=0, n=5000):
    rng = np.random.default_rng(seed)
    pts = (rng.normal(size=(n, 3)) * [15, 10, 2]).astype(np.float32).astype(np.float64)
    times = np.sort(rng.uniform(0.0, 0.1, n))
    times[: n // 50] = 0.0  # many points share the first time stamp
    return pts, times


def scipy_deskew_imu(orc, pts, times, Til, imu_times, imu_poses, stamp):
    from scipy.spatial.transform import Rotation, Slerp

    table, idx = [], []
    for t in times:  # cloud_deskewing.cpp:79-84
        if not table or t - table[-1] > 1e-4:
            table.append(t)
        idx.append(len(table) - 1)
    Tli = np.linalg.inv(Til)
    TT, cur, T0w = [], 0, None
    for i, tt in enumerate(table):
        time = stamp + tt
        while cur < len(imu_times) - 1 and imu_times[cur + 1] < time:
            cur += 1
        if i == 0:
            T0w = np.linalg.inv(imu_poses[cur])
        if cur + 1 >= len(imu_times):
            Tw1 = imu_poses[cur]
        else:
            p = max(0.0, min(1.0, (time - imu_times[cur]) / (imu_times[cur + 1] - imu_times[cur])))
            R = Slerp([0, 1], Rotation.from_matrix([imu_poses[cur][:3, :3], imu_poses[cur + 1][:3, :3]]))(p).as_matrix()
            Tw1 = np.eye(4)
            Tw1[:3, :3] = R
            Tw1[:3, 3] = (1 - p) * imu_poses[cur][:3, 3] + p * imu_poses[cur + 1][:3, 3]
        TT.append(Tli @ T0w @ Tw1 @ Til)
    return np.array([(TT[j] @ np.append(p, 1.0))[:3] for p, j in zip(pts, idx)]), len(table)


def imu_track(orc, seed=1):
    rng = np.random.default_rng(seed)
    imu_times = 100.0 + np.array([-0.02, 0.013, 0.031, 0.058, 0.09, 0.13])
    poses = [orc.se3_exp(rng.normal(size=6) * [0.3, 0.3, 0.3, 2, 2, 2])]
    for _ in imu_times[1:]:
        poses.append(poses[-1] @ orc.se3_exp(rng.normal(size=6) * [0.02, 0.02, 0.05, 0.05, 0.05, 0.02]))
    return imu_times, poses


# ---- designed tracks: the branches of the host table of glim_amd/csrc/deskew.hip that small random rotations never take ----------------------
DESIGNED_ANGLES = np.deg2rad([110.0, 118.0, 121.0, 150.0, 179.0, 179.9])  # trace > 0 below 120 degrees: arms w w i i i i of quat_from_rot
DESIGNED_AXES = {"+x": (1.0, 0.03, -0.02), "+y": (0.02, 1.0, 0.03), "+z": (-0.03, 0.02, 1.0), "-x": (-1.0, 0.02, 0.03)}
CONSTVEL_LINEAR = [4.0, -2.0, 0.3]
DESIGNED_FORMS = ["imu_turn+x", "imu_turn+y", "imu_turn+z", "imu_turn-x", "imu_identical", "constvel_1e-7", "constvel_3e-7", "imu_times_descend"]


def eigen_quat(R):
    """Eigen::Quaterniond(Matrix3d): (arm, (x, y, z, w)) -- arm "w" when the trace is positive, else the index of the largest diagonal entry.
    Only used to show that a designed track takes the arms it was designed for."""
    t = R[0, 0] + (R[1, 1] + R[2, 2])
    q = np.zeros(4)
    if t > 0.0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[:3] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
        return "w", q
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
    q[i] = 0.5 * t
    t = 0.5 / t
    q[3], q[j], q[k] = (R[k, j] - R[j, k]) * t, (R[j, i] + R[i, j]) * t, (R[k, i] + R[i, k]) * t
    return i, q


def turn_track(orc, axis):
    """six IMU poses at the imu_track times whose rotations are DESIGNED_ANGLES about (nearly) one coordinate axis"""
    a = np.array(DESIGNED_AXES[axis])
    a /= np.linalg.norm(a)
    rng = np.random.default_rng(31)
    return imu_track(orc)[0], [orc.se3_exp(np.r_[ang * a, rng.normal(size=3) * 2.0 + 0.05 * i]) for i, ang in enumerate(DESIGNED_ANGLES)]


def designed_case(orc, form, times):
    """(times, keyword arguments of orc.deskew / clone_deskewed) of a designed form"""
    if form.startswith("imu_turn"):
        it, ip = turn_track(orc, form[len("imu_turn"):])
        return times, dict(imu_times=it, imu_poses=ip, stamp=100.0)
    if form == "imu_identical":  # slerp between equal quaternions: |dot| >= 1 - eps, the linear arm
        it = imu_track(orc)[0]
        return times, dict(imu_times=it, imu_poses=[orc.se3_exp([1.5, -1.2, 1.6, 3.0, -1.0, 0.5])] * len(it), stamp=100.0)
    if form.startswith("constvel_"):  # theta2 = (dt |omega|)^2 against eps = 2.2e-16: dt |omega| against 1.49e-8, dt in [0, 0.1]
        w = float(form[len("constvel_"):])
        return times, dict(linear_vel=CONSTVEL_LINEAR, angular_vel=list(w * np.array([2.0, -1.0, 2.0]) / 3.0))
    assert form == "imu_times_descend"
    t = times.copy()
    third = len(t) // 3
    t[third:] = np.sort(t[third:])[::-1] * 0.9  # descends after the first third: no later stamp opens a table entry
    it, ip = imu_track(orc)
    return t, dict(imu_times=it, imu_poses=ip, stamp=100.0)


def test_designed_tracks_take_the_arms_they_were_designed_for(orc):
    eps = 2.220446049250313e-16
    negative = set()
    for axis, i in (("+x", 0), ("+y", 1), ("+z", 2), ("-x", 0)):
        _, poses = turn_track(orc, axis)
        arms, quats = zip(*[eigen_quat(P[:3, :3]) for P in poses])
        assert list(arms) == ["w", "w", i, i, i, i], (axis, arms)
        dots = [float(a @ b) for a, b in zip(quats[:-1], quats[1:])]
        assert all(0.9 < abs(d) < 1.0 - eps for d in dots), dots  # the trigonometric arm of the slerp
        if min(dots) < 0.0:
            negative.add(axis)
    assert negative == {"-x"}, negative  # arm i makes q[i] positive: about -x that is the other sign of the w arm's quaternion, a slerp pair with dot < 0
    _, kw = designed_case(orc, "imu_identical", None)
    _, q = eigen_quat(kw["imu_poses"][0][:3, :3])
    assert np.degrees(np.linalg.norm([1.5, -1.2, 1.6])) > 120.0 and abs(float(q @ q)) >= 1.0 - eps
    # the constant-velocity pair: every table entry on the first-order side at 1e-7 rad/s, entries on both sides at 3e-7
    assert (0.1 * 1e-7) ** 2 <= eps and (0.01 * 3e-7) ** 2 <= eps < (0.09 * 3e-7) ** 2
    t, _ = designed_case(orc, "imu_times_descend", np.sort(np.random.default_rng(0).uniform(0, 0.1, 600)))
    assert np.all(np.diff(t[:200]) >= 0) and np.all(np.diff(t[200:]) <= 0) and t[200] > t[199] + 1e-4 and t[-1] < t[199]


def exact_constvel_deskew(pts, times, Til, linear_vel, angular_vel):
    """T_lidar_imu Exp(dt [omega; v])^-1 T_imu_lidar per 0.1 ms table entry (cloud_deskewing.cpp:22-45), the exponential at 200 bits
    (tests/se3_reference.py); returns the deskewed points and, per point, dt |omega| and dt |v| of its table entry."""
    import se3_reference as sr

    table, idx = [], []
    for t in times:
        if not table or t - table[-1] > 1e-4:
            table.append(t)
        idx.append(len(table) - 1)
    xi = np.r_[angular_vel, linear_vel]
    T12 = [float(x) for x in Til[:3, :4].reshape(12)]
    TT = []
    for dt in table:
        T = sr.compose(sr.compose(sr.inverse(T12), sr.inverse(sr.Exp(dt * xi))), T12)
        TT.append(np.array(sr.to_double(T)).reshape(3, 4))
    TT, idx, table = np.array(TT), np.array(idx), np.array(table)
    out = np.einsum("nij,nj->ni", TT[idx][:, :, :3], pts) + TT[idx][:, :, 3]
    return out, table[idx] * np.linalg.norm(angular_vel), table[idx] * np.linalg.norm(linear_vel)


def constvel_tolerance(theta, dist):
    """How far gtsam::Pose3::Expmap, which the reference calls and the oracle restates bit for bit, may be from the exponential, per point:
    1e-11 (the file's bound on FP64 rounding at these ranges) plus what its translation loses by construction --
    theta^2 <= eps: t = v instead of V(omega) v = v + omega x v / 2 + ..., at most theta |v| / 2 (+ theta^2 |v| / 6, below 1e-11 here);
    otherwise t = (c - R c + omega (omega . v)) / theta^2 with c = omega x v: c and R c carry 2 and 3 roundings of size eps theta |v| and
    cancel to theta^2 |v|, so the quotient is within 8 eps |v| / theta (5 from the two products, the rest for the subtraction and the sum)."""
    eps = 2.220446049250313e-16
    first_order = theta * theta <= eps
    return 1e-11 + dist * np.where(first_order, theta / 2.0, 8.0 * eps / np.maximum(theta, 1e-300))


def assert_oracle_is_right(orc, form, pts, times, Til, kw, want):
    if "imu_times" in kw:
        ref, _ = scipy_deskew_imu(orc, pts, times, Til, kw["imu_times"], kw["imu_poses"], kw["stamp"])
        err = np.abs(want - ref).max()
        print(f"{form}: oracle against the scipy restatement, max |difference| = {err:.2e}")
        assert err <= 1e-11, (form, err)
    else:
        ref, theta, dist = exact_constvel_deskew(pts, times, Til, kw["linear_vel"], kw["angular_vel"])
        err = np.linalg.norm(want - ref, axis=1)
        tol = constvel_tolerance(theta, dist)
        print(f"{form}: oracle against the 200-bit exponential, max |difference| = {err.max():.2e}, max difference / tolerance = {(err / tol).max():.2e}, "
              f"first-order entries {np.mean(theta * theta <= 2.220446049250313e-16):.2f}")
        assert np.all(err <= tol), (form, float((err / tol).max()))


def test_oracle_zero_velocity_is_identity(orc):
    pts, times = make_case()
    Til = orc.se3_exp([0.1, -0.2, 0.05, 0.3, 0.1, -0.2])
    np.testing.assert_allclose(orc.deskew(pts, times, Til), pts, atol=1e-12)
    # no IMU poses -> the IMU form falls back to zero velocity (cloud_deskewing.cpp:66-68)
    np.testing.assert_allclose(orc.deskew(pts, times, Til, imu_times=[], imu_poses=[]), pts, atol=1e-12)


def test_oracle_constant_velocity_closed_form(orc):
    """Pure translation velocity v in the IMU frame, identity extrinsic: T_lidar0_lidar1 = Exp(dt v)^-1 => p - dt v."""
    pts, times = make_case()
    v = np.array([3.0, -1.0, 0.5])
    out = orc.deskew(pts, times, np.eye(4), linear_vel=v, angular_vel=[0, 0, 0])
    # time is quantised to the 0.1 ms table
    table, q = [], []
    for t in times:
        if not table or t - table[-1] > 1e-4:
            table.append(t)
        q.append(table[-1])
    np.testing.assert_allclose(out, pts - np.array(q)[:, None] * v[None, :], atol=1e-12)
    # pure rotation about z: points rotate by -w dt
    w = np.array([0.0, 0.0, 2.0])
    out = orc.deskew(pts, times, np.eye(4), linear_vel=[0, 0, 0], angular_vel=w)
    ang = -np.array(q) * 2.0
    ref = np.stack([np.cos(ang) * pts[:, 0] - np.sin(ang) * pts[:, 1], np.sin(ang) * pts[:, 0] + np.cos(ang) * pts[:, 1], pts[:, 2]], 1)
    np.testing.assert_allclose(out, ref, atol=1e-11)


def test_oracle_imu_form_matches_scipy_restatement(orc):
    pts, times = make_case(3)
    Til = orc.se3_exp([0.05, 0.02, -0.1, 0.2, -0.1, 0.05])
    imu_times, poses = imu_track(orc)
    out = orc.deskew(pts, times, Til, imu_times=imu_times, imu_poses=poses, stamp=100.0)
    ref, table_size = scipy_deskew_imu(orc, pts, times, Til, imu_times, poses, 100.0)
    assert 300 < table_size < 1100
    np.testing.assert_allclose(out, ref, atol=1e-11)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["imu", "constvel", "zero"] + DESIGNED_FORMS)
def test_hip_deskew_matches_oracle(orc, form):
    from glim_amd import api

    ctx = api.Context(0, 1)
    pts, times = make_case(5, n=600 if form in DESIGNED_FORMS else 131072)
    Til = orc.se3_exp([0.05, 0.02, -0.1, 0.2, -0.1, 0.05])
    if form in DESIGNED_FORMS:
        times, kw = designed_case(orc, form, times)
    elif form == "imu":
        imu_times, poses = imu_track(orc)
        kw = dict(imu_times=imu_times, imu_poses=poses, stamp=100.0)
    elif form == "constvel":
        kw = dict(linear_vel=[4.0, -2.0, 0.3], angular_vel=[0.1, -0.2, 1.5])
    else:
        kw = {}
    ref = orc.deskew(pts, times, Til, **kw)
    g = api.PointCloudGPU.clone_deskewed(pts, times, Til, ctx=ctx, **kw)
    assert g.size() == len(pts)
    xyz, _, _ = g.download(covs=False, normals=False)
    # FP64 transform on the device, stored as FP32: within one FP32 ulp of the oracle's FP64 result
    ref32 = ref.astype(np.float32)
    ulp = np.spacing(np.abs(ref32))
    assert np.all(np.abs(xyz.astype(np.float64) - ref) <= ulp.astype(np.float64))
    assert (xyz == ref32).mean() > 0.9999  # separate roundings on both sides (no FMA contraction): equal bar host-side table differences
    if form == "zero":
        np.testing.assert_array_equal(xyz, pts.astype(np.float32))
    # the deskewed cloud feeds the rest of the path: kNN + covariances + voxel map + factor run on it
    g.find_neighbors(10, download=False)
    g.estimate_covariances(10)
    assert api.GaussianVoxelMapGPU(0.5, ctx=ctx).insert(g).voxelmap_info()["num_voxels"] > 100
    empty = api.PointCloudGPU.clone_deskewed(np.zeros((0, 3)), np.zeros(0), Til, ctx=ctx)
    assert empty.size() == 0


@pytest.mark.parametrize("form", ["constvel", "constvel_still", "imu", "imu_short"] + DESIGNED_FORMS)
def test_library_deskew_table_reproduces_the_oracle_bit_for_bit(orc, form):
    """Host logic of glim_amd/csrc/deskew.hip (no device needed): the time table and the per-entry transforms the deskewing kernel gathers from,
    applied here with numpy in the kernel's operation order (three 4-term sums, separate roundings), give the oracle's -- hence the compiled
    reference's (tests/test_ref.py) -- FP64 deskewed points bit for bit, and so does the IMU-frame step on top."""
    import ctypes as C

    from glim_amd import _lib

    rng = np.random.default_rng(12)
    n = 5000
    pts = rng.uniform(-40, 40, (n, 3)).astype(np.float32).astype(np.float64)
    times = np.sort(rng.uniform(0, 0.1, n))
    times[200:260] = times[200]
    Til = orc.se3_exp([0.3, -0.2, 0.4, 0.5, -0.3, 1.2])
    it = 100.0 + np.sort(rng.uniform(-0.05, 0.15, 9))
    ip = [orc.se3_exp(rng.normal(size=6))]
    for _ in it[1:]:
        ip.append(ip[-1] @ orc.se3_exp(rng.normal(size=6) * 0.05))
    if form in DESIGNED_FORMS:
        times, kw = designed_case(orc, form, times)
    else:
        kw = {"constvel": dict(linear_vel=[4.0, -2.0, 0.3], angular_vel=[0.1, -0.2, 1.5]), "constvel_still": dict(linear_vel=[0.5, 0, 0], angular_vel=[0, 0, 0]),
              "imu": dict(imu_times=it, imu_poses=ip, stamp=100.0), "imu_short": dict(imu_times=it[:1], imu_poses=ip[:1], stamp=100.0)}[form]
    want = orc.deskew(pts, times, Til, **kw)
    if form in DESIGNED_FORMS:
        assert_oracle_is_right(orc, form, pts, times, Til, kw, want)
    L = _lib.lib()
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    T12 = np.ascontiguousarray(Til[:3, :4].reshape(12))
    if "imu_times" in kw:
        imu_t = np.ascontiguousarray(kw["imu_times"], dtype=np.float64)
        imu_p = np.ascontiguousarray(np.stack([P[:3, :4].reshape(12) for P in kw["imu_poses"]]))
        n_imu, lv, av = len(imu_t), None, None
    else:
        imu_t = imu_p = None
        n_imu, lv, av = 0, np.array(kw["linear_vel"], dtype=np.float64), np.array(kw["angular_vel"], dtype=np.float64)
    entry = np.zeros(n, dtype=np.int32)
    table = np.zeros((n, 12))
    size = C.c_int32()
    rc = L.glim_amd_debug_deskew_table(n, dp(times), dp(T12), n_imu, dp(imu_t), dp(imu_p), float(kw.get("stamp", 0.0)), dp(lv), dp(av),
                                       entry.ctypes.data_as(C.POINTER(C.c_int32)), dp(table), n, C.byref(size))
    assert rc == 0 and 0 < size.value <= n

    def apply(T, p):  # Isometry3d * Vector4d in the kernel's order
        return np.stack([((T[:, 4 * r] * p[:, 0] + T[:, 4 * r + 1] * p[:, 1]) + T[:, 4 * r + 2] * p[:, 2]) + T[:, 4 * r + 3] * 1.0 for r in range(3)], axis=1)

    got = apply(table[entry], pts)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(apply(np.tile(T12, (n, 1)), got), orc.transform_points(Til, want))
