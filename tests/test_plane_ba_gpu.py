"""Plane / edge bundle-adjustment factors and ball selection on the device (glim_amd/csrc/plane_ba.hip) against the NumPy restatement
(tests/plane_ba_restatement.py, whose docstring derives every gate used here).

Scene: 4 clouds of 1, 257, 1000 and 0 points from a 2 cm slab through the centre plus clutter, poses with translations of order 20 m; r = 1
selects 553 points (1 / 113 / 439 / 0).  Figures of this scene, measured on the CPU (the gates are computed by the tests, these are the
values they came to):
  eigen-solver   oracle.eigen3 on the three covariances (the ball's; the plane factor's; the rod-shaped factor's): residual
                 |C u - lambda u| / |C| and orthonormality defect at most 7.2e-14 (the rod, whose two small eigenvalues nearly coincide; 2.2e-16
                 and 3.8e-16 on the other two); gate 8 x that = 5.8e-13.  The device's solver measured 2.2e-16 / 3.8e-16 / 7.2e-14 (residual) and
                 2.2e-16 / 2.2e-16 / 1.4e-14 (orthonormality).
  plane factor   restatement with eigh against restatement with oracle.eigen3: 2.0e-16 in g, 7.0e-17 in H (relative to the size of the
                 terms, see the restatement's docstring); share of the sums 6.9e-12; gates 6.9e-12 (g and H), condition
                 lambda_2 / (lambda_1 - lambda_0) = 1.14.  At the moved poses: gates 7.2e-11, condition 2.66.  Device minus restatement:
                 g 1.8e-13, H 7.9e-16 (creation poses); g 2.4e-14, H 4.4e-15 (moved); cost 1.2e-17 / 1.9e-16.
  edge factor    (rod-shaped scene, 982 points) solver 1.7e-14 in g, 1.4e-15 in H; share of the sums 6.8e-12; gates 7.0e-12 (g), 6.8e-12 (H),
                 condition lambda_2 / (lambda_2 - lambda_1) = 1.0003; moved poses: gates 5.5e-11.  Device minus restatement: g 2.6e-12,
                 H 2.4e-15 (creation poses); g 1.6e-14, H 7.4e-15 (moved).
  shapes         (test_factor_shapes) gates 6.5e-13 .. 1.7e-11; device g <= 4.7e-13, H <= 2.1e-15.
One run on an MI355X.
"""
import numpy as np
import pytest

import plane_ba_restatement as R

pytestmark = pytest.mark.gpu

RADIUS = 1.0


@pytest.fixture(scope="module")
def ctx():
    from glim_amd import api

    return api.Context(0, 1)


def _upload(api, ctx, clouds):
    out = []
    for s, p in enumerate(clouds):
        if s == 2:  # the FP32 cloud: its points are widened on the device
            out.append(api.PointCloudGPU.clone(p.astype(np.float32), ctx=ctx))
        else:
            out.append(api.clone_exact(p, ctx=ctx))
    return out


@pytest.fixture(scope="module")
def scene(ctx):
    from glim_amd import api

    clouds, poses = R.make_scene()
    pairs, q = R.select(clouds, poses, R.CENTER, RADIUS)
    return {"clouds": clouds, "poses": poses, "gpu": _upload(api, ctx, clouds), "pairs": pairs, "q": q}


@pytest.fixture(scope="module")
def line_scene(ctx):
    from glim_amd import api

    clouds, poses = R.make_scene(line=True)
    pairs, q = R.select(clouds, poses, R.CENTER, RADIUS)
    return {"clouds": clouds, "poses": poses, "gpu": _upload(api, ctx, clouds), "pairs": pairs, "q": q}


def _frames(sc):
    kept = sorted(set(sc["pairs"][:, 0].tolist()))
    return kept, [sc["clouds"][s][sc["pairs"][sc["pairs"][:, 0] == s, 1]] for s in kept]


def test_selection_equals_the_restatement_and_the_boundary_point_is_out(scene):
    from glim_amd import api

    pairs, count = api.ba_ball_select(scene["gpu"], scene["poses"], R.CENTER, RADIUS)
    assert count == len(scene["pairs"])
    np.testing.assert_array_equal(pairs, scene["pairs"])
    # cloud 1's point 0 is CENTER + (1, 0, 0) under the identity: q.q == r r exactly, and the comparison is strict
    q = R.transform(scene["clouds"][1][:1], scene["poses"][1], R.CENTER)
    assert R.sqnorm(q)[0] == RADIUS * RADIUS
    assert not ((pairs[:, 0] == 1) & (pairs[:, 1] == 0)).any()
    # a capacity below the count: the true count and the prefix
    part, count2 = api.ba_ball_select(scene["gpu"], scene["poses"], R.CENTER, RADIUS, capacity=100)
    assert count2 == count and len(part) == 100
    np.testing.assert_array_equal(part, scene["pairs"][:100])
    none, count3 = api.ba_ball_select(scene["gpu"], scene["poses"], R.CENTER, RADIUS, capacity=0)
    assert count3 == count and len(none) == 0


def test_sums_are_within_the_two_order_bound_and_repeat_bit_for_bit(scene):
    from glim_amd import api

    a = api.ba_ball_stats(scene["gpu"], scene["poses"], R.CENTER, RADIUS)
    b = api.ba_ball_stats(scene["gpu"], scene["poses"], R.CENTER, RADIUS)
    n, s, S = R.sums(scene["q"])
    bs, bS = R.sum_bounds(scene["q"])
    print("sum differences", np.abs(a["sum"] - s), "bounds", bs, "\ncross differences", np.abs(a["sum_cross"] - S).max(), "bound", bS.min())
    assert a["num_points"] == n
    assert (np.abs(a["sum"] - s) <= bs).all()
    assert (np.abs(a["sum_cross"] - S) <= bS).all()
    for k in ("sum", "sum_cross", "eigenvalues"):
        assert a[k].tobytes() == b[k].tobytes(), k


def _solver_quality(C, lam, V):
    """(residual |C u - lambda u| / |C|, orthonormality defect); V columns = eigenvectors"""
    return np.abs(C @ V - V * lam).max() / np.abs(C).max(), np.abs(V.T @ V - np.eye(3)).max()


def _solver_gate(orc, covs):
    worst = 0.0
    for C in covs:
        lam, V = orc.eigen3(C)
        worst = max(worst, *_solver_quality(C, lam, V))
    return worst, 8 * worst


def _moment_covariance(mom, poses):
    """the covariance from the factor's moments, as glim_amd.h states it (about tau of frame 0)"""
    tau0 = poses[0][:3, :3] @ mom[0, 1:4] + poses[0][:3, 3]
    sq, sqq, N = np.zeros(3), np.zeros((3, 3)), 0.0
    for m, T in zip(mom, poses):
        Rm, n, c, v = T[:3, :3], m[0], m[1:4], m[4:7]
        P = np.array([[m[7], m[8], m[9]], [m[8], m[10], m[11]], [m[9], m[11], m[12]]])
        tau = Rm @ c + T[:3, 3] - tau0
        sq += Rm @ v + n * tau
        sqq += Rm @ P @ Rm.T + np.outer(Rm @ v, tau) + np.outer(tau, Rm @ v) + n * np.outer(tau, tau)
        N += n
    mean = sq / N
    return sqq / N - np.outer(mean, mean)


def test_eigenvalues_of_the_ball_and_eigenpairs_of_the_factor(scene, line_scene, ctx, orc):
    from glim_amd import api

    st = api.ba_ball_stats(scene["gpu"], scene["poses"], R.CENTER, RADIUS)
    C_ball = R.covariance(st["num_points"], st["sum"], st["sum_cross"])  # teacher-forced: the device's own sums
    covs = [C_ball]
    for sc in (scene, line_scene):
        f = api.PlaneEVMFactor.from_ball(sc["gpu"], sc["poses"], R.CENTER, RADIUS)
        kept = f.frames()
        covs.append(_moment_covariance(f.moments(), [sc["poses"][s] for s in kept]))
        f.close()
    worst, gate = _solver_gate(orc, covs)
    print("oracle.eigen3 on the scene's covariances: worst", worst, "gate", gate)
    # the ball: eigenvalues only.  |lambda_device - lambda_oracle| <= gate |C| follows from both residuals being within the gate
    lam_o, _ = orc.eigen3(C_ball)
    print("ball eigenvalues: device", st["eigenvalues"], "oracle", lam_o)
    assert np.abs(st["eigenvalues"] - lam_o).max() <= 2 * gate * np.abs(C_ball).max()
    assert (np.diff(st["eigenvalues"]) >= 0).all()
    lam, U = api.ba_debug_eigen3(np.array(covs), ctx=ctx)
    for C, l, u in zip(covs, lam, U):
        res, orth = _solver_quality(C, l, u.T)
        print("device solver: residual", res, "orthonormality", orth)
        assert res <= gate and orth <= gate
        assert (np.diff(l) >= 0).all()


PARAM_SETS = {  # (min_radius, max_radius, plane_eps) -> the stop each forces on this scene from r0 = 1
    "range": (0.3, 5.0, 1e-6),
    "few_points": (0.01, 5.0, 1e-6),
    "plane_eps": (0.1, 5.0, 0.03),
    "trials": (0.1, 5.0, 0.5),
}


@pytest.mark.parametrize("stop", list(PARAM_SETS))
def test_auto_radius_follows_the_rule(scene, stop):
    from glim_amd import api

    prm = PARAM_SETS[stop]

    def evaluate(r):
        _, q = R.select(scene["clouds"], scene["poses"], R.CENTER, r)
        if len(q) == 0:
            return 0, np.full(3, np.nan)
        return len(q), np.linalg.eigvalsh(R.covariance(*R.sums(q)))

    _, ref_stop, ref_trace = R.auto_radius(evaluate, RADIUS, *prm)
    assert ref_stop == stop  # the parameter set forces the stop it is named after
    got = api.ba_auto_radius(scene["gpu"], scene["poses"], R.CENTER, RADIUS, api.BundleAdjustmentParams(*prm), trace=True)
    plain = api.ba_auto_radius(scene["gpu"], scene["poses"], R.CENTER, RADIUS, api.BundleAdjustmentParams(*prm))
    trace = got["trace"]
    print(stop, [(t["radius"], t["count"], t["decision"]) for t in trace])
    assert sum(1 for t in trace if t["count"] >= 0) <= 11 and len(trace) <= 11
    # per-trial counts equal the restatement's
    assert [t["count"] for t in trace] == [t[1] for t in ref_trace]
    # the rule on the device's reported eigenvalues reproduces every decision and the final radius bit for bit
    table = {t["radius"]: (t["count"], t["eigenvalues"]) for t in trace}
    radius, rule_stop, rule_trace = R.auto_radius(lambda r: table[r], RADIUS, *prm)
    assert [t[3] for t in rule_trace] == [t["decision"] for t in trace]
    assert [t[0] for t in rule_trace] == [t["radius"] for t in trace]
    assert rule_stop == got["stop"] == stop
    assert np.float64(radius).tobytes() == np.float64(got["radius"]).tobytes()
    assert got["trials"] == sum(1 for t in trace[1:] if t["count"] >= 0)
    assert plain["radius"] == got["radius"] and plain["num_points"] == got["num_points"] and plain["stop"] == got["stop"]
    assert plain["eigenvalues"].tobytes() == got["eigenvalues"].tobytes()
    assert got["num_points"] == table[got["radius"]][0]


def _moved(poses, seed, size=0.05):
    from glim_amd.se3 import se3_exp

    rng = np.random.default_rng(seed)
    out = []
    for T in poses:
        xi = rng.normal(size=6)
        out.append(T @ se3_exp(size * xi / np.linalg.norm(xi)))
    return out


def _check_factor(f, frames, poses, kind, orc, planar=False):
    gates = R.factor_gates(frames, poses, kind, orc.eigen3)
    ref = R.factor(frames, poses, kind)
    got = f.linearize(poses)
    dg = np.abs(got["g"] - ref["g"]).max() / ref["g_scale"]  # plane_ba_restatement: why not relative to g itself
    dH = np.abs(got["H"] - ref["H"]).max() / ref["H_scale"]
    print(f"kind {kind}: condition {gates['condition']:.4f}, solver share g {gates['solver_g']:.2e} H {gates['solver_H']:.2e}, sums {gates['sum_share']:.2e}; "
          f"device - restatement: g {dg:.2e} (gate {gates['g']:.2e}), H {dH:.2e} (gate {gates['H']:.2e}), cost {got['cost'] - ref['cost']:.2e} (gate {gates['cost']:.2e})")
    assert gates["condition"] <= 10.0
    assert abs(got["cost"] - ref["cost"]) <= gates["cost"]
    assert dg <= gates["g"]
    assert dH <= gates["H"]
    assert np.array_equal(got["H"], got["H"].T)
    assert got["status"] == 0
    assert f.error(poses) == got["cost"]
    return got, gates


@pytest.mark.parametrize("kind", [0, 1])
def test_factor_from_the_ball_and_from_host_arrays(scene, line_scene, ctx, orc, kind):
    from glim_amd import api

    sc = scene if kind == 0 else line_scene  # the edge kind needs lambda_1 apart from lambda_2: a rod
    cls = api.PlaneEVMFactor if kind == 0 else api.EdgeEVMFactor
    kept, frames = _frames(sc)
    assert kept == [0, 1, 2]
    ball = cls.from_ball(sc["gpu"], sc["poses"], R.CENTER, RADIUS)
    assert ball.frames().tolist() == [0, 1, 2]  # the empty cloud is dropped
    assert ball.num_points() == len(sc["pairs"]) and ball.num_frames() == 3
    host = cls.from_points(np.concatenate(frames), np.concatenate([np.full(len(p), 2 * s) for s, p in enumerate(frames)]), num_frames=5, ctx=ctx)
    assert host.frames().tolist() == [0, 2, 4]
    assert ball.moments().tobytes() == host.moments().tobytes()
    mom = ball.moments()
    for s, p in enumerate(frames):
        assert mom[s, 0] == len(p) and np.array_equal(mom[s, 1:4], p[0])
    poses = [sc["poses"][s] for s in kept]
    for ps in (poses, _moved(poses, 3)):
        a, _ = _check_factor(ball, frames, ps, kind, orc)
        b = host.linearize(ps)
        assert a["H"].tobytes() == b["H"].tobytes() and a["g"].tobytes() == b["g"].tobytes() and a["cost"] == b["cost"]
    ball.close()
    host.close()


def _case(name):
    """small factors where a kernel can still go wrong: (frames, poses)"""
    from glim_amd.se3 import se3_exp

    rng = np.random.default_rng(11)

    def slab(n, spread=1.0):
        p = rng.uniform(-spread, spread, size=(n, 3))
        p[:, 2] *= 0.02
        return p

    def pose(i):
        r = np.random.default_rng(100 + i)
        return se3_exp(np.concatenate([r.normal(size=3) * 0.5, r.normal(size=3) * 20.0]))

    def local(world, T):
        return (world - T[:3, 3]) @ T[:3, :3]

    if name == "one_point_frame":
        sizes = [1, 40]
    elif name == "frame_of_257":
        sizes = [257, 5]
    elif name == "one_frame":
        sizes = [300]
    elif name == "k128_three_points_each":
        sizes = [3] * 128
    elif name == "all_points_in_one_frame_of_many":
        sizes = [600]
    elif name == "three_points":
        sizes = [1, 2]
    else:
        raise KeyError(name)
    poses = [pose(i) for i in range(len(sizes))]
    world = [np.array([5.0, -3.0, 2.0]) + slab(n) for n in sizes]
    return [local(w, T) for w, T in zip(world, poses)], poses


@pytest.mark.parametrize("name", ["one_point_frame", "frame_of_257", "one_frame", "k128_three_points_each", "all_points_in_one_frame_of_many", "three_points"])
def test_factor_shapes(ctx, orc, name):
    from glim_amd import api

    frames, poses = _case(name)
    num_frames = len(frames) + (7 if name == "all_points_in_one_frame_of_many" else 0)
    offset = 3 if name == "all_points_in_one_frame_of_many" else 0
    f = api.PlaneEVMFactor.from_points(np.concatenate(frames), np.concatenate([np.full(len(p), s + offset) for s, p in enumerate(frames)]),
                                       num_frames=num_frames, ctx=ctx)
    assert f.num_frames() == len(frames) and f.frames().tolist() == [s + offset for s in range(len(frames))]
    assert f.num_points() == sum(len(p) for p in frames)
    if name == "three_points":
        # three points span a plane: lambda_0 is zero to rounding, and the gaps are wide
        got = f.linearize(poses)
        gates = R.factor_gates(frames, poses, 0, orc.eigen3)
        print("three points: cost", got["cost"], "gate", gates["cost"])
        assert got["cost"] >= -gates["cost"] and abs(got["cost"]) <= gates["cost"]
        assert got["status"] == 0 and np.isfinite(got["H"]).all()
    else:
        _check_factor(f, frames, poses, 0, orc)
        _check_factor(f, frames, _moved(poses, 5), 0, orc)
    f.close()


def test_planar_selection_cost_and_the_degenerate_rule(ctx, orc):
    from glim_amd import _lib, api

    # a perfectly planar selection: points on z = 0 of one frame under the identity, coordinates on a binary grid
    rng = np.random.default_rng(2)
    p = np.zeros((200, 3))
    p[:, :2] = rng.integers(-64, 64, size=(200, 2)) / 64.0
    frames, poses = [p[:120], p[120:]], [np.eye(4), np.eye(4)]
    f = api.PlaneEVMFactor.from_points(np.concatenate(frames), np.concatenate([np.zeros(120), np.ones(80)]), ctx=ctx)
    got = f.linearize(poses)
    gates = R.factor_gates(frames, poses, 0, orc.eigen3)
    lam = R.factor(frames, poses, 0)["eigenvalues"]
    print("planar: cost", got["cost"], "gate", gates["cost"], "eigenvalues", lam)
    assert got["cost"] >= -gates["cost"]
    # the documented rule: a k term is dropped iff |lambda_e - lambda_k| <= 1e-12 max(lambda_2, DBL_MIN); here both gaps are wide
    assert min(lam[1] - lam[0], lam[2] - lam[0]) > 1e-6 * lam[2]
    assert got["status"] == 0 and np.isfinite(got["H"]).all() and np.array_equal(got["H"], got["H"].T)
    f.close()
    # collinear points: lambda_0 = lambda_1 = 0 to rounding, the (0, 1) term has no gap: dropped, and the bit says so
    line = np.zeros((50, 3))
    line[:, 0] = np.arange(50) / 16.0
    g = api.PlaneEVMFactor.from_points(line, np.zeros(50), ctx=ctx)
    out = g.linearize([np.eye(4)])
    assert out["status"] & _lib.BA_DEGENERATE
    assert np.isfinite(out["H"]).all() and np.isfinite(out["g"]).all()
    _, status = g.error([np.eye(4)], with_status=True)
    assert status & _lib.BA_DEGENERATE
    g.close()


def test_refusals(scene, ctx):
    from glim_amd import api

    p = np.random.default_rng(0).normal(size=(129 * 3, 3))
    with pytest.raises(api.GlimAmdError):
        api.PlaneEVMFactor.from_points(p, np.repeat(np.arange(129), 3), num_frames=129, ctx=ctx)  # K = 129
    with pytest.raises(api.GlimAmdError):
        api.PlaneEVMFactor.from_points(p[:2], [0, 1], ctx=ctx)  # N < 3
    with pytest.raises(api.GlimAmdError):
        api.PlaneEVMFactor.from_ball(scene["gpu"][:1], scene["poses"][:1], R.CENTER, RADIUS)  # one point in the ball
    with pytest.raises(api.GlimAmdError):
        api.ba_ball_stats(scene["gpu"], scene["poses"], R.CENTER, 0.0)
    with pytest.raises(api.GlimAmdError):
        api.ba_ball_select(scene["gpu"], scene["poses"], R.CENTER, RADIUS, capacity=-1)
    empty = api.ba_ball_stats(scene["gpu"][3:], scene["poses"][3:], R.CENTER, RADIUS)  # the empty cloud alone
    assert empty["num_points"] == 0 and not empty["sum"].any() and np.isnan(empty["eigenvalues"]).all()


@pytest.mark.parametrize("kind", [0, 1])
def test_drop_in_blocks_are_the_linearization_byte_for_byte(scene, ctx, tmp_path_factory, kind):
    """a C++ program over the drop-in header adds the same points key by key, linearises over gtsam::Values and writes the HessianFactor's
    blocks: G = H, g = -gradient, f = 2 cost, the bytes of glim_amd_ba_factor_linearize"""
    import subprocess

    from glim_amd import api

    tmp = tmp_path_factory.mktemp("plane_ba_drop_in")
    exe = R.build_drop_in(tmp)
    kept, frames = _frames(scene)
    poses = _moved([scene["poses"][s] for s in kept], 9)
    R.write_problem(str(tmp / "in.txt"), frames, poses, kind)
    res = subprocess.run([exe, str(tmp / "in.txt"), str(tmp / "out.txt")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "OK" in res.stdout, res.stdout + res.stderr
    v = np.array([float(x) for x in open(tmp / "out.txt").read().split()])
    K = len(frames)
    cls = api.PlaneEVMFactor if kind == 0 else api.EdgeEVMFactor
    f = cls.from_points(np.concatenate(frames), np.concatenate([np.full(len(p), s) for s, p in enumerate(frames)]), ctx=ctx)
    ref = f.linearize(poses)
    f.close()
    assert v[0] == 2.0 * ref["cost"]
    assert (-v[1 : 1 + 6 * K]).tobytes() == ref["g"].tobytes()
    blocks = v[1 + 6 * K :].reshape(-1, 6, 6)
    assert len(blocks) == K * (K + 1) // 2
    b = 0
    for i in range(K):
        for j in range(i, K):
            assert blocks[b].tobytes() == np.ascontiguousarray(ref["H"][6 * i : 6 * i + 6, 6 * j : 6 * j + 6]).tobytes(), (i, j)
            b += 1
