"""The GICP search index against brute force on adversarial clouds (tests/gicp_search_cases.py): every GICP-family path -- the rigid factor,
the continuous-time factor, the batched LM registration -- takes its correspondences from nearest() in glim_amd/csrc/gicp.hip, which claims an
exact search: smallest FP64 (dx^2 + dy^2) + dz^2, ties to the smaller original index, valid iff d^2 <= max_d^2, a radius beyond the bounded ring
walk refused.  The un-marked tests check the cases themselves (ties, inlier shares, cell-edge regimes, the two references against each other);
the gpu tests hold the device to the references index by index.

The ring limit: include/glim_amd.h promises every distance up to 21 x hint.  With hint = 0.9 and a dense target (h = hint / 3.0), d = 21 * 0.9
gives d / h = 63.00000000000001; rings() used to take ceil(d / h) + 1 = 65 > 64 and refuse it (test_cell_edge_regimes_and_the_ring_limit
restates that count; test_ring_limit[blob] is the device case)."""
import functools

import numpy as np
import pytest

import gicp_search_cases as gsc

ERROR_RTOL = 2e-4  # tests/test_gicp.py: a device error against the FP64 value


# ---- references, computed once --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_cases():
    return gsc.exact_cases()


@functools.lru_cache(maxsize=None)
def exact_ref(name, pose, max_d):
    """-> (source, corr, multiplicity, d2) of a family-1 run (the index's hint does not enter the answer)"""
    case = exact_cases()[name]
    src = gsc.exact_source(name, case, pose)
    return (src,) + gsc.brute_force(case["target"], gsc.transform(gsc.EXACT_POSES[pose], src), max_d)


def general_pose(orc):
    return orc.se3_exp(gsc.GENERAL_XI)


_GENERAL = {}


def general_ref(orc, name, max_d):
    """-> (target, source, oracle correspondences, brute-force correspondences, d2) of a family-2 run"""
    if (name, max_d) not in _GENERAL:
        T = general_pose(orc)
        target, src = gsc.general_case(name, max_d, T)
        L = orc.gicp_linearize(target, gsc.eye_covs(len(target)), src, gsc.eye_covs(len(src)), T, max_d, want_corr=True)
        corr, _, d2 = gsc.brute_force(target, gsc.transform(T, src), max_d)
        _GENERAL[(name, max_d)] = (target, src, L["corr"], corr, d2)
    return _GENERAL[(name, max_d)]


@functools.lru_cache(maxsize=None)
def ring_case(name):
    target = gsc.general_targets()[name]
    src = gsc.ring_limit_source(target, seed=40 + ["blob", "plane", "line"].index(name))
    return (target, src) + gsc.brute_force(target, src, gsc.RING_D)


# ---- the cases themselves (CPU) -------------------------------------------------------------------------------------------------------------
def test_brute_force_on_answers_known_by_hand():
    target, source, max_d, expected = gsc.radius_case()
    corr, mult, d2 = gsc.brute_force(target, source, max_d)
    np.testing.assert_array_equal(corr, expected)
    assert d2[0] == d2[1] == max_d * max_d and d2[2] > max_d * max_d and d2[3] > max_d * max_d  # two at the radius exactly, two beyond
    assert d2[3] - max_d * max_d < 1e-6  # ... one of them by an FP32 ulp of the coordinate
    # ties go to the smaller index whatever the order of the points; non-finite points are never matched and shift no index
    t = np.array([[np.nan, 0, 0], [1.0, 0, 0], [np.inf, 0, 0], [-1.0, 0, 0], [1.0, 0, 0]])
    corr, mult, _ = gsc.brute_force(t, np.array([[0.0, 0, 0], [0.75, 0, 0], [np.nan, 0, 0], [0.0, 5.0, 0]]), 2.0)
    np.testing.assert_array_equal(corr, [1, 1, -1, -1])
    np.testing.assert_array_equal(mult, [3, 2, 0, 3])
    corr, mult, _ = gsc.brute_force(gsc.nonfinite_target(), np.zeros((3, 3)), 1.0)
    assert np.all(corr == -1) and np.all(mult == 0)


def test_exact_cases_are_exact_and_hold_what_they_are_for():
    cases = exact_cases()
    for name, c in cases.items():
        src = np.delete(c["source"], 3, axis=0) if name == "radius" else c["source"]  # (10, 0, 0.7500001): the FP32 ulp beyond the radius
        assert gsc.is_exact(c["target"]) and gsc.is_exact(src), name
        for pose in c["poses"]:
            assert gsc.is_exact(gsc.transform(gsc.EXACT_POSES[pose], gsc.exact_source(name, c, pose))) or name == "radius", (name, pose)
    # lattice: ties of every multiplicity at the identity pose, a radius that cuts between the tie classes, points exactly at the radius
    _, corr, mult, d2 = exact_ref("lattice", "identity", 1.0)
    hist = {m: int((mult == m).sum()) for m in (1, 2, 4, 8)}
    print("lattice tie histogram (identity):", hist)
    assert all(v >= 40 for v in hist.values()) and sum(hist.values()) == 256
    inliers = [int((exact_ref("lattice", "identity", d)[1] >= 0).sum()) for d in gsc.LATTICE_MAX_D]
    assert inliers == [256, 256, 192, 128], inliers
    assert (d2 == 0.25 * 0.25).sum() == 64  # the edge midpoints: AT the radius 0.25
    _, corr, mult, _ = exact_ref("lattice", "rz90", 1.0)
    print("lattice tie histogram (rz90):", {int(m): int((mult == m).sum()) for m in np.unique(mult)})
    assert (mult > 1).sum() >= 40 and (mult == 1).sum() >= 40
    for hint in gsc.LATTICE_HINTS:
        assert gsc.cell_edge(cases["lattice"]["target"], hint)[0] == hint  # 0.5: every lattice point lies on a cell face
    # duplicates: the queries at the pile tie 300 ways and take the pile's smallest index, which is not the cloud's
    for pose in ("identity", "rz90"):
        _, corr, mult, _ = exact_ref("duplicates", pose, 0.25)
        assert (mult[:128] == 300).sum() >= 100 and np.all(corr[:128][mult[:128] == 300] == gsc.PILE_FIRST) and 0 < (corr[128:] >= 0).sum() < 128
        _, corr, mult, _ = exact_ref("identical", pose, 1.0)
        assert np.all(mult == 1000) and set(corr) == {0, -1} and 10 < (corr == 0).sum() < 60
        _, corr, mult, _ = exact_ref("n2", pose, 1.0)
        assert (mult == 2).sum() >= 8 and {0, 1, -1} <= set(corr)
        assert {0, -1} == set(exact_ref("n1", pose, 1.0)[1])
        src, corr, mult, _ = exact_ref("broken", pose, 0.25)
        finite = np.isfinite(cases["broken"]["target"]).all(axis=1)
        assert finite.sum() == 32 and not finite[0] and np.all(finite[corr[corr >= 0]]) and (corr >= 0).sum() > 20 and (mult > 1).sum() > 5
        assert np.all(corr[~np.isfinite(src).all(axis=1)] == -1) and (~np.isfinite(src).all(axis=1)).sum() == 4
        assert np.all(exact_ref("nonfinite", pose, 1.0)[1] == -1)


@pytest.mark.parametrize("name", list(gsc.exact_cases()))
def test_oracle_agrees_with_brute_force_on_exact_data(orc, name):
    c = exact_cases()[name]
    for pose in c["poses"]:
        for max_d in c["max_ds"]:
            src, corr, _, d2 = exact_ref(name, pose, max_d)
            L = orc.gicp_linearize(c["target"], gsc.eye_covs(len(c["target"])), src, gsc.eye_covs(len(src)), gsc.EXACT_POSES[pose], max_d, want_corr=True)
            np.testing.assert_array_equal(L["corr"], corr, err_msg=f"{name} {pose} {max_d}")
            assert L["num_inliers"] == (corr >= 0).sum()
            np.testing.assert_allclose(L["error"], gsc.half_sum_d2(corr, d2), rtol=1e-12)  # identity covariances: M = I / 2


@pytest.mark.parametrize("name,max_d", gsc.general_runs())
def test_the_two_references_agree_at_a_general_pose(orc, name, max_d):
    target, src, corr_oracle, corr_brute, _ = general_ref(orc, name, max_d)
    np.testing.assert_array_equal(corr_oracle, corr_brute)
    share = (corr_brute >= 0).mean()
    print(f"{name} max_d {max_d}: inlier share {share:.3f}, distinct matches {len(set(corr_brute[corr_brute >= 0]))}")
    assert 0.05 < share < 0.995


def test_cell_edge_regimes_and_the_ring_limit():
    targets = gsc.general_targets()
    edge = lambda name, hint: gsc.cell_edge(targets[name], hint)[0]
    for hint in (1.0, gsc.RING_HINT):
        assert edge("blob", hint) == hint / 3.0  # volumetric: clamped below
        assert hint / 3.0 < edge("plane", hint) < hint  # between the clamps
    assert 0.25 / 3.0 < edge("blob", 0.25) < 0.25 and edge("plane", 0.25) == 0.25
    for hint in (0.25, 1.0, gsc.RING_HINT):
        assert edge("line", hint) == hint  # degenerate area estimate: clamped above
    for hint, want_bits in ((0.01, 60), (0.05, 51)):  # +-2990 m in cells of the hint: 20 key bits per axis at 0.01 (a 61-bit sort), all inside the grid
        h, ok = gsc.cell_edge(targets["clusters"], hint)
        bits = [int(e).bit_length() for e in np.ptp(np.floor(targets["clusters"] / h), axis=0)]
        print(f"clusters hint {hint}: h {h:.6g}, key bits {bits}")
        assert ok.all() and sum(bits) >= want_bits
    # the documented limit, 21 x hint, for sixteen hints and the densest target (h = hint / 3.0): only 0.9 makes d / h exceed 63
    hints = [0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.4, 0.5, 0.6, 0.75, 0.9, 1.0, 1.5, 2.0, 2.5, 3.0]
    over = [hint for hint in hints if np.ceil(21 * hint / (hint / 3.0)) + 1.0 > gsc.MAX_RING]  # the count rings() used to take
    assert over == [0.9] and 21 * 0.9 / (0.9 / 3.0) == 63.00000000000001
    for hint in hints:
        for h in (hint / 3.0, hint / 2.0, hint):
            assert np.ceil(21 * hint / h) <= gsc.rings_needed(21 * hint, h) <= gsc.MAX_RING  # accepted, and no fewer rings than the radius spans
            assert gsc.rings_needed(64 * hint, h) > gsc.MAX_RING  # refused
    # the ring-limit queries: half just inside 21 x 0.9 of their nearest target point, half just outside
    for name in ("blob", "plane", "line"):
        target, src, corr, _, d2 = ring_case(name)
        d = np.sqrt(d2)
        h = gsc.cell_edge(target, gsc.RING_HINT)[0]
        print(f"ring limit {name}: h {h:.6g}, d / h {gsc.RING_D / h!r}, rings {gsc.rings_needed(gsc.RING_D, h)}, |d - limit| {np.abs(d - gsc.RING_D).min():.2e} .. {np.abs(d - gsc.RING_D).max():.2e}")
        assert (corr[:32] >= 0).all() and (corr[32:] == -1).all() and np.abs(d - gsc.RING_D).max() < 2 * gsc.RING_EPS and np.abs(d - gsc.RING_D).min() > gsc.RING_EPS / 2
    assert gsc.RING_D / edge("blob", gsc.RING_HINT) == 63.00000000000001  # the case rings() used to refuse
    # out of the grid: half of the target has no cell at h = 0.001; the queries around those points find nothing, the others are untouched
    target, src, max_d = gsc.out_of_grid_case()
    h, ok = gsc.cell_edge(target, gsc.OUT_HINT)
    assert h == gsc.OUT_HINT and ok.sum() == 512 and np.all((np.abs(target) > 1048.576).any(axis=1) == ~ok)
    corr_all = gsc.brute_force(target, src, max_d)[0]
    corr = gsc.brute_force(target, src, max_d, usable=ok)[0]
    near = ok[np.where(corr_all >= 0, corr_all, 0)] & (corr_all >= 0)
    assert np.array_equal(corr[near], corr_all[near]) and np.all(corr[~near] == -1) and near.sum() > 50 and (~ok[corr_all[corr_all >= 0]]).sum() > 50


# ---- the device -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from glim_amd import api

    return api.Context(0, 1)


def upload(ctx, points):
    from glim_amd import api

    return api.PointCloudGPU.clone(np.asarray(points, dtype=np.float64), covs=gsc.eye_covs(len(points)), ctx=ctx)


def check_rigid(f, values, corr, d2, what):
    """correspondences index by index; the counts of linearize() and error(); the error itself (identity covariances: 0.5 sum d^2)"""
    np.testing.assert_array_equal(f.correspondences(values), corr, err_msg=what)
    n, want = int((corr >= 0).sum()), gsc.half_sum_d2(corr, d2)
    L = f.linearize(values)
    assert L["num_inliers"] == n, what
    np.testing.assert_allclose(L["error"], want, rtol=ERROR_RTOL, err_msg=what)
    e = f.error(values)
    assert f._inliers == n, what
    np.testing.assert_allclose(e, want, rtol=ERROR_RTOL, err_msg=what)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(gsc.exact_cases()))
def test_rigid_factor_on_exact_data(ctx, name):
    from glim_amd import api

    c = exact_cases()[name]
    tg = upload(ctx, c["target"])
    for pose in c["poses"]:
        T = gsc.EXACT_POSES[pose]
        sg = upload(ctx, gsc.exact_source(name, c, pose))
        for hint in c["hints"]:
            for max_d in c["max_ds"]:
                _, corr, _, d2 = exact_ref(name, pose, max_d)
                f = api.IntegratedGICPFactor(np.eye(4), 1, tg, sg, max_correspondence_distance=max_d if hint is None else hint)
                f.set_max_correspondence_distance(max_d)
                check_rigid(f, {1: T}, corr, d2, f"{name} {pose} hint {hint} max_d {max_d}")
                f.close()
        sg.close()
    tg.close()


@pytest.mark.gpu
def test_rigid_factor_binary_form(ctx):
    from glim_amd import api

    c = exact_cases()["lattice"]
    tg, sg = upload(ctx, c["target"]), upload(ctx, c["source"])
    _, corr, _, d2 = exact_ref("lattice", "rz90", 0.5)
    f = api.IntegratedGICPFactor(0, 1, tg, sg, max_correspondence_distance=0.5)
    check_rigid(f, {0: np.eye(4), 1: gsc.RZ90}, corr, d2, "lattice rz90 binary")
    # the same relative pose from two moved keys (exact: both are signed permutations with dyadic translations)
    check_rigid(f, {0: gsc.exact_inverse(gsc.RZ90), 1: np.eye(4)}, corr, d2, "lattice rz90 binary, moved target")
    f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,max_d", gsc.general_runs())
def test_rigid_factor_at_a_general_pose(orc, ctx, name, max_d):
    from glim_amd import api

    target, src, corr, corr_brute, d2 = general_ref(orc, name, max_d)
    np.testing.assert_array_equal(corr, corr_brute)
    tg, sg = upload(ctx, target), upload(ctx, src)
    f = api.IntegratedGICPFactor(np.eye(4), 1, tg, sg, max_correspondence_distance=max_d)
    check_rigid(f, {1: general_pose(orc)}, corr, d2, f"{name} max_d {max_d}")
    f.close()


@pytest.mark.gpu
def test_shared_index_gives_the_same_bytes_at_every_distance(ctx):
    """one index (hint 0.5), borrowed by a factor per distance from 0 to 5 x the hint, up and then down"""
    from glim_amd import api

    c = exact_cases()["lattice"]
    tg, sg = upload(ctx, c["target"]), upload(ctx, c["source"])
    owner = api.IntegratedGICPFactor(np.eye(4), 1, tg, sg, max_correspondence_distance=0.5)
    up = [0.0, 0.25, 0.433, 0.5, 1.0, 2.5]
    seen = {}
    for max_d in up + up[::-1]:
        f = api.IntegratedGICPFactor(np.eye(4), 1, tg, sg, target_tree=owner.target_tree, max_correspondence_distance=max_d)
        got = f.correspondences({1: gsc.RZ90})
        f.close()
        corr = gsc.brute_force(c["target"], gsc.transform(gsc.RZ90, c["source"]), max_d)[0]
        np.testing.assert_array_equal(got, corr, err_msg=f"max_d {max_d}")
        assert seen.setdefault(max_d, got.tobytes()) == got.tobytes(), max_d
    assert 0 < (np.frombuffer(seen[0.0], dtype=np.int32) >= 0).sum() < (np.frombuffer(seen[0.25], dtype=np.int32) >= 0).sum() < 256
    owner.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["blob", "plane", "line"])
def test_ring_limit(ctx, name):
    """an index built with hint 0.9 answers at 21 x 0.9, the documented limit, exactly; 64 x the hint is refused and the factor still works"""
    from glim_amd import api

    target, src, corr, _, _ = ring_case(name)
    tg, sg = upload(ctx, target), upload(ctx, src)
    f = api.IntegratedGICPFactor(np.eye(4), 1, tg, sg, max_correspondence_distance=gsc.RING_HINT)
    f.set_max_correspondence_distance(gsc.RING_D)
    values = {1: np.eye(4)}
    np.testing.assert_array_equal(f.correspondences(values), corr)
    f.set_max_correspondence_distance(64 * gsc.RING_HINT)
    for call in (f.correspondences, f.linearize, f.error):
        with pytest.raises(api.GlimAmdError):
            call(values)
    f.set_max_correspondence_distance(gsc.RING_D)
    np.testing.assert_array_equal(f.correspondences(values), corr)
    f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,max_d", [("lattice", 0.5), ("duplicates", 0.25), ("broken", 0.25), ("nonfinite", 1.0)])
def test_ct_factor(orc, ctx, name, max_d):
    """one bucket per exact pose (X = Y = the pose: the bucket's pose is X to the bit); for the lattice and the duplicates also two buckets
    between the identity and Rz(90), where the second bucket's pose is what Exp(Log()) returns and the oracle at that pose is the reference"""
    from glim_amd import api

    c = exact_cases()[name]
    tg = upload(ctx, c["target"])
    for pose in c["poses"]:
        T = gsc.EXACT_POSES[pose]
        src, corr, _, _ = exact_ref(name, pose, max_d)
        sg = upload(ctx, src)
        f = api.IntegratedCT_GICPFactor(0, 1, tg, sg, max_correspondence_distance=max_d, times=np.zeros(len(src)))
        vals = {0: T, 1: T}
        tab, Tk, _, _, idx = f.debug_poses(vals)
        assert len(tab) == 1 and np.array_equal(Tk[0], T) and not idx.any()
        np.testing.assert_array_equal(f.correspondences(vals), corr, err_msg=f"{name} {pose}")
        assert f.linearize(vals)["num_inliers"] == (corr >= 0).sum() == f.error(vals, with_inliers=True)[1]
        f.close()
        sg.close()
    if name in ("lattice", "duplicates"):
        src = c["source"]
        sg = upload(ctx, src)
        times = np.where(np.arange(len(src)) % 64 < 32, 0.0, 0.002)
        times = times[np.argsort(times, kind="stable")]
        max_d = {"lattice": 0.5, "duplicates": 1.0}[name]  # the second half of the duplicates' source is spread over the cube: few matches at 0.25
        f = api.IntegratedCT_GICPFactor(0, 1, tg, sg, max_correspondence_distance=max_d, times=times)
        vals = {0: np.eye(4), 1: gsc.RZ90}
        tab, Tk, _, _, idx = f.debug_poses(vals)
        assert len(tab) == 2 and np.array_equal(Tk[0], np.eye(4)) and np.abs(Tk[1] - gsc.RZ90).max() < 1e-12 and idx.sum() == len(src) // 2
        want = np.full(len(src), -1, dtype=np.int32)
        for k in range(2):
            sel = np.flatnonzero(idx == k)
            want[sel] = orc.gicp_linearize(c["target"], gsc.eye_covs(len(c["target"])), src[sel], gsc.eye_covs(len(sel)), Tk[k], max_d, want_corr=True)["corr"]
        first = gsc.brute_force(c["target"], src[idx == 0], max_d)[0]
        np.testing.assert_array_equal(want[idx == 0], first)  # the identity bucket: brute force again
        assert (want[idx == 1] >= 0).sum() > 10
        np.testing.assert_array_equal(f.correspondences(vals), want, err_msg=f"{name} two buckets")
        f.close()
        sg.close()
    tg.close()


@pytest.mark.gpu
def test_align_batch_counts_inliers_like_the_reference(orc, ctx):
    """one batch: the blob, the plane, the duplicates and the one-point target; at every pose the LM loop evaluated (read from the trace) the
    record's num_inliers is the reference's count at that pose"""
    from glim_amd import api

    T0 = general_pose(orc) @ orc.se3_exp([0.01, -0.02, 0.015, 0.03, -0.02, 0.04])
    problems = []
    for name, max_d in (("blob", 0.25), ("plane", 1.0), ("duplicates", 0.25)):
        target, src = general_ref(orc, name, max_d)[:2]
        problems.append((target, src, T0, max_d))
    one = gsc.tiny_targets()["n1"]
    problems.append((one, gsc.exact_source("n1", exact_cases()["n1"], "rz90"), gsc.RZ90, 1.0))
    tgs, sgs = [upload(ctx, p[0]) for p in problems], [upload(ctx, p[1]) for p in problems]
    results, traces = api.gicp_align_debug_trace(tgs, sgs, [p[2] for p in problems], [p[3] for p in problems], api.LMParams(max_iterations=3))
    for (target, src, T_init, max_d), r, trace in zip(problems, results, traces):
        assert len(trace) >= 1 and np.array_equal(trace[0]["T"], T_init)
        for k, e in enumerate(trace):
            ref = orc.gicp_linearize(target, gsc.eye_covs(len(target)), src, gsc.eye_covs(len(src)), e["T"], max_d, want_corr=True)
            assert int(e["compact"][0]) == ref["num_inliers"] == (ref["corr"] >= 0).sum(), (len(target), k)
        assert r.num_inliers == orc.gicp_linearize(target, gsc.eye_covs(len(target)), src, gsc.eye_covs(len(src)), r.T_target_source, max_d)["num_inliers"]
    assert results[0].trials >= 1 and results[1].trials >= 1 and results[0].num_inliers > 100
    # the first round of the one-point problem is exact data: brute force counts it too
    assert int(traces[3][0]["compact"][0]) == (exact_ref("n1", "rz90", 1.0)[1] >= 0).sum() > 0


@pytest.mark.gpu
def test_target_points_outside_the_grid_are_never_matched(ctx):
    """include/glim_amd.h at glim_amd_nn_index_create: a target point beyond 2^20 cells from the origin is kept out of the index; every other
    answer is what it would be without those points"""
    from glim_amd import api

    target, src, max_d = gsc.out_of_grid_case()
    _, ok = gsc.cell_edge(target, gsc.OUT_HINT)
    corr, _, d2 = gsc.brute_force(target, src, max_d, usable=ok)
    tg, sg = upload(ctx, target), upload(ctx, src)
    f = api.IntegratedGICPFactor(np.eye(4), 1, tg, sg, max_correspondence_distance=gsc.OUT_HINT)
    f.set_max_correspondence_distance(max_d)
    check_rigid(f, {1: np.eye(4)}, corr, d2, "out of the grid")
    f.close()
    only = upload(ctx, target[ok])  # the same cloud without the far points: the same matches, renumbered
    g = api.IntegratedGICPFactor(np.eye(4), 1, only, sg, max_correspondence_distance=gsc.OUT_HINT)
    g.set_max_correspondence_distance(max_d)
    got = g.correspondences({1: np.eye(4)})
    np.testing.assert_array_equal(np.where(got >= 0, np.flatnonzero(ok)[np.maximum(got, 0)], -1), corr)
    g.close()
