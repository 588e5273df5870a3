"""The factor records of vgicp_kernel (accumulate_point, both forms), gicp_kernel (gicp_point) and icp_kernel (icp_point), entry by entry:
every one of the 28 accumulated sums behind a record against the FP64 restatement of tests/record_slots.py, each within the gate that module
derives for it from the FP32 restatement (m P_j + s 2^-24 Q_j + 64 2^-53 max|block|) -- not within 2e-4 of the record's largest entry.

Teacher-forced: only the factor kernel is under test.  The matched set is the device's (asserted equal to the oracle's first), the pose is
the delta the factor itself forms, the voxel covariances are the downloaded table's.  The voxel MEANS are the table's too, but restated: the
table keeps them relative to the voxel centre, the download returns absolute FP32 values (2e-6 m a step at 30 m, 1.5e-5 m at 200 m -- a
hundred times the FP32 step of the residual), so record_slots.voxel_table restates the map's integer sums and the test asserts that every
downloaded mean is that record's value rounded as the download rounds it.  The plane view (C_B + I)^-1 is restated from the downloaded
covariances the same way (FP64 inverse, stored FP32).

s = ppt + 8 where ppt= pins the points per thread; a set left to the planner is a small set here (at most 8 points per thread:
vgicp.hip small_set_ppt), so s = 16.  The GICP family takes one point per thread at these sizes (gicp_factor.hpp points_per_thread): s = 9.

Worst |device - S_j| / P_j over every slot of every case, per family and form, and the m chosen (at least twice the figure, at most 8;
test_the_margins_hold asserts both for the run at hand); in brackets the largest |device - S_j| / gate_j at that m:
  VGICP general         1.05 on slot 20 (M22), the 300-point factor of the set of twenty                     m = 3   [0.20]
  VGICP plane           1.91 on slot 18 (M11), the one-point source (0.85 on every larger one: slot 5)       m = 4   [0.43]
  VGICP error-only      0.07 general, 0.25 plane (slot 27); frozen 0.07, 0.15                                 (the form's m)
  GICP                  2.75 on slot 18 (M11), the one-point source (0.95 on every larger one: slot 19)      m = 6   [0.16]
  ICP point-to-point    2.22 on slot 2 (Hww02), 65 points                                                     m = 5   [0.10]
  ICP point-to-plane    2.03 on slot 6 (G00), 65 points                                                       m = 5   [0.16]
Every record was bit-identical on its second call; every matched set equal to the oracle's (ICP: to brute force); every downloaded voxel mean
the restated record's.  One run on an MI355X.

What the first runs found, and what became of it (no kernel was changed: none was wrong):
  * With LAPACK's inverse in the FP32 restatement the device stood up to 12.4 P_j from the reference (G00 of the one-point GICP factor; 4.2 on
    Hww01 of a 33-point VGICP factor).  The kernels' general path inverts S by the adjugate over the determinant, and the determinant of
    S (eigenvalues 0.02, 2, 2) cancels where an LU does not: a conditioning effect of the kernel's algebraic form.  The stage went into the
    restatement (record_slots._inv), as the gate's derivation asks.
  * With ONE FP32 draw per term, one-point factors stood up to 23 P_j away (slot 27 of the GICP one: its restated term happened to be right to
    a quarter of an FP32 step) while inside the gate through the s 2^-24 Q_j term: the ratio of two single rounding errors has no bound.
    P_j now takes, point by point, the largest error of six draws -- the same FP32 evaluation in the six right-handed relabellings of the
    axes (record_slots.draws) -- and the figures above are against that P_j.
"""
import numpy as np
import pytest

import icp_restatement as icpr
import record_slots as rs
from test_gpu_parity import assert_linearization_close

pytestmark = pytest.mark.gpu

M = {"vgicp general": 3.0, "vgicp plane": 4.0, "gicp": 6.0, "icp_point": 5.0, "icp_plane": 5.0}  # (the module docstring: measured worst x 2, rounded up)
WORST = {}
T_TARGET = np.eye(4)
T_TARGET[:3, :3], T_TARGET[:3, 3] = rs.rodrigues([0.1, -0.2, 0.3]), [1.0, 2.0, -0.5]
PLANE_BYTES, GENERAL_BYTES = 16 + 24 + 16 + 24, 16 + 24 + 16 + 36 + 16  # per point: points, covariances, normals, factor stream


@pytest.fixture(scope="module")
def api():
    from glim_amd import api as _api

    assert _api.device_count() >= 1, "these tests need a GPU and must not fall back"
    return _api


@pytest.fixture(scope="module")
def ctx(api):
    return api.Context(0, 1)


@pytest.fixture(scope="module")
def maps(api, ctx, orc, small_pair):
    """(shift, res) -> the device map, the oracle's map, and the table the kernel reads, restated and checked against the download"""
    cache = {}

    def get(shift, res):
        if (shift, res) not in cache:
            sc = rs.vgicp_scene(small_pair, False, shift)
            tg = api.PointCloudGPU.clone(sc["tp"].astype(np.float64), sc["tc"], ctx=ctx)
            vm = api.GaussianVoxelMapGPU(res, ctx=ctx).insert(tg)
            gc, gn, gm, gC = vm.voxels()
            host = rs.voxel_table(sc["tp"], sc["tc"], res)
            assert len(host) == len(gc)
            table = {}
            for c, n, mean, C in zip(gc, gn, gm, gC):
                key = tuple(int(x) for x in c)
                k, rel, _ = host[key]
                assert k == n
                np.testing.assert_array_equal(rs.absolute_means(c, rel, res), mean)
                table[key] = (k, rel, C)
            cache[(shift, res)] = dict(vm=vm, tg=tg, table=table, ref=orc.VoxelMap(res).insert(sc["tp"], sc["tc"]))
        return cache[(shift, res)]

    return get


def note(family, ratios, label, of_gate=None):
    """keeps the worst |device - S_j| / P_j of a family for the module's docstring (of_gate: the largest |device - S_j| / gate_j, printed)"""
    if np.all(np.isnan(ratios)):
        return
    j = int(np.nanargmax(ratios))
    if ratios[j] > WORST.get(family, (0.0, 0, ""))[0]:
        WORST[family] = (float(ratios[j]), j, label)
    print(f"{family}: {label}: worst |device - S| / P = {ratios[j]:.3f} on slot {j} ({rs.SLOT_NAMES[j]})" + ("" if of_gate is None else f", / gate = {of_gate:.3f}"))


def check_and_note(family, sums, g, label):
    ratios = rs.check(sums, g, label)
    note(family, ratios, label, float(np.max(np.where(g["exact"], 0.0, np.abs(sums - g["S"]) / np.where(g["exact"], 1.0, g["gate"])))))


def same_bits(a, b):
    assert a["num_inliers"] == b["num_inliers"] and a["error"] == b["error"]
    for k in ("H_ss", "b_s", "H_tt", "H_ts", "b_t"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def check_target_blocks(L, T, binary):
    """H_tt = Ad^T H_ss Ad, H_ts = -Ad^T H_ss, b_t = -Ad^T b_s from the DEVICE's own source blocks: FP64 host code, 1e-12 of the absolute sums"""
    if not binary:
        assert not np.any(L["H_tt"]) and not np.any(L["H_ts"]) and not np.any(L["b_t"])
        return
    Ad, H, b = rs.adjoint(T), L["H_ss"], L["b_s"]
    aA, aH = np.abs(Ad), np.abs(H)
    assert np.all(np.abs(L["H_tt"] - Ad.T @ H @ Ad) <= 1e-12 * (aA.T @ aH @ aA))
    assert np.all(np.abs(L["H_ts"] + Ad.T @ H) <= 1e-12 * (aA.T @ aH))
    assert np.all(np.abs(L["b_t"] + Ad.T @ b) <= 1e-12 * (aA.T @ np.abs(b)))


def is_zero(L):
    return L["num_inliers"] == 0 and L["error"] == 0.0 and not any(np.any(L[k]) for k in ("H_ss", "b_s", "H_tt", "H_ts", "b_t"))


def upload_source(api, ctx, sc):
    if len(sc["sp"]) == 0:
        return api.PointCloudGPU.clone(np.zeros((0, 3)), np.zeros((0, 3, 3)), ctx=ctx)
    return api.PointCloudGPU.clone(sc["sp"].astype(np.float64), sc["sc"], sc["sn"].astype(np.float64), ctx=ctx)


def assert_form(sg, sc):
    """the cloud took the form the case is about (its factor stream: 24 B a point in plane form, 36 + 16 otherwise)"""
    assert sg.memory_usage_gpu() == len(sc["sp"]) * (PLANE_BYTES if sc["plane"] else GENERAL_BYTES)


def check_vgicp_record(orc, mp, sc, res, fset, index, factor, values, L, s, label):
    """one VGICP record on all 28 slots"""
    T = factor.calc_delta(values)
    corr = fset.correspondences(index, T)
    if len(sc["sp"]):
        ref = orc.vgicp_linearize(mp["ref"], sc["sp"], sc["sc"], T, want_corr=True)
        np.testing.assert_array_equal(corr[:, :3], ref["corr"][:, :3])
        np.testing.assert_array_equal(corr[:, 3] > 0, ref["corr"][:, 3] >= 0)
    m = rs.vgicp_matched(sc, res, mp["table"], corr[:, :3])
    np.testing.assert_array_equal(m["idx"], np.flatnonzero(corr[:, 3] > 0))
    assert L["num_inliers"] == len(m["idx"])
    family = "vgicp plane" if sc["plane"] else "vgicp general"
    if len(m["idx"]) == 0:
        assert is_zero(L), label
        return m
    g = rs.gate(rs.vgicp_draws(sc, m, T=T), rs.vgicp_terms(sc, m, np.float64, T=T), s, m=M[family])
    check_and_note(family, rs.sums_of_record(L, T), g, label)
    check_target_blocks(L, T, factor.is_binary)
    return m


def poses(sc, binary):
    return ({0: T_TARGET, 1: T_TARGET @ sc["T"]}, 0) if binary else ({1: T_TARGET @ sc["T"]}, T_TARGET)


@pytest.mark.parametrize("binary", [False, True], ids=["unary", "binary"])
@pytest.mark.parametrize("res,shift", [(0.5, False), (1.0, False), (0.5, True)], ids=["0.5", "1.0", "0.5-at-200m"])
@pytest.mark.parametrize("plane", [False, True], ids=["general", "plane"])
def test_vgicp_record_slot_by_slot(api, ctx, orc, small_pair, maps, plane, res, shift, binary):
    mp = maps(shift, res)
    sc = rs.vgicp_scene(small_pair, plane, shift)
    sg = upload_source(api, ctx, sc)
    values, target = poses(sc, binary)
    f = api.IntegratedVGICPFactorGPU(target, 1, mp["vm"], sg)
    fset = api.NonlinearFactorSetGPU(ctx)
    fset.add(f)
    L = fset.linearize(values)[0]
    assert_form(sg, sc)
    same_bits(L, fset.linearize(values)[0])
    m = check_vgicp_record(orc, mp, sc, res, fset, 0, f, values, L, rs.additions(8), f"res {res} shift {shift} binary {binary}")
    assert len(m["idx"]) > 1000
    # the suite's older rule on the same record (2e-4 of each block's largest entry and the Gauss-Newton step, against the oracle on FP64 voxel
    # statistics): kept beside the per-slot gate, which is the tighter of the two on every slot (tests/test_record_slots.py)
    assert_linearization_close(L, orc.vgicp_linearize(mp["ref"], sc["sp"], sc["sc"], f.calc_delta(values)), binary)


TAILS = [(0, n) for n in (1, 63, 64, 65, 255, 256, 257)] + [(ppt, 256 * ppt + d) for ppt in (1, 3, 8) for d in (-1, 0, 1)]


@pytest.mark.parametrize("ppt,n", TAILS)
def test_vgicp_tails_and_reduction_paths(api, ctx, orc, small_pair, maps, ppt, n):
    """the first n points of the scan, both forms: the smallest sizes that reach one lane, a wavefront's edge, a block's edge and, with the
    points per thread pinned, a thread's last trip"""
    mp = maps(False, 0.5)
    for plane in (False, True):
        sc = rs.vgicp_scene(small_pair, plane, False, n)
        sg = upload_source(api, ctx, sc)
        with ctx.diag(f"ppt={ppt}" if ppt else ""):
            f = api.IntegratedVGICPFactorGPU(T_TARGET, 1, mp["vm"], sg)
            fset = api.NonlinearFactorSetGPU(ctx)
            fset.add(f)
            values = {1: T_TARGET @ sc["T"]}
            L = fset.linearize(values)[0]
            same_bits(L, fset.linearize(values)[0])
            assert_form(sg, sc)
            check_vgicp_record(orc, mp, sc, 0.5, fset, 0, f, values, L, rs.additions(ppt or 8), f"n {n} ppt {ppt} plane {plane}")


@pytest.mark.parametrize("plane", [False, True], ids=["general", "plane"])
def test_vgicp_record_in_a_set_of_twenty(api, ctx, orc, small_pair, maps, plane):
    """16 or more factors switch on the XCD-aware block map: 20 factors of different sizes over two maps, unary and binary, one of them with an
    empty source and one whose pose misses the map -- every record on all slots, the two empty ones exactly zero"""
    mps = [maps(False, 0.5), maps(False, 1.0)]
    sizes = [700, 257, 1, 4096, 64, 1000, 0, 1500, 300, 2049, 65, 511, 4095, 128, 900, 33, 2500, 256, 1023, 77]
    fset = api.NonlinearFactorSetGPU(ctx)
    values = {0: T_TARGET}
    cases = []
    for k, n in enumerate(sizes):
        sc = rs.vgicp_scene(small_pair, plane, False, n)
        sg = upload_source(api, ctx, sc)
        T = rs.perturbed(sc["T"], w=(0.001 * k, -0.002, 0.0015), v=(0.002 * k, 0.01, -0.01))
        if k == 12:
            T[:3, 3] += 1e4  # (misses the map)
        values[k + 1] = T_TARGET @ T
        f = api.IntegratedVGICPFactorGPU(0 if k % 3 else T_TARGET, k + 1, mps[k % 2]["vm"], sg)
        fset.add(f)
        cases.append((sc, f))
    out = fset.linearize(values)
    again = fset.linearize(values)
    for k, ((sc, f), L, L2) in enumerate(zip(cases, out, again)):
        same_bits(L, L2)
        if sizes[k]:
            assert_form(f.source, sc)
        m = check_vgicp_record(orc, mps[k % 2], sc, (0.5, 1.0)[k % 2], fset, k, f, values, L, rs.additions(8), f"factor {k} of 20, n {sizes[k]}")
        if k in (6, 12):
            assert len(m["idx"]) == 0 and is_zero(L)
    assert sum(L["num_inliers"] > 0 for L in out) >= 17


@pytest.mark.parametrize("plane", [False, True], ids=["general", "plane"])
def test_vgicp_error_only_and_frozen_forms(api, ctx, orc, small_pair, maps, plane):
    """fset.error(values) (correspondences at the evaluation pose) and fset.error(values, values_lin=...) (frozen at the linearisation pose)
    against slot 27 of the restatement over the matching correspondence set, within slot 27's gate"""
    mp = maps(False, 0.5)
    sc = rs.vgicp_scene(small_pair, plane)
    sg = upload_source(api, ctx, sc)
    f = api.IntegratedVGICPFactorGPU(np.eye(4), 1, mp["vm"], sg)
    fset = api.NonlinearFactorSetGPU(ctx)
    fset.add(f)
    T_lin = sc["T"]
    T_eval = rs.perturbed(T_lin, w=(0.002, -0.001, 0.003), v=(0.02, -0.03, 0.01))
    family = "vgicp plane" if plane else "vgicp general"
    for frozen in (False, True):
        e = fset.error({1: T_eval}, values_lin={1: T_lin} if frozen else None)[0]
        assert e == fset.error({1: T_eval}, values_lin={1: T_lin} if frozen else None)[0]
        T_match = T_lin if frozen else T_eval
        corr = fset.correspondences(0, T_match)
        ref = orc.vgicp_linearize(mp["ref"], sc["sp"], sc["sc"], T_match, want_corr=True)
        np.testing.assert_array_equal(corr[:, :3], ref["corr"][:, :3])
        np.testing.assert_array_equal(corr[:, 3] > 0, ref["corr"][:, 3] >= 0)
        m = rs.vgicp_matched(sc, 0.5, mp["table"], corr[:, :3])
        assert fset.last_error_inliers[0] == len(m["idx"]) > 1000
        kw = dict(T=T_lin, T_eval=T_eval) if frozen else dict(T=T_eval)
        g = rs.gate(rs.vgicp_draws(sc, m, **kw), rs.vgicp_terms(sc, m, np.float64, **kw), rs.additions(8), m=M[family])
        err = abs(e - g["S"][27])
        print(f"{family} error, frozen {frozen}: |device - S| / P = {err / g['P'][27]:.3f}, / gate = {err / g['gate'][27]:.3f}")
        assert err <= g["gate"][27]
        ratios = np.full(rs.NSLOTS, np.nan)
        ratios[27] = err / g["P"][27]
        note(family, ratios, f"error frozen {frozen}")


def check_source_frame_record(L, sc, m, kind, T, binary, label):
    assert L["num_inliers"] == len(m["idx"])
    if len(m["idx"]) == 0:
        assert is_zero(L), label
        return
    g = rs.gate(rs.gicp_draws(sc, m, kind, T=T), rs.gicp_terms(sc, m, kind, np.float64, T=T), rs.additions(1), m=M[kind])
    if kind == "icp_point":
        # the zeros of hat(p) and of I, and the counts (a point with a zero coordinate adds exact terms elsewhere too)
        assert {6, 10, 14, 15, 16, 17, 18, 19, 20} <= set(np.flatnonzero(g["exact"]).tolist())
        assert g["S"][15] == g["S"][18] == g["S"][20] == len(m["idx"])
    check_and_note(kind, rs.sums_of_record(L), g, label)
    check_target_blocks(L, T, binary)


@pytest.fixture(scope="module")
def gicp_clouds(api, ctx, small_pair):
    """n -> the scene and its clouds on the device; the target carries covariances and normals and serves every factor of the family"""
    cache = {}

    def get(n):
        if n not in cache:
            sc = rs.gicp_scene(small_pair, n)
            if "tg" not in cache:
                cache["tg"] = api.PointCloudGPU.clone(sc["tp"].astype(np.float64), sc["tc"], sc["tn"].astype(np.float64), ctx=ctx)
            cache[n] = (sc, cache["tg"], api.PointCloudGPU.clone(sc["sp"].astype(np.float64), sc["sc"], ctx=ctx))
        return cache[n]

    return get


@pytest.mark.parametrize("binary", [False, True], ids=["unary", "binary"])
@pytest.mark.parametrize("n", [1, 65, 257, 4096])
def test_gicp_record_slot_by_slot(api, ctx, orc, gicp_clouds, n, binary):
    sc, tg, sg = gicp_clouds(n)
    values, target = poses(sc, binary)
    f = api.IntegratedGICPFactor(target, 1, tg, sg, max_correspondence_distance=1.0)
    T = f.calc_delta(values)
    L = f.linearize(values)
    same_bits(L, f.linearize(values))
    corr = f.correspondences(values)
    ref = orc.gicp_linearize(sc["tp"], sc["tc"], sc["sp"], sc["sc"], T, 1.0, want_corr=True)
    np.testing.assert_array_equal(corr, ref["corr"])
    np.testing.assert_array_equal(corr, rs.nearest(sc["tp"], icpr.transform(sc["sp"], T), 1.0))  # ... which is brute force's
    m = rs.gicp_matched(sc, corr)
    assert n < 4096 or len(m["idx"]) > 1000
    check_source_frame_record(L, sc, m, "gicp", T, binary, f"gicp n {n} binary {binary}")
    f.close()


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
@pytest.mark.parametrize("n", [1, 65, 4096])
def test_icp_record_slot_by_slot(api, ctx, gicp_clouds, n, plane):
    """exact slots (point-to-point: the zeros of hat(p) and of the identity, the three counts) with ==, the others by their gates"""
    sc, tg, sg = gicp_clouds(n)
    kind = "icp_plane" if plane else "icp_point"
    for binary in (False, True):
        values, target = poses(sc, binary)
        f = api.IntegratedICPFactor(target, 1, tg, sg, max_correspondence_distance=1.0, use_point_to_plane=plane)
        T = f.calc_delta(values)
        L = f.linearize(values)
        same_bits(L, f.linearize(values))
        corr = f.correspondences(values)
        np.testing.assert_array_equal(corr, rs.nearest(sc["tp"], icpr.transform(sc["sp"], T), 1.0))
        m = rs.gicp_matched(sc, corr)
        assert n < 4096 or len(m["idx"]) > 1000
        check_source_frame_record(L, sc, m, kind, T, binary, f"{kind} n {n} binary {binary}")
        f.close()


def test_the_margins_hold():
    """runs last: every family's m keeps a factor 2 over the worst |device - S_j| / P_j this run measured, and is at most 8"""
    for family, (worst, j, label) in WORST.items():
        print(f"{family}: worst |device - S| / P = {worst:.3f} on slot {j} ({rs.SLOT_NAMES[j]}) in '{label}'; m = {M[family]}")
        assert 2.0 * worst <= M[family] <= rs.M_MAX, (family, worst, j, label)
