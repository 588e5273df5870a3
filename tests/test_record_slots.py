"""tests/record_slots.py proven on the CPU: the FP64 restatements against the oracle, the FP32 restatements against the gate, the gate
against single wrong entries, the inverse map against itself.  The cases are those of tests/test_gpu_record_slots.py with the voxel tables
and the matched sets restated on the host.

Figures of one run (the tests print them; -s shows them):
  FP32 restatement, added in the shape of the device's reduction, against the m = 2 gate: at most 0.07 of it (VGICP general), 0.36 (plane),
  0.49 (the tails: one point), 0.35 (GICP), 0.17 / 0.20 (ICP point-to-point / point-to-plane).
  Old gate / new gate (m = 2, s = 16) over the VGICP cases: between 2.5 (slot 27 in plane form, where Sherman-Morrison's denominator
  >= 0.002 makes P_j 3e-5 of Q_j) and 3e5 (slot 17); above 1 on every slot of every case.
  Mutations, against the widest gate the GPU tests may use (m = 8, s = 16), voxels of 0.5 m / 1.0 m:
    A02 taken for A12 in slot 19                  19 807 / 6 991 gates on slot 19      NOT caught by 2e-4 of the largest entry
    sign of G22 flipped                           39 273 / 9 037 gates on slot 14      caught
    one matched point left out of slots 15..20       472 /   178 gates on slot 20 / 18 NOT caught
    slot 17 multiplied by 1.5                     12 163 / 6 176 gates on slot 17      NOT caught
    0.999 replaced by 1.0 in the plane form        3 216 / 3 188 gates on slot 20 / 3  caught
    R taken for R^T in GICP's S                   19 399 gates on slot 23              caught
"""
import numpy as np
import pytest

import icp_restatement as icpr
import record_slots as rs

RES = (0.5, 1.0)
VGICP_CASES = [(plane, res, shift) for plane in (False, True) for res in RES for shift in (False, True) if not (shift and res == 1.0)]
GICP_KINDS = ("gicp", "icp_point", "icp_plane")


def _vgicp(pair, plane, res, shift, n=None):
    sc = rs.vgicp_scene(pair, plane, shift, n)
    return sc, rs.vgicp_matched(sc, res, rs.voxel_table(sc["tp"], sc["tc"], res))


_GICP = {}


def _gicp(pair, n=None):
    if n not in _GICP:
        sc = rs.gicp_scene(pair, n)
        _GICP[n] = (sc, rs.gicp_matched(sc, rs.nearest(sc["tp"], rs.transform(sc["T"], sc["sp"]), 1.0)))
    return _GICP[n]


def assert_record_close(got, ref, absum):
    """the rule of tests/test_restatement_4x4.py: 1e-9 of the block's largest entry plus 1e-13 of the absolute sums"""
    for k in ("H_ss", "b_s"):
        assert np.abs(got[k] - ref[k]).max() <= 1e-9 * np.abs(ref[k]).max() + 1e-13 * absum[k], (k, np.abs(got[k] - ref[k]).max())
    assert got["error"] == pytest.approx(ref["error"], rel=1e-9, abs=1e-12)


def _absum(c64):
    Q = np.abs(c64).sum(axis=0)
    return {"H_ss": Q[:21].max(), "b_s": Q[21:27].max()}


@pytest.mark.parametrize("res", RES)
@pytest.mark.parametrize("plane", [False, True], ids=["general", "plane"])
def test_fp64_vgicp_restatement_agrees_with_the_oracle(orc, small_pair, plane, res):
    """both forms on FP64 voxel statistics (the oracle's own): the general form as it stands; the plane form with the oracle given
    C_A = I - 0.999 n n^T exactly and the helper the unrounded (C_B + I)^-1 -- Sherman-Morrison then IS the oracle's inverse"""
    sc = rs.vgicp_scene(small_pair, plane)
    ref_vm = orc.VoxelMap(res).insert(sc["tp"], sc["tc"])
    rc, rn, rm, rC = ref_vm.voxels()
    table = {tuple(int(x) for x in c): (int(n), m - (c + 0.5) * res, C) for c, n, m, C in zip(rc, rn, rm[:, :3], rC[:, :3, :3])}
    coords = rs.voxel_coords(rs.transform(sc["T"], sc["sp"]), res)
    keys = [tuple(int(x) for x in c) for c in coords]
    i = np.array([k in table for k in keys]).nonzero()[0]
    mu, CB = np.stack([table[keys[k]][1] for k in i]), np.stack([table[keys[k]][2] for k in i])
    if plane:
        nrm = sc["sn"].astype(np.float64)
        covs = np.eye(3)[None] - 0.999 * nrm[:, :, None] * nrm[:, None, :]
        c64 = rs.vgicp_plane(sc["sp"][i], nrm[i], coords[i], mu, np.linalg.inv(CB + np.eye(3)), sc["T"], res, np.float64)
    else:
        covs = sc["sc"]
        c64 = rs.vgicp_general(sc["sp"][i], covs[i], coords[i], mu, CB, sc["T"], res, np.float64)
    ref = orc.vgicp_linearize(ref_vm, sc["sp"], covs, sc["T"], want_corr=True)
    np.testing.assert_array_equal(ref["corr"][:, :3], coords)
    np.testing.assert_array_equal(np.flatnonzero(ref["corr"][:, 3] >= 0), i)
    assert ref["num_inliers"] == len(i) > 1000
    assert_record_close(rs.record_of_sums(c64.sum(axis=0), sc["T"]), ref, _absum(c64))


def test_fp64_gicp_restatement_agrees_with_the_oracle(orc, small_pair):
    sc, m = _gicp(small_pair)
    ref = orc.gicp_linearize(sc["tp"], sc["tc"], sc["sp"], sc["sc"], sc["T"], 1.0, want_corr=True)
    np.testing.assert_array_equal(np.flatnonzero(ref["corr"] >= 0), m["idx"])
    c64 = rs.gicp_terms(sc, m, "gicp", np.float64)
    assert ref["num_inliers"] == len(c64) > 1000
    assert_record_close(rs.record_of_sums(c64.sum(axis=0)), ref, _absum(c64))


@pytest.mark.parametrize("kind", ["icp_point", "icp_plane"])
def test_fp64_icp_restatement_agrees_with_the_icp_restatement(small_pair, kind):
    sc, m = _gicp(small_pair)
    corr = np.full(len(sc["sp"]), -1)
    corr[m["idx"]] = rs.nearest(sc["tp"], rs.transform(sc["T"], sc["sp"]), 1.0)[m["idx"]]
    ref = icpr.icp_linearize(sc["tp"], sc["sp"], sc["T"], 1.0, normals=sc["tn"] if kind == "icp_plane" else None, corr=corr,
                             q=rs.transform(sc["T"], sc["sp"]))
    c64 = rs.gicp_terms(sc, m, kind, np.float64)
    assert ref["num_inliers"] == len(c64) > 1000
    assert_record_close(rs.record_of_sums(c64.sum(axis=0)), ref, _absum(c64))


def _ratio(c32, c64, m, ppt):
    """c32: the draws of the FP32 restatement; [0], the restatement itself, is what is added up"""
    g = rs.gate(c32, c64, rs.additions(ppt))
    err = np.abs(rs.device_sum(c32[0], m["idx"], m["n"], ppt) - g["S"])
    assert np.all(err[g["exact"]] == 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(g["exact"], 0.0, err / g["gate"])


def test_fp32_restatement_stays_within_the_gate(small_pair):
    """The condition that the inputs were chosen well: on every case of the GPU tests the FP32 restatement, its terms added in FP32 in the
    shape of the device's reduction (device_sum), stays within the m = 2 gate on every slot.  (|sum c32 - S| <= P by construction; the FP32
    additions are what this checks the s 2^-24 Q term against.)  Measured: at most 0.50 anywhere."""
    worst = {}
    for plane, res, shift in VGICP_CASES:
        for ppt in (1, 3, 8):
            sc, m = _vgicp(small_pair, plane, res, shift)
            r = _ratio(rs.vgicp_draws(sc, m), rs.vgicp_terms(sc, m, np.float64), m, ppt)
            key = "vgicp plane" if plane else "vgicp general"
            worst[key] = max(worst.get(key, (0.0, 0)), (r.max(), int(r.argmax())))
    for n in (1, 63, 64, 65, 255, 256, 257, 767, 768, 769, 2047, 2048, 2049):
        for plane in (False, True):
            sc, m = _vgicp(small_pair, plane, 0.5, False, n)
            r = _ratio(rs.vgicp_draws(sc, m), rs.vgicp_terms(sc, m, np.float64), m, 1)
            key = "vgicp tails"
            worst[key] = max(worst.get(key, (0.0, 0)), (r.max(), int(r.argmax())))
    for kind in GICP_KINDS:
        for n in (1, 65, 257, 4096):
            sc, m = _gicp(small_pair, n)
            r = _ratio(rs.gicp_draws(sc, m, kind), rs.gicp_terms(sc, m, kind, np.float64), m, 1)
            worst[kind] = max(worst.get(kind, (0.0, 0)), (r.max(), int(r.argmax())))
    for k, (v, j) in worst.items():
        print(f"{k:14s} worst |FP32 sums - S| / gate(m = 2) = {v:.3f} on slot {j} ({rs.SLOT_NAMES[j]})")
        assert v <= 1.0, (k, v, j)


def test_new_gate_against_the_old_one(small_pair):
    """what the per-slot gate buys: old gate / new gate per slot, the smallest and the largest over the VGICP cases"""
    lo, hi = np.full(rs.NSLOTS, np.inf), np.zeros(rs.NSLOTS)
    for plane, res, shift in VGICP_CASES:
        sc, m = _vgicp(small_pair, plane, res, shift)
        g = rs.gate(rs.vgicp_draws(sc, m), rs.vgicp_terms(sc, m, np.float64), rs.additions(8))
        ratio = rs.old_gate(g["S"]) / g["gate"]
        lo, hi = np.minimum(lo, ratio), np.maximum(hi, ratio)
    for j in range(rs.NSLOTS):
        print(f"slot {j:2d} {rs.SLOT_NAMES[j]:6s} old gate / new gate: {lo[j]:10.1f} .. {hi[j]:10.1f}")
    assert lo.min() > 1.0  # the new gate is the tighter one on every slot of every case


def _mutations(pair, res):
    """(name, family, c32 mutated, c64, matched) one wrong entry at a time"""
    out = []
    sc, m = _vgicp(pair, False, res, False)
    c32, c64 = rs.vgicp_draws(sc, m), rs.vgicp_terms(sc, m, np.float64)

    def mutated(f):
        c = c32[0].copy()
        f(c)
        return c

    def swap(c):
        c[:, 19] = c[:, 17]

    def flip(c):
        c[:, 14] = -c[:, 14]

    def drop(c):
        c[len(c) // 2, 15:21] = 0.0

    def scale(c):
        c[:, 17] *= np.float32(1.5)

    out.append(("A02 taken for A12 in slot 19", c32, mutated(swap), c64, m))
    out.append(("sign of G22 (slot 14) flipped", c32, mutated(flip), c64, m))
    out.append(("one matched point left out of slots 15..20", c32, mutated(drop), c64, m))
    out.append(("slot 17 multiplied by 1.5", c32, mutated(scale), c64, m))
    scp, mp = _vgicp(pair, True, res, False)
    out.append(("0.999 replaced by 1.0 in the plane form", rs.vgicp_draws(scp, mp), rs.vgicp_terms(scp, mp, np.float32, w=1.0),
                rs.vgicp_terms(scp, mp, np.float64), mp))
    scg, mg = _gicp(pair)
    out.append(("R taken for R^T in GICP's S", rs.gicp_draws(scg, mg, "gicp"), rs.gicp_terms(scg, mg, "gicp", np.float32, transpose=True),
                rs.gicp_terms(scg, mg, "gicp", np.float64), mg))
    return out


@pytest.mark.parametrize("res", RES)
def test_gate_catches_single_wrong_entries(small_pair, res):
    """Each mutation of the FP32 terms pushes at least one slot beyond its gate -- at the widest gate the GPU tests may use (m = 8, ppt = 8) --
    while the unmutated terms pass at m = 2.  The gate is made of the UNMUTATED restatement, as in the GPU tests; the mutated terms stand for
    the device.  Printed per mutation: the slot it trips worst, by how much, and whether the suite's 2e-4-of-the-largest-entry rule would
    have seen it."""
    unseen = []
    for name, good, bad, ref, mm in _mutations(small_pair, res):
        g0 = rs.gate(good, ref, rs.additions(1))
        assert np.all(np.abs(rs.device_sum(good[0], mm["idx"], mm["n"], 1) - g0["S"]) <= g0["gate"])
        assert 1024 < len(mm["idx"]) <= 4096  # ("one matched point in 4096": the scan has 4096 points)
        clean = rs.gate(good, ref, rs.additions(8), m=rs.M_MAX)
        err = np.abs(rs.device_sum(bad, mm["idx"], mm["n"], 1) - clean["S"])
        over = err / clean["gate"]
        old = bool(np.any(err > rs.old_gate(clean["S"])))
        j = int(over.argmax())
        print(f"res {res}: {name:44s} trips slot {j:2d} ({rs.SLOT_NAMES[j]}) at {over[j]:9.1f} gates (m = 8); 2e-4-of-max rule: {'caught' if old else 'NOT caught'}")
        assert over[j] > 1.0, name
        if not old:
            unseen.append(name)
    assert len(unseen) >= 3, unseen  # the point of the per-slot gate


def test_inverse_map_is_exact(small_pair):
    rng = np.random.default_rng(3)
    sc, m = _vgicp(small_pair, False, 0.5, True)
    S = rs.vgicp_terms(sc, m, np.float64).sum(axis=0)
    for T in (sc["T"], None):
        for sums in (S, rng.normal(size=rs.NSLOTS) * np.abs(S)):
            back = rs.sums_of_record(rs.record_of_sums(sums, T), T)
            assert np.all(np.abs(back - sums) <= 64 * 2.0 ** -53 * rs.block_max(sums)), np.abs(back - sums) / rs.block_max(sums)
    z = rs.record_of_sums(np.zeros(rs.NSLOTS), sc["T"])
    assert not np.any(z["H_ss"]) and not np.any(z["b_s"]) and z["error"] == 0.0


def test_voxel_table_restates_the_oracle_map(orc, small_pair):
    """counts and coordinates equal; the centre-relative FP32 mean is the FP64 oracle mean to half an FP32 step of a number below res / 2
    (plus the fixed point's 2^-28); absolute_means rounds it as a download does"""
    for shift in (False, True):
        sc = rs.vgicp_scene(small_pair, False, shift)
        for res in RES:
            table = rs.voxel_table(sc["tp"], sc["tc"], res)
            rc, rn, rm, rC = orc.VoxelMap(res).insert(sc["tp"], sc["tc"]).voxels()
            assert len(table) == len(rc)
            for c, n, mu, C in zip(rc, rn, rm[:, :3], rC[:, :3, :3]):
                k, rel, CB = table[tuple(int(x) for x in c)]
                assert k == n
                assert np.abs(rel.astype(np.float64) - (mu - (c + 0.5) * res)).max() <= 2.0 ** -24 * res / 2 + 2.0 ** -28
                np.testing.assert_allclose(CB, C, rtol=2.0 ** -24, atol=1e-30)
                np.testing.assert_array_equal(rs.absolute_means(c, rel, res), (rel.astype(np.float64) + (c + 0.5) * res).astype(np.float32))
