"""The records of the continuous-time GICP factor (ct_gicp_block, ct_bucket_block, ct_sum_rows of ct_factor.hpp; ct_gicp_kernel, ct_bucket_kernel,
ct_sum_kernel, ct_error_kernel of gicp.hip) and of the GICP and CT factors over a device iVox (IvoxSearch), entry by entry: each of the 92
entries of a CT record against the FP64 restatement of tests/record_slots.py (ct_record), within the gate ct_gate derives for it from the FP32
restatement bucket by bucket -- not within 2e-4 of the record's largest entry, which ct_restatement._check_record keeps asserting beside it.

Teacher-forced, like tests/test_gpu_record_slots.py: the matched set is the device's (asserted equal to the oracle's per-bucket search, or to the
restated map's bounded search with no fragile point, first), the pose tables T, D0, D1 are the device's (asserted within 1e-12 of ct_poses and
the bucket of every point equal to time_table's), the source covariances are the device's own estimates, downloaded, and over a map the target
points and covariances are the downloaded cells' FP32 values.  The cases are tests/ct_record_cases.py's; a CT block takes one point per thread
at these sizes (record_slots.points_per_thread), so s = 9.

error(values) after linearize(values) runs ct_error_kernel over the kept M = R A R^T at the same poses; it is held to the record's own error
entry and gate.  error(moved) is held to ct_frozen_terms' gate (slot 27's formula).

Worst |device - S_E| / P_E over every entry of every case, per family, and the m chosen (at least twice the figure, at most 8;
test_the_margins_hold asserts both for the run at hand); in brackets the largest |device - S_E| / gate_E at that m:
  CT record                 2.48 on H2_7, nbk9 (25 pairs in 9 buckets); 0.33 on the sweep (H1_1), 0.30 on the tails   m = 6   [0.39]
  CT error() at the point   0.83 on the error, nbk1 (3 pairs); 0.55 on nbk8, 0.08 on the tails, 0.001 on the sweep     (the record's m) [0.12]
  CT frozen error           0.70 on the error, nbk8; 0.63 on nbk1, 0.30 on the registered scan, 0.08 on the tails                  m = 2   [0.23]
  CT record over the map    0.31 on H1_5, the tails; 0.16 on the sweep (H1_1)                                          m = 6   [0.04]
  ... error() at the point  0.07 (tails), 0.05 (sweep)                                                                  (the record's m) [0.01]
  ... frozen error          0.07 (tails), 0.04 (sweep)                                                                  m = 2   [0.03]
  GICP over the map         1.00 on G10, the one-point source; 0.42 on 65 and 257 points, 0.14 on 4096                 m = 6 (the GICP family's) [0.15]
The frozen error adds the FP32 stage M = R A R^T to the per-point algebra: measured 0.70, so m = 2.  Every record was bit-identical on its
second and third call; every matched set equal to the oracle's, over the map to the restated bounded search with no fragile point; every pose
table within 1e-12 of ct_poses.  One run on an MI355X; every test under 0.2 s there.  No kernel was changed: none was wrong.

What the first run found: ct_restatement._check_record's Gauss-Newton step failed on the three pairs of nbk1 with every entry at 0.13 of its
gate (m = 6) or less -- the begin pose's block of three pairs is singular (smallest eigenvalue 3e-10 of the largest, below the rule's damping), so the
step is the damping's.  The rule now leaves the step out where the reference says so (check_ct_case); its entry tolerances stay.
"""
import numpy as np
import pytest

import ct_record_cases as cc
import ct_restatement as ctg
import ivox_restatement as ivr
import record_slots as rs
import test_gpu_record_slots as grs
from test_gpu_record_slots import check_source_frame_record, check_target_blocks  # noqa: F401  (check_target_blocks runs inside the former)
from test_ivox import _glim_ct_map, _hits_to_pairs, assert_same_map

pytestmark = pytest.mark.gpu

# (the module docstring: measured worst x 2, rounded up; error() at the linearisation point is held to the record's gate, so to its m)
M = {"ct": 6.0, "ct frozen": 2.0, "ivox ct": 6.0, "ivox ct frozen": 2.0}
M["ct error()"], M["ivox ct error()"] = M["ct"], M["ivox ct"]
WORST = {}
S = rs.additions(1)
CASES = cc.cases()


@pytest.fixture(scope="module")
def api():
    from glim_amd import api as _api

    assert _api.device_count() >= 1, "these tests need a GPU and must not fall back"
    return _api


@pytest.fixture(scope="module")
def gpu_ctx(api):
    return api.Context(0, 1)


@pytest.fixture(scope="module")
def world(api, gpu_ctx):
    """the target (ct_restatement._target(16, 512)) and the 4096-point scan with the covariances the device estimates for it"""
    tp, tc, tg = ctg._target(api, gpu_ctx, 16, 512)
    p, _ = ctg.moving_source(16, 256)
    g = api.PointCloudGPU.clone(p, ctx=gpu_ctx)
    g.find_neighbors(10, download=False)
    g.estimate_covariances(10)
    xyz, covs, _ = g.download(covs=True, normals=False)
    np.testing.assert_array_equal(xyz, p.astype(np.float32))
    return dict(tp=tp, tc=tc, tg=tg, p=xyz.astype(np.float64), covs=covs.astype(np.float64))


@pytest.fixture(scope="module")
def ivox(api, gpu_ctx, world):
    """the target cloud in a device iVox and in the restated one; cells: the downloaded FP32 points and covariances, slot by slot"""
    dev, ref = _glim_ct_map(api, gpu_ctx)
    dev.insert(world["tg"])
    ref.insert(world["tp"].astype(np.float32), world["tc"].astype(np.float32))
    coords, counts, points, covs = assert_same_map(dev, ref)
    yield dict(dev=dev, ref=ref, points=points, covs=covs, cap=dev.max_points)
    dev.close()


def note(family, ratios, label, of_gate):
    if np.all(np.isnan(ratios)):
        return
    j = int(np.nanargmax(ratios))
    if ratios[j] > WORST.get(family, (0.0, 0, ""))[0]:
        WORST[family] = (float(ratios[j]), j, label)
    print(f"{family}: {label}: worst |device - S| / P = {ratios[j]:.3f} on entry {j} ({rs.CT_NAMES[j]}), / gate = {of_gate:.3f}")


def upload(api, ctx, case, world):
    sc = cc.scene(case, world["tp"], world["tc"], world["p"], world["covs"])
    sg = api.PointCloudGPU.clone(sc["sp"], sc["sc"], ctx=ctx)
    xyz, covs, _ = sg.download(covs=True, normals=False)
    np.testing.assert_array_equal(xyz.astype(np.float64), sc["sp"])  # the scene holds FP32 values: the device holds the same
    np.testing.assert_array_equal(covs.astype(np.float64), sc["sc"])
    return sc, sg


def index_matched(orc, sc, case):
    """the matched set over a search index: the device's, asserted equal to the oracle's search bucket by bucket; and the older rule's reference"""

    def get(f, values, T, D0, D1, idx):
        ref = ctg.np_ct_linearize(orc, sc["tp"], sc["tc"], sc["sp"], sc["sc"], case["times"], case["X"], case["Y"], 1.0, poses=(T, D0, D1))
        corr = f.correspondences(values)
        np.testing.assert_array_equal(corr, ref["corr"])
        return rs.ct_matched(sc, corr, idx), ref

    return get


def cells_matched(mp, sc, corr, bucket):
    """the matched set over a map: target point and covariance of a pair are the FP32 values of the cell slot the device names"""
    i = np.flatnonzero(corr >= 0)
    slot, place = corr[i] // mp["cap"], corr[i] % mp["cap"]
    return dict(idx=i, p=sc["sp"][i], CA=sc["sc"][i], b=mp["points"][slot, place].astype(np.float64), CB=mp["covs"][slot, place].astype(np.float64),
                bucket=np.asarray(bucket)[i], all_buckets=np.asarray(bucket), n=len(sc["sp"]), nrm=None)


def ivox_matched(mp, sc):
    def get(f, values, T, D0, D1, idx):
        want, hits, fragile = ivr.ct_on_ivox(mp["ref"], sc["sp"], sc["sc"], idx, (T, D0, D1), 1.0)
        assert fragile == []  # the cap is 2 fragile points; the inputs have none, so the pairs below are compared exactly
        corr = f.correspondences(values)
        assert _hits_to_pairs(mp["dev"], corr) == hits
        return cells_matched(mp, sc, corr, idx), want

    return get


def same_ct_bits(a, b):
    assert a["num_inliers"] == b["num_inliers"] and a["error"] == b["error"]
    for k in ("H_00", "H_01", "H_11", "b_0", "b_1"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def check_ct_case(f, case, sc, matched, family, label, min_inliers=1):
    """everything the module asserts of one CT factor at one pair of poses"""
    assert rs.points_per_thread(case["n"]) == 1 and case["n"] < 262144  # s = 9 holds below that many points
    X, Y = case["X"], case["Y"]
    values = {0: X, 1: Y}
    # the tables the kernels read
    tab, T, D0, D1, idx = f.debug_poses(values)
    table, idx_ref = ctg.time_table(case["times"])
    np.testing.assert_array_equal(idx, idx_ref)
    np.testing.assert_allclose(tab, table, rtol=0, atol=1e-15)
    for a, b in zip((T, D0, D1), ctg.ct_poses(table, X, Y)):
        assert np.abs(a - b).max() < 1e-12
    L = f.linearize(values)
    same_ct_bits(L, f.linearize(values))
    m, ref = matched(f, values, T, D0, D1, idx)
    assert L["num_inliers"] == len(m["idx"]) == ref["num_inliers"] >= min_inliers
    # the record, entry by entry
    c64, c32 = rs.ct_terms(sc, m, np.float64, T), rs.ct_draws(sc, m, T)
    g = rs.ct_gate(c32, c64, m["bucket"], D0, D1, S, m=M[family])
    rec = rs.ct_record_of(L)
    of_gate = np.abs(rec - g["S"])[1:] / np.where(g["gate"][1:] > 0, g["gate"][1:], 1.0)
    print(f"{family}: {label}: {len(m['idx'])} pairs in {len(T)} buckets, largest |device - S| / gate = {of_gate.max():.3f} on {rs.CT_NAMES[1 + int(of_gate.argmax())]}")
    ratios = rs.ct_check(rec, g, label)
    note(family, ratios, label, float(of_gate.max()))
    # the suite's older rule on the same record, kept beside the per-entry gate.  Its Gauss-Newton step compares nothing where the begin pose's
    # block is singular below the rule's own damping (the three pairs of one bucket: smallest eigenvalue 3e-10 of the largest) -- the step is
    # then the damping's, and 1 / lam times any difference of the entries; decided from the reference alone
    Hr = ctg.full_system(ref)[0]
    ctg._check_record(L, ref, step=np.linalg.eigvalsh(Hr[:6, :6])[0] > 1e-6 * np.trace(Hr) / 12)
    # error() at the linearisation point: ct_error_kernel over the kept M, against the record's error entry and its gate
    e0, n0 = f.error(values, with_inliers=True)
    assert n0 == len(m["idx"]) and e0 == f.error(values)
    r0 = np.full(rs.CT_ROW, np.nan)
    r0[1] = abs(e0 - g["S"][1]) / g["P"][1]
    note(family + " error()", r0, label, abs(e0 - g["S"][1]) / g["gate"][1])
    assert abs(e0 - g["S"][1]) <= g["gate"][1], (label, e0, g["S"][1], g["gate"][1])
    # error() at other poses: the kept correspondences and M, residuals at the moved poses
    Xe, Ye = cc.moved(X, Y)
    e1, n1 = f.error({0: Xe, 1: Ye}, with_inliers=True)
    Te = f.debug_poses({0: Xe, 1: Ye})[1]
    assert np.abs(Te - ctg.ct_poses(table, Xe, Ye)[0]).max() < 1e-12 and n1 == len(m["idx"])
    gf = rs.error_gate(rs.ct_frozen_draws(m, T, Te), rs.ct_frozen_terms(m, T, Te, np.float64), S, m=M[family + " frozen"])
    r1 = np.full(rs.CT_ROW, np.nan)
    r1[1] = abs(e1 - gf["S"]) / gf["P"]
    note(family + " frozen", r1, label, abs(e1 - gf["S"]) / gf["gate"])
    assert abs(e1 - gf["S"]) <= gf["gate"], (label, e1, gf["S"], gf["gate"])
    same_ct_bits(L, f.linearize(values))
    return L, m


def run_index_case(api, ctx, orc, world, name, min_inliers=1):
    case = CASES[name]
    sc, sg = upload(api, ctx, case, world)
    f = api.IntegratedCT_GICPFactor(0, 1, world["tg"], sg, max_correspondence_distance=1.0, times=case["times"])
    try:
        return check_ct_case(f, case, sc, index_matched(orc, sc, case), "ct", name, min_inliers) + (f.debug_poses({0: case["X"], 1: case["Y"]})[4],)
    finally:
        f.close()
        sg.close()


def test_bucket_tails(api, gpu_ctx, orc, world):
    """buckets of 1, 63, 64, 65, 255, 256, 257, 513 and 1 points in one cloud: one lane, a wavefront's edge, a block's edge, buckets of two and
    three blocks, a last block of one point"""
    _, _, idx = run_index_case(api, gpu_ctx, orc, world, "tails", 1000)
    np.testing.assert_array_equal(np.bincount(idx), cc.TAILS)


@pytest.mark.parametrize("nbk", cc.NBK)
def test_ordered_sum_edges(api, gpu_ctx, orc, world, nbk):
    """three points per bucket: each group's first row (1, 7, 8, 9 rows), a full trip of 64 rows (63, 64), the first row of a second trip with
    the other loads clamped (65, 73)"""
    _, _, idx = run_index_case(api, gpu_ctx, orc, world, f"nbk{nbk}")
    np.testing.assert_array_equal(np.bincount(idx), [3] * nbk)


def test_the_sweeps_own_times(api, gpu_ctx, orc, world):
    """the 4096 points with their own times: about a hundred uneven buckets; |omega| of the sweep is above SERIES (the closed forms)"""
    _, _, idx = run_index_case(api, gpu_ctx, orc, world, "sweep", 1001)
    sizes = np.bincount(idx)
    assert 80 <= len(sizes) <= 120 and len(set(sizes.tolist())) > 1


@pytest.mark.parametrize("name", ["slow", "equal", "registered"])
def test_series_branch_and_small_rotations(api, gpu_ctx, orc, world, name):
    """slow: a relative rotation below SERIES (the series branch of the SE(3) tables); equal: X == Y; registered: a source already in the
    world frame, R_k a milliradian from I (where an unrotated kept M moves the frozen error by 1e-4 of itself: test_record_slots_ct.py).
    The pose assertion is the check on the table; the record is the check that the kernels used it"""
    run_index_case(api, gpu_ctx, orc, world, name, 1000)


def test_a_bucket_that_matches_nothing(api, gpu_ctx, orc, world):
    """the 255-point bucket moved 1e3 m away: no pair in it, the count that of the other buckets, every entry within its gate.  (The record is
    not compared with that of the cloud without the bucket: its row is zero, but nothing here shows the row itself.)"""
    L, m, idx = run_index_case(api, gpu_ctx, orc, world, "empty-bucket", 1000)
    a, b = CASES["empty-bucket"]["far"]
    assert np.all(idx[a:b] == cc.FAR_BUCKET) and not np.any((m["idx"] >= a) & (m["idx"] < b)) and cc.FAR_BUCKET not in set(m["bucket"].tolist())
    assert L["num_inliers"] == len(m["idx"])


def test_a_non_ascending_time_vector(api, gpu_ctx, orc, world):
    _, _, idx = run_index_case(api, gpu_ctx, orc, world, "non-ascending", 500)
    assert np.any(np.diff(CASES["non-ascending"]["times"]) < 0) and np.all(np.diff(idx) >= 0)


# ---- the same over a device iVox --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", [False, True], ids=["unary", "binary"])
@pytest.mark.parametrize("n", [1, 65, 257, 4096])
def test_rigid_gicp_record_over_the_map(api, gpu_ctx, world, ivox, n, binary):
    """IntegratedGICPFactor over the map, the first n points of the scan at the sweep's begin pose: target point and covariance of every pair
    from the cell slot the device names"""
    sc = dict(sp=world["p"][:n], sc=world["covs"][:n], T=cc.poses()[0])
    sg = api.PointCloudGPU.clone(sc["sp"], sc["sc"], ctx=gpu_ctx)
    values, target = grs.poses(sc, binary)
    f = api.IntegratedGICPFactor(target, 1, ivox["dev"], sg, max_correspondence_distance=1.0)
    T = f.calc_delta(values)
    L = f.linearize(values)
    grs.same_bits(L, f.linearize(values))
    corr = f.correspondences(values)
    hits, fragile = ivr.search_all(ivox["ref"], ivr.transform_q(T, sc["sp"]), 1.0)
    assert fragile == []
    assert _hits_to_pairs(ivox["dev"], corr) == hits
    m = cells_matched(ivox, sc, corr, np.zeros(n, dtype=np.int64))
    assert n < 4096 or len(m["idx"]) > 1000
    check_source_frame_record(L, sc, m, "gicp", T, binary, f"gicp over the map, n {n} binary {binary}")
    f.close()
    sg.close()


@pytest.mark.parametrize("name", ["tails", "sweep"])
def test_ct_record_over_the_map(api, gpu_ctx, world, ivox, name):
    case = CASES[name]
    sc, sg = upload(api, gpu_ctx, case, world)
    f = api.IntegratedCT_GICPFactor(0, 1, ivox["dev"], sg, target_tree=ivox["dev"], max_correspondence_distance=1.0, times=case["times"])
    try:
        check_ct_case(f, case, sc, ivox_matched(ivox, sc), "ivox ct", name + " over the map", 500)
    finally:
        f.close()
        sg.close()


def test_the_margins_hold():
    """runs last: every family's m keeps a factor 2 over the worst |device - S_E| / P_E this run measured, and is at most 8.  The rigid factor
    over the map is the GICP family of tests/test_gpu_record_slots.py, with its m"""
    for family, (worst, j, label) in WORST.items():
        print(f"{family}: worst |device - S| / P = {worst:.3f} on entry {j} ({rs.CT_NAMES[j]}) in '{label}'; m = {M[family]}")
        assert 2.0 * worst <= M[family] <= rs.M_MAX, (family, worst, j, label)
    if "gicp" not in grs.WORST:
        return
    worst, j, label = grs.WORST["gicp"]
    print(f"gicp (over the map among its cases): worst |device - S| / P = {worst:.3f} on slot {j} ({rs.SLOT_NAMES[j]}) in '{label}'; m = {grs.M['gicp']}")
    assert 2.0 * worst <= grs.M["gicp"] <= rs.M_MAX, (worst, j, label)
