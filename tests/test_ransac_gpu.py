"""Device RANSAC global registration (glim_amd_ransac_align / _align_fpfh / _debug_hypotheses) against the NumPy restatement
(tests/ransac_restatement.py), whose docstring derives the gates.

Per hypothesis: samples equal; status equal wherever the restatement's edge and collinearity margins exceed 1e-9 (at most 1 % of the hypotheses
may fall inside, asserted on the restatement); poses within the gates on cond <= 100; inliers within [count - ambiguous, count + ambiguous], and
at most 1 % of the hypotheses may have ambiguous > 0 (a condition on the input, asserted on the restatement; the seeds were chosen on the CPU).
The result rule is checked exactly, on the device's own debug records."""
import subprocess

import numpy as np
import pytest

import ransac_restatement as R
from registration_cases import described_crops, make_case, room_points, write_drop_in_case
from registration_cases import result_bytes as _result_bytes
from registration_cases import upload as _upload

pytestmark = pytest.mark.gpu

ROUND = 1024  # the library's round size (ransac.hip): the shapes below straddle it
TILE = 2048   # source points of a scoring block
RULE_SEED = 14


@pytest.fixture(scope="module")
def ctx():
    """Not closed by hand, as in the other GPU test modules: Context.__del__ sees to it once every child is gone."""
    from glim_amd import api

    return api.Context(0, 1)


def parity_case():
    return make_case(room_points(3001, 21), seed=5, clutter=2000, extent=6.0)


def global_table_case():
    rng = np.random.default_rng(31)
    return make_case(rng.uniform(-20, 20, (3001, 3)).astype(np.float32), seed=6, clutter=16999, extent=25.0)


def result_rule_case():
    """a noisy copy (sigma 8 cm) and 60 % wrong correspondences: the counts of the good hypotheses differ, so that the running maximum still rises
    in the third round (seed chosen on the CPU; the tests assert it on the device's records)"""
    return make_case(room_points(3001, 21), seed=RULE_SEED, clutter=2000, extent=6.0, redirected=0.6, unmatched=0.0, noise=0.08)


def _params(**kw):
    from glim_amd import api

    return api.RansacParams(**kw)


def check_restatement_conditions(ref):
    """the conditions on the INPUT under which the comparison below is exact; True when they hold"""
    n = len(ref["status"])
    inside = np.minimum(ref["edge_margin"], ref["col_margin"]) <= 1e-9
    amb = ref["ambiguous"] > 0
    print(f"hypotheses {n}: ok {np.sum(ref['status'] == 0)}, inside the status margins {inside.sum()}, ambiguous {amb.sum()}, "
          f"cond <= 100 among ok {np.sum((ref['status'] == 0) & (ref['cond'] <= 100))}")
    return inside.mean() <= 0.01 and amb.mean() <= 0.01 and np.sum((ref["status"] == 0) & (ref["cond"] <= 100)) >= 50


def _check_parity(got, ref):
    assert check_restatement_conditions(ref)
    assert np.array_equal(got["samples"], ref["samples"])
    decided = np.minimum(ref["edge_margin"], ref["col_margin"]) > 1e-9
    assert np.array_equal(got["status"][decided], ref["status"][decided])
    both_ok = (got["status"] == 0) & (ref["status"] == 0)
    worst_r = worst_t = 0.0
    for j in np.nonzero(both_ok & (ref["cond"] <= 100))[0]:
        T = got["poses"][j].reshape(3, 4)
        g_r, g_t = R.pose_gates(ref["cond"][j], ref["far_source"], ref["far_target"])
        worst_r = max(worst_r, R.rotation_angle(ref["T"][j][:3, :3], T[:, :3]) / g_r)
        worst_t = max(worst_t, np.linalg.norm(ref["T"][j][:3, 3] - T[:, 3]) / g_t)
    diff = np.abs(got["inliers"][both_ok].astype(np.int64) - ref["inliers"][both_ok])
    print(f"worst rotation / gate {worst_r:.3e}, worst translation / gate {worst_t:.3e}, inlier counts that differ {np.sum(diff > 0)}, "
          f"largest ok count {ref['inliers'].max()}")
    assert worst_r <= 1.0 and worst_t <= 1.0
    assert (diff <= ref["ambiguous"][both_ok]).all()
    bad = got["status"] != 0
    assert not got["inliers"][bad].any() and (got["poses"][bad] == np.eye(4)[:3].ravel()).all()
    assert ref["inliers"].max() >= 2500  # the true motion is among the hypotheses: the counts compared are not all small


@pytest.fixture(scope="module")
def parity(ctx):
    case = parity_case()
    case["clouds"] = _upload(ctx, case)
    return case


@pytest.mark.parametrize("dof", [6, 4])
def test_per_hypothesis_parity_with_the_table_in_lds(parity, dof):
    from glim_amd import api

    prm = _params(seed=11, dof=dof, inlier_voxel_resolution=1.0)
    got = api.ransac_debug_hypotheses(*parity["clouds"], parity["nearest"], prm, 0, 1500)
    assert got["table_in_lds"] == 1 and got["table_slots"] <= 8192
    ref = R.hypotheses(parity["target"], parity["source"], parity["nearest"], 11, 0.5, 1.0, dof, 0, 1500)
    _check_parity(got, ref)


def test_per_hypothesis_parity_with_the_table_in_global_memory(ctx):
    from glim_amd import api

    case = global_table_case()
    prm = _params(seed=12, dof=6, inlier_voxel_resolution=0.5)
    got = api.ransac_debug_hypotheses(*_upload(ctx, case), case["nearest"], prm, 0, 1500)
    assert got["table_in_lds"] == 0 and got["table_slots"] > 8192
    ref = R.hypotheses(case["target"], case["source"], case["nearest"], 12, 0.5, 0.5, 6, 0, 1500)
    _check_parity(got, ref)


def test_both_table_forms_count_the_same_on_one_input(parity):
    from glim_amd import _lib, api

    prm = _params(seed=11, dof=6)
    a = api.ransac_debug_hypotheses(*parity["clouds"], parity["nearest"], prm, 3, 1500)  # (first = 3: a window that does not start a round)
    assert _lib.lib().glim_amd_debug_ransac_max_lds_slots(0) == 0
    try:
        b = api.ransac_debug_hypotheses(*parity["clouds"], parity["nearest"], prm, 3, 1500)
    finally:
        _lib.lib().glim_amd_debug_ransac_max_lds_slots(8192)
    assert a["table_in_lds"] == 1 and b["table_in_lds"] == 0 and a["table_slots"] == b["table_slots"]
    for k in ("samples", "status", "poses", "inliers"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["inliers"].max() >= 2500
    whole = api.ransac_debug_hypotheses(*parity["clouds"], parity["nearest"], prm, 0, 1503)
    for k in ("samples", "status", "poses", "inliers"):
        assert whole[k][3:].tobytes() == a[k].tobytes(), k  # a hypothesis does not depend on where its round starts


def _check_result_rule(clouds, nearest, n_source, records, prm):
    from glim_amd import api

    r = api.ransac_align(*clouds, nearest, prm)
    best, count, run = R.sequential_result(records["status"], records["inliers"], n_source, prm.early_stop_inlier_rate, prm.max_iterations)
    print(f"rate {prm.early_stop_inlier_rate:.6f}, max {prm.max_iterations}: best {r.best_iteration}, inliers {r.num_inliers}, run {r.iterations_run}")
    assert (r.best_iteration, r.num_inliers, r.iterations_run) == (best, count, run)
    assert r.inlier_rate == (count / n_source if best >= 0 else 0.0)
    want = records["poses"][best].reshape(3, 4) if best >= 0 else np.eye(4)[:3]
    assert r.T_target_source[:3].tobytes() == np.ascontiguousarray(want).tobytes() and r.T_target_source[3].tolist() == [0, 0, 0, 1]
    return r


@pytest.fixture(scope="module")
def rule(ctx):
    from glim_amd import api

    case = result_rule_case()
    case["clouds"] = _upload(ctx, case)
    case["records"] = api.ransac_debug_hypotheses(*case["clouds"], case["nearest"], _params(seed=3), 0, 2500)
    return case


def stop_points(records):
    """(index < 1024 that is not 0, index > 1024) at which the running maximum of the ok counts rises, or None: where an early stop can be put"""
    c = np.where(records["status"] == 0, records["inliers"], -1)
    run = np.maximum.accumulate(c)
    rises = np.nonzero((c > np.concatenate([[-1], run[:-1]])) & (c > 0))[0]
    early = [i for i in rises if 0 < i < ROUND and i % ROUND != 0]
    late = [i for i in rises if i > ROUND and i % ROUND != 0]
    return (early[-1] if early else None), (late[0] if late else None)


def test_result_rule_with_a_stop_in_the_middle_of_the_first_round(rule):
    early, _ = stop_points(rule["records"])
    assert early is not None
    n = len(rule["source"])
    rate = (int(rule["records"]["inliers"][early]) - 0.5) / n
    r = _check_result_rule(rule["clouds"], rule["nearest"], n, rule["records"], _params(seed=3, max_iterations=2500, early_stop_inlier_rate=rate))
    assert r.best_iteration == early and r.iterations_run == early + 1


def test_result_rule_with_a_stop_in_a_later_round(rule):
    _, late = stop_points(rule["records"])
    assert late is not None
    n = len(rule["source"])
    rate = (int(rule["records"]["inliers"][late]) - 0.5) / n
    r = _check_result_rule(rule["clouds"], rule["nearest"], n, rule["records"], _params(seed=3, max_iterations=2500, early_stop_inlier_rate=rate))
    assert r.best_iteration == late and r.iterations_run == late + 1


def test_result_rule_without_a_stop_and_with_one_iteration(rule):
    n = len(rule["source"])
    r = _check_result_rule(rule["clouds"], rule["nearest"], n, rule["records"], _params(seed=3, max_iterations=2500, early_stop_inlier_rate=2.0))
    assert r.iterations_run == 2500 and r.best_iteration >= 0
    _check_result_rule(rule["clouds"], rule["nearest"], n, rule["records"], _params(seed=3, max_iterations=1500, early_stop_inlier_rate=2.0))
    r = _check_result_rule(rule["clouds"], rule["nearest"], n, rule["records"], _params(seed=3, max_iterations=1, early_stop_inlier_rate=2.0))
    assert r.iterations_run == 1


def test_two_calls_and_a_second_context_return_the_same_bytes(parity):
    from glim_amd import api

    prm = _params(seed=11, max_iterations=1500, early_stop_inlier_rate=2.0)
    a = api.ransac_align(*parity["clouds"], parity["nearest"], prm)
    b = api.ransac_align(*parity["clouds"], parity["nearest"], prm)
    assert a.best_iteration >= 0 and _result_bytes(a) == _result_bytes(b)
    other = api.Context(0, 1)
    clouds = _upload(other, parity)
    try:
        c = api.ransac_align(*clouds, parity["nearest"], prm)
        assert _result_bytes(a) == _result_bytes(c)
    finally:
        for cl in clouds:
            cl.close()
        other.close()


def test_profile_reports_the_round_and_leaves_no_state(parity):
    """glim_amd_ransac_profile on the parity case (3 001 source points: one scoring tile and a remainder; the table in LDS), two timed rounds: the
    three kernel times are finite and positive, the table is the one ransac_debug_hypotheses reports on the same arguments, the LDS cut moves it
    to global memory, and ransac_align returns the same bytes before and after.  No wall-clock threshold: the times are only looked at."""
    from glim_amd import _lib, api

    prm = _params(seed=11, max_iterations=1500, early_stop_inlier_rate=2.0)
    args = (*parity["clouds"], parity["nearest"], prm)
    before = api.ransac_align(*args)
    rec = api.ransac_debug_hypotheses(*args, 0, 1)
    prof = api.ransac_profile(*args, iters=2)
    print(prof)
    for k in ("hypothesis_us", "score_us", "fold_us"):
        assert np.isfinite(prof[k]) and prof[k] > 0, k
    assert (prof["table_slots"], prof["table_in_lds"]) == (rec["table_slots"], rec["table_in_lds"]) and prof["table_in_lds"] == 1
    assert _lib.lib().glim_amd_debug_ransac_max_lds_slots(0) == 0
    try:
        cut = api.ransac_profile(*args, iters=2)
    finally:
        _lib.lib().glim_amd_debug_ransac_max_lds_slots(8192)
    assert cut["table_in_lds"] == 0 and cut["table_slots"] == prof["table_slots"]
    after = api.ransac_align(*args)
    assert before.best_iteration >= 0 and _result_bytes(before) == _result_bytes(after)


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, TILE + 1])
def test_small_and_odd_source_sizes(ctx, n):
    from glim_amd import api

    case = make_case(room_points(3001, 21)[:n], seed=40 + n, clutter=50, extent=6.0, redirected=0.0, unmatched=0.0)
    clouds = _upload(ctx, case)
    prm = _params(seed=n, max_iterations=300, early_stop_inlier_rate=2.0)
    rec = api.ransac_debug_hypotheses(*clouds, case["nearest"], prm, 0, 300)
    ref = R.hypotheses(case["target"], case["source"], case["nearest"], n, 0.5, 1.0, 6, 0, 300)
    assert np.array_equal(rec["samples"], ref["samples"])
    decided = np.minimum(ref["edge_margin"], ref["col_margin"]) > 1e-9
    assert np.array_equal(rec["status"][decided], ref["status"][decided])
    both = (rec["status"] == 0) & (ref["status"] == 0)
    assert (np.abs(rec["inliers"][both] - ref["inliers"][both]) <= ref["ambiguous"][both]).all()
    r = _check_result_rule(clouds, case["nearest"], n, rec, prm)
    if n < 3:
        assert (rec["status"] == 2).all() and r.best_iteration == -1 and r.inlier_rate == 0.0 and r.iterations_run == 300
    if n >= 63:
        # a copy up to FP32 rounding (<= 5e-7 m here) and a three-point pose of the same order: only a point that close to a voxel face can leave
        assert r.num_inliers >= 0.98 * n


def test_unmatched_non_finite_and_out_of_range_points_and_an_empty_target(ctx):
    from glim_amd import api

    case = make_case(room_points(3001, 21)[:500], seed=50, clutter=100, extent=6.0, redirected=0.0, unmatched=0.0)
    src, tgt = case["source"].copy(), case["target"].copy()
    src[[5, 17]] = np.nan
    src[40, 1] = np.inf
    src[[60, 61]] = [3.0e6, 0.0, 0.0]     # finite, outside the key range at res 1
    tgt[7, 2] = np.nan                     # the partner of a finite source point
    tgt[[90, 91]] = [0.0, -3.0e6, 0.0]
    tgt[550] = np.nan                      # clutter
    case["source"], case["target"] = src, tgt
    clouds = _upload(ctx, case)
    prm = _params(seed=8, max_iterations=1200, early_stop_inlier_rate=2.0)
    rec = api.ransac_debug_hypotheses(*clouds, case["nearest"], prm, 0, 1200)
    ref = R.hypotheses(tgt, src, case["nearest"], 8, 0.5, 1.0, 6, 0, 1200)
    assert np.array_equal(rec["samples"], ref["samples"])
    bad_src = np.isin(rec["samples"], [5, 17, 40]).any(axis=1) | (rec["samples"] == 7).any(axis=1)  # (source 7's target is NaN)
    assert bad_src.sum() >= 5 and (rec["status"][bad_src & (rec["status"] > 2)] == 4).all() and (rec["status"][bad_src] != 0).all()
    decided = np.minimum(ref["edge_margin"], ref["col_margin"]) > 1e-9
    assert np.array_equal(rec["status"][decided], ref["status"][decided])
    both = (rec["status"] == 0) & (ref["status"] == 0)
    assert (np.abs(rec["inliers"][both] - ref["inliers"][both]) <= ref["ambiguous"][both]).all()
    # 500 points, 3 not finite, 2 out of range, 3 whose partner left the occupancy set or the range: no count can exceed 495
    assert rec["inliers"].max() <= 495 and rec["inliers"].max() >= 480
    _check_result_rule(clouds, case["nearest"], 500, rec, prm)
    # nothing matched
    none = np.full(500, -1, dtype=np.int32)
    rec = api.ransac_debug_hypotheses(*clouds, none, prm, 0, 100)
    assert (rec["status"] == 1).all() and not rec["inliers"].any()
    r = api.ransac_align(*clouds, none, prm)
    assert (r.best_iteration, r.num_inliers, r.inlier_rate, r.iterations_run) == (-1, 0, 0.0, 1200) and np.array_equal(r.T_target_source, np.eye(4))
    # an empty target
    empty = api.PointCloudGPU.clone(np.zeros((0, 3), dtype=np.float32), ctx=ctx)
    r = api.ransac_align(empty, clouds[1], none, prm)
    assert (r.best_iteration, r.iterations_run) == (-1, 1200) and np.array_equal(r.T_target_source, np.eye(4))
    rec = api.ransac_debug_hypotheses(empty, clouds[1], none, prm, 0, 10)
    assert (rec["status"] == 1).all() and rec["table_slots"] == 64


def test_invalid_arguments_with_real_handles(ctx, parity):
    from glim_amd import api

    t, s = parity["clouds"]
    near = parity["nearest"]
    for kw in ({"dof": 5}, {"max_iterations": 0}, {"inlier_voxel_resolution": 0.0}, {"inlier_voxel_resolution": float("inf")},
               {"early_stop_inlier_rate": float("nan")}, {"poly_error_thresh": float("nan")}):
        with pytest.raises(api.GlimAmdError) as e:
            api.ransac_align(t, s, near, _params(**kw))
        assert e.value.code == -1, kw
    for bad in (t.size(), -2):
        wrong = near.copy()
        wrong[10] = bad
        with pytest.raises(api.GlimAmdError) as e:
            api.ransac_align(t, s, wrong, _params())
        assert e.value.code == -1
    other = api.Context(0, 1)
    foreign = api.PointCloudGPU.clone(parity["target"], ctx=other)
    try:
        with pytest.raises(api.GlimAmdError) as e:
            api.ransac_align(foreign, s, near, _params())
        assert e.value.code == -1
        f = api.FPFHFeatures.from_host(np.zeros((5, 33), dtype=np.float32), ctx=ctx)
        with pytest.raises(api.GlimAmdError) as e:
            api.ransac_align_fpfh(t, s, f, f, _params())  # descriptor counts that are not the cloud sizes
        assert e.value.code == -1
        f.close()
    finally:
        foreign.close()
        other.close()


@pytest.fixture(scope="module")
def described(ctx):
    """two overlapping crops of a room scan with normals and FPFH descriptors"""
    return described_crops(ctx)


@pytest.mark.parametrize("reciprocal", [False, True])
def test_align_fpfh_equals_align_on_the_matcher_s_correspondences(described, reciprocal):
    from glim_amd import api

    (tc, tf, _), (sc, sf, _) = described["target"], described["source"]
    nearest, _ = api.match_fpfh(tf, sf, reciprocal=reciprocal)
    prm = _params(seed=4, max_iterations=1500, early_stop_inlier_rate=2.0)
    a = api.ransac_align(tc, sc, nearest, prm)
    b = api.ransac_align_fpfh(tc, sc, tf, sf, prm, reciprocal=reciprocal)
    assert a.best_iteration >= 0 and _result_bytes(a) == _result_bytes(b)


def test_uploaded_descriptors_match_like_the_estimated_ones(ctx, described):
    from glim_amd import api

    (_, tf, _), (_, sf, _) = described["target"], described["source"]
    tu, su = api.FPFHFeatures.from_host(tf.download(), ctx=ctx), api.FPFHFeatures.from_host(sf.download(), ctx=ctx)
    assert tu.size() == 1537 and tu.download().tobytes() == tf.download().tobytes()
    for recip in (False, True):
        i0, d0 = api.match_fpfh(tf, sf, reciprocal=recip)
        i1, d1 = api.match_fpfh(tu, su, reciprocal=recip)
        assert i0.tobytes() == i1.tobytes() and d0.tobytes() == d1.tobytes()


def test_cpp_drop_in_returns_the_python_result(ctx, described, tmp_path):
    """tests/cpp/test_ransac.cpp calls gtsam_points::estimate_pose_ransac (the drop-in, the modal's argument list) on the two crops and their
    descriptors and compares with what this process got through ransac_align_fpfh on the same inputs."""
    from glim_amd import api
    from test_ransac import build_cpp

    (tc, tf, _), (sc, sf, _) = described["target"], described["source"]
    prm = _params(seed=77, dof=4)
    r = api.ransac_align_fpfh(tc, sc, tf, sf, prm)
    path = tmp_path / "case.bin"
    write_drop_in_case(path, described, 4, 77, r)
    out = subprocess.run([build_cpp(tmp_path), str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "test_ransac OK (1537 x 1000 points, dof 4)" in out.stdout, out.stdout + out.stderr
