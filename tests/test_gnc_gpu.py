"""Device GNC global registration (glim_amd_gnc_align / _align_fpfh / _debug_trace) against the NumPy restatement (tests/gnc_restatement.py),
whose docstring derives the gates.

Per step, teacher-forced: iteration k of the device trace is compared with the restatement's step from the DEVICE's pose k - 1 at the device's
mu_k, so that rounding does not compound and the gate is a single step's.  Condition on the input, asserted on the restatement: S / gap <= 100 at
every step.  The list, c_s / c_t and D2 are compared exactly (the restatement sums the centroids in the documented tree).

Measured on an MI355X, worst error / gate: 3.4e-5 over the 64 iterations of the 2 851-entry lists, 3.6e-3 on the 3-entry list (the largest)."""
import subprocess

import numpy as np
import pytest

import gnc_restatement as G
import ransac_restatement as R
from registration_cases import described_crops, make_case, room_points, write_drop_in_case
from registration_cases import result_bytes as _result_bytes
from registration_cases import upload as _upload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    """Not closed by hand, as in the other GPU test modules: Context.__del__ sees to it once every child is gone."""
    from glim_amd import api

    return api.Context(0, 1)


def _params(**kw):
    from glim_amd import api

    return api.GncParams(**kw)


@pytest.fixture(scope="module")
def cases(ctx):
    """dof 6: the planted motion of the RANSAC tests; dof 4: the same with zero pitch"""
    out = {}
    for dof, pitch in ((6, 0.25), (4, 0.0)):
        c = make_case(room_points(3001, 21), seed=5, clutter=2000, extent=6.0, pitch=pitch)
        c["clouds"] = _upload(ctx, c)
        out[dof] = c
    return out


def check_teacher_forced(case, tr, dof, expect_iterations):
    """every iteration of the trace against the restatement's step from the device's previous pose; returns (worst ratio to a gate, summed gates)"""
    P, Q = G.points_of(tr["list"], case["target"], case["source"])
    n = len(P)
    k_run = tr["result"].iterations_run
    assert k_run == expect_iterations == len(tr["mu"])
    T_prev = np.eye(4)[:3]
    worst = 0.0
    sum_r = sum_t = 0.0
    worst_cond = 0.0
    worst_each = np.zeros(4)
    for k in range(k_run):
        st = G.step(P, Q, T_prev, tr["mu"][k], dof)
        worst_cond = max(worst_cond, st["S"] / st["gap"])
        assert st["S"] / st["gap"] <= 100.0, (k, st["S"] / st["gap"])  # the condition on the input
        g_r, g_t, g_w, g_c = G.step_gates(st, n)
        T = tr["poses"][k]
        e = (R.rotation_angle(st["T"][:3, :3], T[:, :3]) / g_r, np.linalg.norm(st["T"][:3, 3] - T[:, 3]) / g_t,
             abs(tr["W"][k] - st["W"]) / g_w, abs(tr["cost"][k] - st["cost"]) / g_c)
        assert max(e) <= 1.0, (k, e)
        worst = max(worst, max(e))
        worst_each = np.maximum(worst_each, e)
        sum_r += g_r
        sum_t += g_t
        T_prev = T
    print(f"dof {dof}, list {n}, {k_run} iterations: worst error / gate {worst:.3e} (rotation, translation, W, cost: "
          f"{worst_each[0]:.2e} {worst_each[1]:.2e} {worst_each[2]:.2e} {worst_each[3]:.2e}), worst S / gap {worst_cond:.2f}")
    return worst, sum_r, sum_t


def check_schedule(tr, prm):
    """mu_0 = D2 and the division every fourth iteration, in the device's own numbers (the restatement applies the same two statements)"""
    mu_min = G.mu_min_of(tr["D2"], prm.max_corr_dist)
    mu = tr["D2"]
    for k in range(len(tr["mu"])):
        assert tr["mu"][k] == mu, k
        if k % 4 == 3 and mu > mu_min:
            mu = max(mu / prm.div_factor, mu_min)


def check_list_and_frame(case, tr, prm):
    lst = G.select(case["target"], case["source"], case["nearest"], prm.seed, prm.max_init_samples)
    info = tr["result"].info
    assert info["num_correspondences"] == len(lst)
    kept = 0
    if prm.tuple_check:
        lst, kept, passed, margin = G.tuples(lst, case["target"], case["source"], prm.seed, prm.tuple_thresh, prm.max_num_tuples)
        print(f"tuples: {passed} trials pass, {kept} kept, smallest edge margin {margin:.3e}")
    assert info["num_tuples"] == kept and info["list_length"] == len(lst)
    assert np.array_equal(tr["list"], lst)
    if len(lst) >= 3:
        c_s, c_t, D2 = G.frame(*G.points_of(lst, case["target"], case["source"]))
        assert tr["c_s"].tobytes() == c_s.tobytes() and tr["c_t"].tobytes() == c_t.tobytes() and tr["D2"] == D2
    return lst


@pytest.mark.parametrize("dof", [6, 4])
def test_per_step_parity_teacher_forced_and_the_planted_motion(cases, dof):
    from glim_amd import api

    case = cases[dof]
    prm = _params(seed=11, dof=dof)
    tr = api.gnc_debug_trace(*case["clouds"], case["nearest"], prm)
    lst = check_list_and_frame(case, tr, prm)
    check_schedule(tr, prm)
    _, sum_r, sum_t = check_teacher_forced(case, tr, dof, 64)
    # the weights of the last iteration are those of the pose before it
    P, Q = G.points_of(lst, case["target"], case["source"])
    w = G.step(P, Q, tr["poses"][62], tr["mu"][63], dof)["w"]
    assert np.allclose(tr["weights"], w, rtol=1e-9, atol=1e-300) and tr["result"].info["mu_final"] == tr["mu"][63]
    assert tr["result"].info["weight_sum"] == tr["W"][63] and tr["result"].info["cost"] == tr["cost"][63]
    # recovers the planted motion: no worse than the restatement's free-running result on the same list by more than 1 % + the summed step gates
    free = G.run(P, Q, dof)
    M = case["M"]
    T = tr["result"].T_target_source
    err_r, err_t = R.rotation_angle(M[:3, :3], T[:3, :3]), np.linalg.norm(M[:3, 3] - T[:3, 3])
    ref_r, ref_t = R.rotation_angle(M[:3, :3], free["T"][:3, :3]), np.linalg.norm(M[:3, 3] - free["T"][:3, 3])
    print(f"dof {dof}: device error {err_r:.3e} rad {err_t:.3e} m, restatement free-running {ref_r:.3e} rad {ref_t:.3e} m")
    assert free["iterations_run"] == 64 and err_r <= 1.01 * ref_r + sum_r and err_t <= 1.01 * ref_t + sum_t
    far = float(np.linalg.norm(case["source"].astype(np.float64), axis=1).max())
    planted, _ = G.inliers(M, case["target"], case["source"], 1.0, 0.0)
    assert tr["result"].inlier_rate >= 0.9 * planted / len(case["source"]) and planted >= 2500 and far > 0


def test_planted_motion_with_60_percent_redirected_and_2_cm_noise(ctx):
    """the harder input the issue quotes: outlier leakage costs a few milliradians, in the restatement as on the device"""
    from glim_amd import api

    case = make_case(room_points(3001, 21), seed=5, clutter=2000, extent=6.0, redirected=0.6, unmatched=0.05, noise=0.02)
    prm = _params(seed=11)
    tr = api.gnc_debug_trace(*_upload(ctx, case), case["nearest"], prm)
    lst = check_list_and_frame(case, tr, prm)
    _, sum_r, sum_t = check_teacher_forced(case, tr, 6, 64)
    P, Q = G.points_of(lst, case["target"], case["source"])
    free = G.run(P, Q, 6)
    M, T = case["M"], tr["result"].T_target_source
    err_r, err_t = R.rotation_angle(M[:3, :3], T[:3, :3]), np.linalg.norm(M[:3, 3] - T[:3, 3])
    ref_r, ref_t = R.rotation_angle(M[:3, :3], free["T"][:3, :3]), np.linalg.norm(M[:3, 3] - free["T"][:3, 3])
    print(f"device error {err_r:.3e} rad {err_t:.3e} m, restatement free-running {ref_r:.3e} rad {ref_t:.3e} m")
    assert err_r <= 1.01 * ref_r + sum_r and err_t <= 1.01 * ref_t + sum_t and ref_r < 1e-2 and ref_t < 5e-2
    planted, _ = G.inliers(M, case["target"], case["source"], 1.0, 0.0)
    assert tr["result"].inlier_rate >= 0.9 * planted / 3001


def test_tuple_rule_on_zero_length_edges_and_repeated_entries(ctx):
    """12 exact pairs, entries 0 and 1 the same point pair: with tuple_thresh 0 every trial of three distinct entries passes but those that hold
    both (an edge of length 0 on both sides); the list is the restatement's, duplicates and order included, also with the stop at 7 tuples"""
    from glim_amd import api

    src = np.random.default_rng(3).uniform(-5, 5, (12, 3)).astype(np.float32)
    src[1] = src[0]
    tgt = src.copy()
    near = np.arange(12, dtype=np.int32)
    clouds = api.PointCloudGPU.clone(tgt, ctx=ctx), api.PointCloudGPU.clone(src, ctx=ctx)
    case = {"source": src, "target": tgt, "nearest": near}
    for max_tuples in (10 ** 6, 7):
        prm = _params(seed=5, tuple_check=True, tuple_thresh=0.0, max_num_tuples=max_tuples, max_iterations=2)
        tr = api.gnc_debug_trace(*clouds, near, prm)
        lst = check_list_and_frame(case, tr, prm)
        trios = lst[:, 0].reshape(-1, 3)
        assert len(trios) == tr["result"].info["num_tuples"] > 0 and not np.any(np.sum(trios <= 1, axis=1) == 2)  # never 0 and 1 together
        assert len(np.unique(lst[:, 0])) < len(lst)  # repeated entries stay
    assert len(trios) == 7
    everything = G.tuples(G.select(tgt, src, near, 5, 5000), tgt, src, 5, 0.0, 10 ** 6)
    distinct = int(np.sum([len({R.sample_hash(6, 3 * j + k) % 12 for k in range(3)}) == 3 for j in range(1200)]))
    assert 7 < everything[2] < distinct  # the zero-length rule removed trials that three distinct entries alone would have passed


@pytest.mark.parametrize("samples,tuple_check,max_tuples", [(1000, False, 1000), (10000, False, 1000), (1000, True, 100), (10000, True, 1000),
                                                            (10000, True, 10 ** 6)])
def test_list_and_scale_are_the_restatement_s_exactly(cases, samples, tuple_check, max_tuples):
    from glim_amd import api

    case = cases[6]
    prm = _params(seed=23, max_init_samples=samples, tuple_check=tuple_check, tuple_thresh=0.9, max_num_tuples=max_tuples, max_iterations=4)
    tr = api.gnc_debug_trace(*case["clouds"], case["nearest"], prm)
    lst = check_list_and_frame(case, tr, prm)
    info = tr["result"].info
    if samples < 3001:
        assert info["num_correspondences"] < samples  # the draws repeat and some candidates are unmatched
    if tuple_check:
        reached = info["num_tuples"] == max_tuples
        assert reached == (max_tuples <= 1000) and len(lst) == 3 * info["num_tuples"] and info["num_tuples"] > 0
    check_teacher_forced(case, tr, 6, 4)


def test_result_is_the_last_trace_record_scored_by_ransac_s_rule(cases):
    from glim_amd import api

    case = cases[6]
    prm = _params(seed=11, inlier_voxel_resolution=1.0)
    tr = api.gnc_debug_trace(*case["clouds"], case["nearest"], prm)
    r = api.gnc_align(*case["clouds"], case["nearest"], prm)
    assert _result_bytes(r) == _result_bytes(tr["result"]) and r.info == tr["result"].info
    assert r.T_target_source[:3].tobytes() == np.ascontiguousarray(tr["poses"][-1]).tobytes() and r.T_target_source[3].tolist() == [0, 0, 0, 1]
    assert (r.iterations_run, r.best_iteration) == (64, 63)
    sp = case["source"].astype(np.float64)
    _, delta = R.pose_gates(1.0, float(np.linalg.norm(sp, axis=1).max()), float(np.linalg.norm(case["target"].astype(np.float64), axis=1).max()))
    count, ambiguous = G.inliers(r.T_target_source, case["target"], case["source"], 1.0, 1e-9 + delta)
    print(f"inliers {r.num_inliers}, restatement {count} +- {ambiguous}")
    assert abs(r.num_inliers - count) <= ambiguous and r.inlier_rate == r.num_inliers / 3001 and r.num_inliers >= 2500
    # the pose does not depend on the resolution, the count does
    r2 = api.gnc_align(*case["clouds"], case["nearest"], _params(seed=11, inlier_voxel_resolution=0.25))
    assert r2.T_target_source.tobytes() == r.T_target_source.tobytes()
    count2, amb2 = G.inliers(r.T_target_source, case["target"], case["source"], 0.25, 1e-9 + delta)
    assert abs(r2.num_inliers - count2) <= amb2


@pytest.mark.parametrize("length", [0, 1, 2, 3, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2049])
def test_list_lengths_at_which_the_block_can_go_wrong(ctx, length):
    """lengths around a wavefront, around the block (512 lanes) and around twice the block; 1023 .. 1025 are the issue's"""
    from glim_amd import api

    case = make_case(room_points(3001, 21)[:2100], seed=70 + length, clutter=50, extent=6.0, redirected=0.3, unmatched=0.0)
    # (length 3: a draw whose triangle meets the S / gap condition, chosen on the CPU -- the generator's own draw for 3 is nearly collinear)
    keep = np.sort(np.random.default_rng(202 if length == 3 else length).permutation(2100)[:length])
    near = np.full(2100, -1, dtype=np.int32)
    near[keep] = case["nearest"][keep]
    case["nearest"] = near
    prm = _params(seed=1, max_iterations=8, max_init_samples=2100)
    tr = api.gnc_debug_trace(*_upload(ctx, case), near, prm)
    lst = check_list_and_frame(case, tr, prm)
    assert len(lst) == length
    r = tr["result"]
    if length < 3:
        assert (r.best_iteration, r.iterations_run, r.num_inliers, r.inlier_rate) == (-1, 0, 0, 0.0) and np.array_equal(r.T_target_source, np.eye(4))
        return
    check_schedule(tr, prm)
    check_teacher_forced(case, tr, 6, 8)
    assert np.all(np.isfinite(r.T_target_source)) and (r.best_iteration, r.iterations_run) == (7, 8)
    if length >= 63:
        assert R.rotation_angle(case["M"][:3, :3], r.T_target_source[:3, :3]) < 0.2  # (8 iterations: mu is still large, the outliers still pull)


def test_non_finite_points_unmatched_lists_an_empty_target_and_collinear_points(ctx):
    from glim_amd import api

    case = make_case(room_points(3001, 21)[:500], seed=50, clutter=100, extent=6.0, redirected=0.0, unmatched=0.0)
    src, tgt = case["source"].copy(), case["target"].copy()
    src[[5, 17]] = np.nan
    src[40, 1] = np.inf
    src[[60, 61]] = [3.0e6, 0.0, 0.0]     # finite, outside the key range at res 1: unmatched below (they would swamp the sums), never inliers
    tgt[7, 2] = np.nan                     # the partner of a finite source point
    tgt[550] = np.nan                      # clutter
    case["source"], case["target"] = src, tgt
    case["nearest"][[60, 61]] = -1
    clouds = _upload(ctx, case)
    prm = _params(seed=8, max_iterations=16)
    tr = api.gnc_debug_trace(*clouds, case["nearest"], prm)
    lst = check_list_and_frame(case, tr, prm)
    assert not np.isin([5, 7, 17, 40, 60, 61], lst[:, 0]).any() and len(lst) == 494
    check_teacher_forced(case, tr, 6, 16)
    r = tr["result"]
    assert np.all(np.isfinite(r.T_target_source)) and 480 <= r.num_inliers <= 495  # 3 not finite, 2 out of range: never counted
    # nothing matched
    none = np.full(500, -1, dtype=np.int32)
    r = api.gnc_align(*clouds, none, prm)
    assert (r.best_iteration, r.num_inliers, r.inlier_rate, r.iterations_run) == (-1, 0, 0.0, 0) and np.array_equal(r.T_target_source, np.eye(4))
    assert r.info["num_correspondences"] == 0 and r.info["list_length"] == 0
    # an empty target
    empty = api.PointCloudGPU.clone(np.zeros((0, 3), dtype=np.float32), ctx=ctx)
    r = api.gnc_align(empty, clouds[1], none, prm)
    assert (r.best_iteration, r.iterations_run) == (-1, 0) and np.array_equal(r.T_target_source, np.eye(4))
    # collinear listed points, dof 6: finite numbers or "no estimate", never a NaN pose
    line = (np.arange(40, dtype=np.float32)[:, None] * np.array([[0.5, 0.25, 0.125]], dtype=np.float32))
    tl, sl = api.PointCloudGPU.clone(line + np.float32(1.0), ctx=ctx), api.PointCloudGPU.clone(line, ctx=ctx)
    r = api.gnc_align(tl, sl, np.arange(40, dtype=np.int32), _params(dof=6))
    assert np.all(np.isfinite(r.T_target_source)) and np.isfinite(r.inlier_rate) and (r.best_iteration == r.iterations_run - 1)
    # one point repeated: D2 = 0, the weights are 0 / 0 -- no iteration completes
    same = np.ones((10, 3), dtype=np.float32)
    ts, ss = api.PointCloudGPU.clone(same, ctx=ctx), api.PointCloudGPU.clone(same, ctx=ctx)
    r = api.gnc_align(ts, ss, np.arange(10, dtype=np.int32), _params())
    assert (r.best_iteration, r.iterations_run, r.inlier_rate) == (-1, 0, 0.0) and np.array_equal(r.T_target_source, np.eye(4))


def test_two_calls_and_a_second_context_return_the_same_bytes(cases):
    from glim_amd import api

    case = cases[6]
    for prm in (_params(seed=11), _params(seed=11, tuple_check=True, max_num_tuples=500, max_iterations=16)):
        a = api.gnc_align(*case["clouds"], case["nearest"], prm)
        b = api.gnc_align(*case["clouds"], case["nearest"], prm)
        assert a.best_iteration >= 0 and _result_bytes(a) == _result_bytes(b) and a.info == b.info
        other = api.Context(0, 1)
        clouds = _upload(other, case)
        try:
            c = api.gnc_align(*clouds, case["nearest"], prm)
            assert _result_bytes(a) == _result_bytes(c) and a.info == c.info
        finally:
            for cl in clouds:
                cl.close()
            other.close()


def test_profile_reports_the_stages_and_leaves_no_state(cases):
    """glim_amd_gnc_profile on the dof-6 case, two timed calls, without and with the tuple test: the five stage times are finite and not negative,
    every stage that always launches something takes time, and gnc_align returns the same bytes and info before and after.  No wall-clock
    threshold: the times are only looked at."""
    from glim_amd import api

    case = cases[6]
    for prm in (_params(seed=11), _params(seed=11, tuple_check=True, max_num_tuples=500, max_iterations=16)):
        args = (*case["clouds"], case["nearest"], prm)
        before = api.gnc_align(*args)
        prof = api.gnc_profile(*args, iters=2)
        print(prof)
        assert len(prof) == 5 and all(np.isfinite(v) and v >= 0 for v in prof.values())
        for k in ("select_us", "gather_and_solve_us", "table_us", "score_us"):
            assert prof[k] > 0, k
        after = api.gnc_align(*args)
        assert before.best_iteration >= 0 and _result_bytes(before) == _result_bytes(after) and before.info == after.info


def test_invalid_arguments_with_real_handles(ctx, cases):
    from glim_amd import api

    t, s = cases[6]["clouds"]
    near = cases[6]["nearest"]
    nan, inf = float("nan"), float("inf")
    for kw in ({"dof": 5}, {"max_iterations": 0}, {"max_init_samples": 0}, {"tuple_check": True, "max_num_tuples": 0}, {"div_factor": 1.0},
               {"div_factor": inf}, {"div_factor": nan}, {"tuple_thresh": nan}, {"inlier_voxel_resolution": 0.0}, {"inlier_voxel_resolution": inf},
               {"max_corr_dist": nan}, {"max_corr_dist": inf}):
        with pytest.raises(api.GlimAmdError) as e:
            api.gnc_align(t, s, near, _params(**kw))
        assert e.value.code == -1, kw
    api.gnc_align(t, s, near, _params(max_num_tuples=0, max_iterations=1))  # (max_num_tuples is not looked at without tuple_check)
    for bad in (t.size(), -2):
        wrong = near.copy()
        wrong[10] = bad
        with pytest.raises(api.GlimAmdError) as e:
            api.gnc_align(t, s, wrong, _params())
        assert e.value.code == -1
    other = api.Context(0, 1)
    foreign = api.PointCloudGPU.clone(cases[6]["target"], ctx=other)
    try:
        with pytest.raises(api.GlimAmdError) as e:
            api.gnc_align(foreign, s, near, _params())
        assert e.value.code == -1
        f = api.FPFHFeatures.from_host(np.zeros((5, 33), dtype=np.float32), ctx=ctx)
        with pytest.raises(api.GlimAmdError) as e:
            api.gnc_align_fpfh(t, s, f, f, _params())  # descriptor counts that are not the cloud sizes
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
    prm = _params(seed=4)
    a = api.gnc_align(tc, sc, nearest, prm)
    b = api.gnc_align_fpfh(tc, sc, tf, sf, prm, reciprocal=reciprocal)
    assert a.info["num_correspondences"] == int(np.sum(nearest >= 0)) >= 3
    assert a.best_iteration >= 0 and _result_bytes(a) == _result_bytes(b) and a.info == b.info


def test_cpp_drop_in_returns_the_python_result(ctx, described, tmp_path):
    """tests/cpp/test_gnc.cpp calls gtsam_points::estimate_pose_gnc (the drop-in, the modal's argument list and fields) on the two crops and their
    descriptors and compares with what this process got through gnc_align_fpfh on the same inputs."""
    from glim_amd import api
    from test_gnc import build_cpp

    (tc, tf, _), (sc, sf, _) = described["target"], described["source"]
    prm = _params(seed=77, dof=4, max_init_samples=10000, max_num_tuples=5000)
    r = api.gnc_align_fpfh(tc, sc, tf, sf, prm, reciprocal=True)
    path = tmp_path / "case.bin"
    write_drop_in_case(path, described, 4, 77, r)
    out = subprocess.run([build_cpp(tmp_path), str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "test_gnc OK (1537 x 1000 points, dof 4)" in out.stdout, out.stdout + out.stderr
