"""VGICP fine registration on the device (include/glim_amd.h "VGICP fine registration"; glim_amd/csrc/vgicp_align.hip over vgicp_batch.hpp): every
trial record is the bits NonlinearFactorSetGPU.linearize_poses returns for a set of the same pairs at the trial's poses, the decisions are those
of tests/lm_restatement.py, and the caller's own sets, plans and resident session are left alone.

The cases were chosen on the CPU with lm_restatement.run over orc.vgicp_linearize (CPU kNN covariances rounded to FP32); "rel" below is
(e_new - e_cur) / e_cur of a trial, A an accepted and r a rejected round, as the oracle ran them there:
  small = (16, 128) 2 048 points, big = (32, 384) 12 288 points, resolutions 0.5 / 1.0, parameters max_iterations = 3 unless stated
  big/big     PERT_A  0.5: AAArrrr rel -0.958 -0.0067 +0.0063 x4   7 126 inliers;  1.0: AAAA rel -0.962 -0.0029 -0.0  10 521 inliers
  big/small   PERT_B  0.5: AAAA rel -0.979 -0.017 -0.001           1 065 inliers;  1.0: AAAA rel -0.980 -0.0054 -0.0   1 547 inliers
  small/small PERT_A  0.5: AAAA rel -0.905 -0.017 -0.0046            811 inliers;  1.0: AAAA rel -0.903 -0.0032 -0.0094 1 497 inliers
  (with surface validation the same sequences but big/big 0.5: AAAA; inliers 6 827 / 1 064 / 811 / 10 218 / 1 546 / 1 497)
  REJECT_CASE small/small PERT_B 0.5: AArrrrr rel -0.920, then +0.0259 five times (MAX_TRIALS, 1 iteration, 6 trials, 653 inliers): the
              smallest margin is 130 x the record tolerance 2e-4
  CASES       every trial of every case moves the error by more than 5e-3 of itself (smallest: 0.0168); see the list
The device's clouds carry the device's own FP32 covariances, so each test that rests on such a condition asserts it again on the oracle run it
makes itself."""
import struct
import subprocess

import numpy as np
import pytest

import align_cases
import lm_restatement as lmr
from align_cases import (BIG, MOVES, PERT_A, PERT_B, PERT_C, PERT_D, RECORD_TOL, SMALL, api_params, build_cpp, ctx, moves, packed, pair,  # noqa: F401 (ctx: a fixture)
                         same_record, same_result, vmap)
from test_gicp import POSE_TOL, clouds

pytestmark = pytest.mark.gpu
THREE = dict(max_iterations=3)
REJECT_CASE = (SMALL, 0.5, PERT_B, THREE)
# test 3: (size, resolution, perturbation, parameters) -- the oracle's trials on the CPU:
CASES = [
    (SMALL, 0.5, PERT_A, dict(relative_error_tol=5e-2)),  # AAA rel -0.905 -0.0168: CONVERGED, 2 iterations
    (SMALL, 0.5, PERT_B, THREE),                          # AArrrrr rel -0.920 +0.0259 x5: MAX_TRIALS, 1 iteration, 6 trials
    (SMALL, 1.0, PERT_C, dict(relative_error_tol=5e-2)),  # AAA rel -0.953 -0.0272: CONVERGED
    (BIG, 0.5, PERT_B, dict(relative_error_tol=5e-2)),    # AAA rel -0.969 -0.0312: CONVERGED
    (BIG, 1.0, PERT_D, dict(relative_error_tol=5e-2)),    # AAA rel -0.975 -0.0320: CONVERGED
]


def factor_set(ctx, targets, sources, flags):
    """a caller's NonlinearFactorSetGPU of the same pairs in the same order with the same flags"""
    from glim_amd import api

    fset = api.NonlinearFactorSetGPU(ctx)
    for t, s in zip(targets, sources):
        f = api.IntegratedVGICPFactorGPU(np.eye(4), 1, t, s)
        f.set_enable_surface_validation(bool(flags & api.FACTOR_SURFACE_VALIDATION))
        fset.add(f)
    return fset


def teacher_forced(fset, results, traces, T0s, p):
    """align_cases.teacher_forced with round k of the batch as ONE linearize_poses of the caller's set"""
    from glim_amd import api

    return align_cases.teacher_forced(lambda poses: fset.linearize_poses(np.stack([api.pose12(T) for T in poses])), results, traces, T0s, p)


# ---- 1. the teacher-forced trace ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sv", [False, True])
@pytest.mark.parametrize("res", [0.5, 1.0])
def test_every_trial_is_the_set_record_and_the_restatement_decision(orc, ctx, res, sv):
    from glim_amd import api

    flags = api.FACTOR_SURFACE_VALIDATION if sv else 0
    (_, (_, _, sg_big)), delta = pair(orc, ctx, BIG)
    (_, (_, _, sg_small)), _ = pair(orc, ctx, SMALL)
    vb, vs = vmap(orc, ctx, BIG, res), vmap(orc, ctx, SMALL, res)
    TA, TB = delta @ orc.se3_exp(PERT_A), delta @ orc.se3_exp(PERT_B)
    p = lmr.params(**THREE)
    # B = 1, and B = 3: mixed sizes, the big map shared by two problems
    for targets, sources, T0s in (([vb], [sg_big], [TA]), ([vb, vb, vs], [sg_big, sg_small, sg_small], [TA, TB, TA])):
        fset = factor_set(ctx, targets, sources, flags)
        results, traces = api.vgicp_align_debug_trace(targets, sources, T0s, flags, api_params(THREE))
        states = teacher_forced(fset, results, traces, T0s, p)
        fset.close()
        for r, s in zip(results, states):
            print(res, sv, len(targets), "status", r.status_name, "iterations", r.iterations, "trials", r.trials, "inliers", r.num_inliers)
            assert s["iterations"] >= 1 and r.num_inliers > 100


def test_a_general_form_source_beside_a_plane_form_one(orc, ctx):
    """The scans above carry plane-form covariances (the plan's first segment, the 24 B/pt kernel); a source whose covariances are not of that
    form takes the general segment and its kernel.  One batch with both: the same teacher-forced check."""
    from glim_amd import api

    (_, (sp, sc, sg)), delta = pair(orc, ctx, SMALL)
    general = api.PointCloudGPU.clone(sp, covs=sc + 0.01 * np.eye(3)[None], ctx=ctx)
    vm = vmap(orc, ctx, SMALL, 0.5)
    TA = delta @ orc.se3_exp(PERT_A)
    targets, sources, T0s = [vm, vm], [sg, general], [TA, TA]
    fset = factor_set(ctx, targets, sources, 0)
    results, traces = api.vgicp_align_debug_trace(targets, sources, T0s, 0, api_params(THREE))
    states = teacher_forced(fset, results, traces, T0s, lmr.params(**THREE))
    fset.close()
    assert not same_result(results[0], results[1])  # two different factors
    for r, s in zip(results, states):
        print("plane / general", r.status_name, r.iterations, r.trials, r.num_inliers)
        assert s["iterations"] >= 1 and r.num_inliers > 100


# ---- 2. a rejected trial -----------------------------------------------------------------------------------------------------------------
def test_a_rejected_trial_on_the_device(orc, ctx):
    from glim_amd import api

    size, res, pert, kw = REJECT_CASE
    ((tp, tc, tg), (sp, sc, sg)), delta = pair(orc, ctx, size)
    T0 = delta @ orc.se3_exp(pert)
    p = lmr.params(**kw)
    ref_map = orc.VoxelMap(res).insert(tp, tc)
    final, ref = lmr.run(lambda T: orc.vgicp_linearize(ref_map, sp, sc, T), T0, p)
    accepted = [e["accepted"] for e in ref]
    print("oracle:", "".join("A" if a else "r" for a in accepted), ["%.4f" % m for m in moves(ref)], final["status"], final["iterations"], final["trials"])
    assert accepted[0] and any(accepted[1:]) and not all(accepted[1:]), accepted
    assert min(moves(ref)) >= 10 * RECORD_TOL, moves(ref)  # the oracle's margins: no decision is within reach of the record tolerance
    vm = vmap(orc, ctx, size, res)
    results, traces = api.vgicp_align_debug_trace([vm], [sg], [T0], 0, api_params(kw))
    assert [e["accepted"] for e in traces[0]] == accepted
    assert (results[0].status, results[0].iterations, results[0].trials) == (final["status"], final["iterations"], final["trials"])
    k = accepted.index(False)
    if k + 1 < len(traces[0]):
        assert traces[0][k + 1]["lam"] == traces[0][k]["lam"] * 10  # the next candidate is solved from the kept record with the new lambda
    fset = factor_set(ctx, [vm], [sg], 0)
    teacher_forced(fset, results, traces, [T0], p)
    fset.close()


# ---- 3. against the oracle-driven loop ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def end_to_end(orc, ctx):
    """per case of CASES, computed once: the device result and the restatement over the FP64 oracle"""
    from glim_amd import api

    out = []
    for size, res, pert, kw in CASES:
        ((tp, tc, tg), (sp, sc, sg)), delta = pair(orc, ctx, size)
        T0 = delta @ orc.se3_exp(pert)
        dev = api.vgicp_align_batch([vmap(orc, ctx, size, res)], [sg], [T0], 0, api_params(kw))[0]
        ref_map = orc.VoxelMap(res).insert(tp, tc)
        ref, ref_trace = lmr.run(lambda T: orc.vgicp_linearize(ref_map, sp, sc, T), T0, lmr.params(**kw))
        out.append(dict(dev=dev, oracle=ref, trace=ref_trace))
    return out


@pytest.mark.parametrize("case", range(len(CASES)))
def test_end_to_end_against_the_oracle_driven_loop(end_to_end, case):
    """Statuses and counts are equal; the final pose is within iterations x POSE_TOL (1e-4 m / rad per Gauss-Newton iteration, the project's gate)."""
    r = end_to_end[case]
    dev, ref = r["dev"], r["oracle"]
    d = np.abs(dev.T_target_source - ref["T"]).max()
    print(f"case {case}: device {dev.status_name} {dev.iterations}/{dev.trials}, oracle-driven {ref['status']} {ref['iterations']}/{ref['trials']}, "
          f"|dT| {d:.3e}, oracle moves {['%.4f' % m for m in moves(r['trace'])]}")
    assert min(moves(r["trace"])) > MOVES, moves(r["trace"])  # the condition the case was chosen for, on this run's oracle
    assert (dev.status, dev.iterations, dev.trials) == (ref["status"], ref["iterations"], ref["trials"])
    assert ref["iterations"] >= 1 and d <= ref["iterations"] * POSE_TOL


# ---- 4. determinism and batch forms ------------------------------------------------------------------------------------------------------
def test_determinism_and_batch_forms(orc, ctx):
    from glim_amd import api

    (_, (_, _, sg_big)), delta = pair(orc, ctx, BIG)
    (_, (_, _, sg_small)), _ = pair(orc, ctx, SMALL)
    vb, vs = vmap(orc, ctx, BIG, 0.5), vmap(orc, ctx, SMALL, 0.5)
    TA, TB = delta @ orc.se3_exp(PERT_A), delta @ orc.se3_exp(PERT_B)
    prm = api_params(dict(relative_error_tol=5e-2))
    batch = ([vs, vb, vs], [sg_small, sg_big, sg_small], [TA, TB, TB], 0, prm)
    a, b = api.vgicp_align_batch(*batch), api.vgicp_align_batch(*batch)
    for x, y in zip(a, b):
        assert same_result(x, y)  # the same batch twice: identical bits
    # the B = 1 form of the factor is the batch of one, bitwise
    f = api.IntegratedVGICPFactorGPU(np.eye(4), 1, vs, sg_small)
    alone = api.vgicp_align_batch([vs], [sg_small], [TA], 0, prm)[0]
    assert same_result(f.align(TA, prm), alone) and alone.iterations >= 1
    with pytest.raises(api.GlimAmdError):
        api.IntegratedVGICPFactorGPU(0, 1, vs, sg_small).align(TA, prm)  # a binary factor
    # a problem in a differently composed batch (another cut of its points into rows): the same decisions, the pose within the gate of test 3
    # (problem 0 is CASES[0], problem 1 CASES[3]: every trial moves the error by more than 5e-3 of itself)
    alone_big = api.vgicp_align_batch([vb], [sg_big], [TB], 0, prm)[0]
    for got, want in ((a[0], alone), (a[1], alone_big)):
        d = np.abs(got.T_target_source - want.T_target_source).max()
        print("another batch: |dT|", d, "bitwise equal" if same_result(got, want) else "different bits")
        assert (got.status, got.iterations, got.trials) == (want.status, want.iterations, want.trials)
        assert d <= max(1, want.iterations) * POSE_TOL


# ---- 5. statuses -------------------------------------------------------------------------------------------------------------------------
def test_statuses(orc, ctx):
    from glim_amd import api

    (_, (_, _, sg)), delta = pair(orc, ctx, SMALL)
    vm = vmap(orc, ctx, SMALL, 0.5)
    TA = delta @ orc.se3_exp(PERT_A)
    far = delta.copy()
    far[0, 3] += 1e3
    fset = factor_set(ctx, [vm], [sg], 0)
    # off the map
    r = api.vgicp_align_batch([vm], [sg], [far])[0]
    assert r.status == lmr.NO_CORRESPONDENCES and np.array_equal(r.T_target_source, far) and (r.iterations, r.trials, r.num_inliers) == (0, 0, 0)
    # max_iterations = 0: the round-0 record and pose
    r = api.vgicp_align_batch([vm], [sg], [TA], 0, api_params(dict(max_iterations=0)))[0]
    assert r.status == lmr.MAX_ITERATIONS and np.array_equal(r.T_target_source, TA) and (r.iterations, r.trials) == (0, 0)
    assert same_record(r.compact, TA, fset.linearize_poses(api.pose12(TA))[0]) and r.num_inliers > 100
    # a NaN in T_init
    bad = TA.copy()
    bad[1, 3] = np.nan
    r = api.vgicp_align_batch([vm], [sg], [bad])[0]
    assert r.status == lmr.NUMERIC and (r.iterations, r.trials) == (0, 0)
    fset.close()
    # a problem that finishes at round 0 beside a running one: the running one's bits are those it has beside a running neighbour of the same
    # pair (the plan is the same: it depends on the pairs, not on the poses)
    prm = api_params(THREE)
    with_far = api.vgicp_align_batch([vm, vm], [sg, sg], [far, TA], 0, prm)
    with_near = api.vgicp_align_batch([vm, vm], [sg, sg], [delta, TA], 0, prm)
    with_nan = api.vgicp_align_batch([vm, vm], [sg, sg], [bad, TA], 0, prm)
    assert with_far[0].status == lmr.NO_CORRESPONDENCES and with_nan[0].status == lmr.NUMERIC and with_near[0].iterations >= 1
    assert with_far[1].iterations >= 1 and same_result(with_far[1], with_near[1]) and same_result(with_nan[1], with_near[1])


def test_argument_errors_with_real_handles(orc, ctx):
    from glim_amd import api

    ((tp, tc, tg), (sp, sc, sg)), delta = pair(orc, ctx, SMALL)
    vm = vmap(orc, ctx, SMALL, 0.5)
    valid = lambda: api.vgicp_align_batch([vm], [sg], [delta])[0]
    good = valid()
    assert good.num_inliers > 100

    def refused(code, targets, sources, flags=0):
        with pytest.raises(api.GlimAmdError) as e:
            api.vgicp_align_batch(targets, sources, [delta] * len(sources), flags)
        assert e.value.code == code, e.value
        assert same_result(valid(), good)  # the next valid call still works

    refused(-1, [vm], [sg], api.FACTOR_BINARY)
    ctx2 = api.Context(0, 1)
    other = api.PointCloudGPU.clone(sp, covs=sc, ctx=ctx2)
    refused(-1, [vm], [other])  # handles of two contexts
    refused(-5, [vm, vm], [sg, api.PointCloudGPU.clone(sp, ctx=ctx)])  # a source without covariances (glim_amd_factor_set_add's answer)
    refused(-5, [api.GaussianVoxelMapGPU(0.5, ctx=ctx)], [sg])  # a map nothing was inserted into (likewise)
    refused(-1, [vm], [api.PointCloudGPU.clone(np.zeros((0, 3)), covs=np.zeros((0, 3, 3)), ctx=ctx)])  # an empty source
    other.close()
    ctx2.close()


# ---- 6. no side effects ------------------------------------------------------------------------------------------------------------------
def _same_lin(a, b):
    return all(x["num_inliers"] == y["num_inliers"] and x["error"] == y["error"] and np.array_equal(x["H_ss"], y["H_ss"]) and np.array_equal(x["b_s"], y["b_s"])
               for x, y in zip(a, b)) and len(a) == len(b)


def test_a_callers_three_factor_set_is_left_alone(orc, ctx):
    from glim_amd import api

    (_, (_, _, sg_big)), delta = pair(orc, ctx, BIG)
    (_, (_, _, sg_small)), _ = pair(orc, ctx, SMALL)
    vb, vs = vmap(orc, ctx, BIG, 0.5), vmap(orc, ctx, SMALL, 0.5)
    TA, TB = delta @ orc.se3_exp(PERT_A), delta @ orc.se3_exp(PERT_B)
    fset = factor_set(ctx, [vb, vb, vs], [sg_big, sg_small, sg_small], 0)
    lin = {1: TA}
    before = fset.linearize(lin)
    frozen_before = fset.error({1: TB}, lin)
    plans = api.plan_stats(ctx)
    # the same pairs (the plan a cache lookup would match) and other pairs
    api.vgicp_align_batch([vb, vb, vs], [sg_big, sg_small, sg_small], [TB, TB, TB])
    api.vgicp_align_batch([vs], [sg_small], [TB])
    assert api.plan_stats(ctx) == plans  # no plan of the context built, recycled, parked or taken
    assert fset.error({1: TB}, lin) == frozen_before  # frozen at the caller's linearisation pose, as before
    assert _same_lin(fset.linearize(lin), before) and before[0]["num_inliers"] > 100
    fset.close()


def test_a_resident_session_of_the_context_is_left_alone(orc):
    """A one-factor set of a priority-1 context is served by a resident session after a few synchronous linearisations; an align call of that
    context in between neither ends the session nor changes what it answers."""
    from glim_amd import api

    ctx1 = api.Context(0, 1, priority=1)
    try:
        ((tp, tc, tg), (sp, sc, sg)), delta = clouds(orc, api, ctx1, rings=SMALL[0], az=SMALL[1])
        vm = api.GaussianVoxelMapGPU(0.5, ctx=ctx1).insert(tg)
        TA, TB = delta @ orc.se3_exp(PERT_A), delta @ orc.se3_exp(PERT_B)
        fset = factor_set(ctx1, [vm], [sg], 0)
        with ctx1.diag("resident=1,resident_idle_us=200000"):
            before = [fset.linearize({1: TA}) for _ in range(6)]
            stats = api.resident_stats(ctx1)
            assert stats["alive"] and _same_lin(before[0], before[-1])
            r = api.vgicp_align_batch([vm], [sg], [TB])[0]
            assert r.iterations >= 1
            assert api.resident_stats(ctx1)["alive"]
            after = fset.linearize({1: TA})
            now = api.resident_stats(ctx1)
            assert _same_lin(after, before[0])
            assert now["launches"] == stats["launches"] and now["requests"] == stats["requests"] + 1, (stats, now)  # the same session answered
        fset.close()
    finally:
        api.resident_stop(ctx1)


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_returns_the_python_result(orc, ctx, tmp_path):
    """tests/cpp/test_vgicp_align.cpp calls glim_amd::align_vgicp (batch and single form) on clouds it uploads itself from the dumped arrays"""
    from glim_amd import api

    ((tp, tc, _), (sp, sc, _)), delta = pair(orc, ctx, SMALL)

    (tp4, tc16), (sp4, sc16) = packed(tp, tc), packed(sp, sc)
    tg, sg = api.PointCloudGPU.clone_packed(tp4, tc16, ctx=ctx), api.PointCloudGPU.clone_packed(sp4, sc16, ctx=ctx)
    vm = api.GaussianVoxelMapGPU(0.5, ctx=ctx).insert(tg)
    T0 = [delta @ orc.se3_exp(PERT_A), delta]
    res = api.vgicp_align_batch([vm, vm], [sg, sg], T0)
    alone = [api.vgicp_align_batch([vm], [sg], [T])[0] for T in T0]
    path = tmp_path / "case.bin"
    with open(path, "wb") as fh:
        fh.write(struct.pack("<iii", len(tp), len(sp), 2))
        for a in (tp4, tc16, sp4, sc16, np.array([0.5]), np.array([api.pose12(T) for T in T0])):
            fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        for r in res + alone:
            row = np.concatenate([api.pose12(r.T_target_source), [r.error, r.inlier_fraction, r.iterations, r.trials, r.status], r.linearized()["H_ss"].reshape(-1)])
            assert row.shape == (53,)
            fh.write(row.astype(np.float64).tobytes())
    out = subprocess.run([build_cpp(tmp_path, "vgicp_align"), str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and f"test_vgicp_align OK ({len(tp)} x {len(sp)} points, 2 problems)" in out.stdout, out.stdout + out.stderr
