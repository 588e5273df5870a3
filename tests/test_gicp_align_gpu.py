"""GICP fine registration on the device (include/glim_amd.h "GICP fine registration", glim_amd/csrc/gicp_align.hip): every trial record is the bits
of IntegratedGICPFactor.linearize at the trial's pose (the partition invariant), the decisions are those of tests/lm_restatement.py, a problem's
result does not depend on the batch it runs in."""
import struct
import subprocess

import numpy as np
import pytest

import lm_restatement as lmr
from align_cases import PERT_A, RECORD_TOL, api_params, build_cpp, ctx, packed, pair, same_record, same_result, teacher_forced  # noqa: F401 (ctx: a fixture)
from test_gicp import POSE_TOL, rigid_edge_sizes, rigid_edge_subset

pytestmark = pytest.mark.gpu
END_GATE = (0.02, 2e-3)  # test_hip_gicp_alignment_converges_like_the_oracle: metres, rotation entries, against the planted motion

# (rings, az, perturbation of the planted motion, max_correspondence_distance, parameters).  Chosen with the oracle on the CPU: in all but the last
# every trial moves the error by more than 5e-3 of itself, far from the record tolerance; the last runs the defaults to the end, where the steps
# become smaller than that tolerance by the nature of convergence -- the one case that may use the allowance of test 2.
CASES = [
    (16, 128, PERT_A, 0.5, dict(max_iterations=2)),
    (32, 384, PERT_A, 0.5, dict(relative_error_tol=5e-2)),
    (24, 256, [0.02, 0.01, -0.015, 0.15, -0.1, 0.05], 1.0, dict(lambda_initial=1e-12, max_iterations=2)),
    (32, 128, [0.03, -0.02, 0.02, 0.2, 0.15, -0.05], 1.0, dict(relative_error_tol=5e-2)),
    (16, 128, PERT_A, 0.5, dict()),
]
# test 4: found with the oracle on the CPU -- two accepted trials (the error falls by 0.91 and 0.56 of itself), then rejected ones (it rises by 0.13)
REJECT_CASE = (16, 128, [-0.002, -0.019, -0.029, 0.086, -0.219, 0.142], 0.3, dict(lambda_initial=1e-12, max_iterations=3))
# the parity row of DESIGN.md 4.7c: the largest |device - oracle-driven| final pose over CASES measured on an MI355X (translation, rotation
# entries; case 4, one run); the gate of test 3 is twice that.  The device and the oracle take the same decisions in these cases, so what is left
# is the fixed point's sensitivity to the FP32 sums of the device's records.
MEASURED_VS_ORACLE = (1.295e-07, 7.286e-08)


def factor_records(f):
    """the batch of one of align_cases.teacher_forced: the factor's own record at the round's pose"""
    return lambda poses: [f.linearize({1: poses[0]})]


@pytest.mark.parametrize("kind", ["index", "ivox1", "ivox7"])
def test_every_trial_is_the_factor_record_and_the_restatement_decision(orc, ctx, kind):
    from glim_amd import api

    ((tp, tc, tg), (sp, sc, sg)), delta = pair(orc, ctx, (32, 384))
    T0 = delta @ orc.se3_exp(PERT_A)
    if kind == "index":
        target = tg
    else:
        target = api.IncrementalVoxelMap(0.5, ctx=ctx).set_neighbor_voxel_mode(int(kind[4:])).insert(tg)
    f = api.IntegratedGICPFactor(np.eye(4), 1, target, sg, max_correspondence_distance=0.5)
    for kw in (dict(), dict(lambda_initial=1e-12, max_iterations=3)):
        results, traces = api.gicp_align_debug_trace([f.target_tree], [sg], [T0], 0.5, api_params(kw))
        s = teacher_forced(factor_records(f), results, traces, [T0], lmr.params(**kw))[0]
        print(kind, kw, "status", results[0].status_name, "iterations", results[0].iterations, "trials", results[0].trials, "inliers", results[0].num_inliers)
        assert s["iterations"] >= 1 and results[0].num_inliers > 100
        assert same_result(results[0], f.align(T0, api_params(kw)))  # the B = 1 form of the factor, without the trace
    f.close()


@pytest.fixture(scope="module")
def end_to_end(orc, ctx):
    """per case of CASES, computed once: the device result, the restatement over IntegratedGICPFactor.linearize (the host-driven loop), the
    restatement over the FP64 oracle"""
    from glim_amd import api

    out = []
    for rings, az, pert, max_d, kw in CASES:
        ((tp, tc, tg), (sp, sc, sg)), delta = pair(orc, ctx, (rings, az))
        T0 = delta @ orc.se3_exp(pert)
        f = api.IntegratedGICPFactor(np.eye(4), 1, tg, sg, max_correspondence_distance=max_d)
        p = lmr.params(**kw)
        dev = f.align(T0, api_params(kw))
        host, host_trace = lmr.run(lambda T: f.linearize({1: T}), T0, p)
        ref, _ = lmr.run(lambda T: orc.gicp_linearize(tp, tc, sp, sc, T, max_d), T0, p)
        f.close()
        out.append(dict(dev=dev, host=host, host_trace=host_trace, oracle=ref, delta=delta))
    return out


def close_trial(trace):
    """first trial of a reference trace whose error is within the record tolerance of the kept one (its decision may fall either way), or None"""
    e_cur = trace[0]["record"]["error"]
    for k, e in enumerate(trace[1:], 1):
        if abs(e["record"]["error"] - e_cur) <= RECORD_TOL * e_cur:
            return k
        e_cur = e["state"]["rec"]["error"]
    return None


@pytest.mark.parametrize("case", range(len(CASES)))
def test_end_to_end_against_the_host_driven_loop(end_to_end, case):
    r = end_to_end[case]
    dev, host = r["dev"], r["host"]
    d = np.abs(dev.T_target_source - host["T"]).max()
    print(f"case {case}: device {dev.status_name} {dev.iterations}/{dev.trials}, host-driven {host['status']} {host['iterations']}/{host['trials']}, |dT| {d:.3e}, "
          f"close trial {close_trial(r['host_trace'])}")
    assert d <= POSE_TOL
    k = close_trial(r["host_trace"])
    if k is None:
        assert (dev.status, dev.iterations, dev.trials) == (host["status"], host["iterations"], host["trials"])
    else:  # equal up to that trial; one trial more or less from there on
        assert abs(dev.trials - host["trials"]) <= 1 and abs(dev.iterations - host["iterations"]) <= 1 and min(dev.trials, host["trials"]) >= k - 1


def test_at_most_one_case_uses_the_allowance(end_to_end):
    assert sum(close_trial(r["host_trace"]) is not None for r in end_to_end) <= 1


@pytest.mark.parametrize("case", range(len(CASES)))
def test_end_to_end_against_the_oracle_driven_loop(end_to_end, case):
    r = end_to_end[case]
    dev, ref = r["dev"], r["oracle"]
    dt, dr = np.abs(dev.T_target_source[:3, 3] - ref["T"][:3, 3]).max(), np.abs(dev.T_target_source[:3, :3] - ref["T"][:3, :3]).max()
    err = np.linalg.inv(r["delta"]) @ dev.T_target_source
    et, er = np.linalg.norm(err[:3, 3]), np.abs(err[:3, :3] - np.eye(3)).max()
    print(f"case {case}: |device - oracle-driven| translation {dt:.3e} rotation {dr:.3e}; against the planted motion {et:.3e} m, {er:.3e}")
    assert et < END_GATE[0] and er < END_GATE[1]
    gate_t = END_GATE[0] if MEASURED_VS_ORACLE[0] is None else min(END_GATE[0], 2 * MEASURED_VS_ORACLE[0])
    gate_r = END_GATE[1] if MEASURED_VS_ORACLE[1] is None else min(END_GATE[1], 2 * MEASURED_VS_ORACLE[1])
    assert dt <= gate_t and dr <= gate_r


def test_a_rejected_trial_on_the_device(orc, ctx):
    from glim_amd import api

    rings, az, pert, max_d, kw = REJECT_CASE
    ((tp, tc, tg), (sp, sc, sg)), delta = pair(orc, ctx, (rings, az))
    T0 = delta @ orc.se3_exp(pert)
    p = lmr.params(**kw)
    _, ref = lmr.run(lambda T: orc.gicp_linearize(tp, tc, sp, sc, T, max_d), T0, p)
    accepted = [e["accepted"] for e in ref]
    assert accepted[:4] == [True, True, True, False], accepted
    f = api.IntegratedGICPFactor(np.eye(4), 1, tg, sg, max_correspondence_distance=max_d)
    results, traces = api.gicp_align_debug_trace([f.target_tree], [sg], [T0], max_d, api_params(kw))
    assert [e["accepted"] for e in traces[0]] == accepted
    assert traces[0][4]["lam"] == traces[0][3]["lam"] * 10  # the next candidate is solved from the kept record with the new lambda
    assert results[0].status == ref[-1]["status"] and results[0].iterations == 2
    teacher_forced(factor_records(f), results, traces, [T0], p)
    f.close()


# ---- batch shapes ------------------------------------------------------------------------------------------------------------------------
SHAPE_PARAMS = dict(lambda_initial=1e-12, max_iterations=3, relative_error_tol=0.5)


@pytest.fixture(scope="module")
def problems(orc, ctx):
    """17 problems over one shared target index (and one target passed as a cloud): ragged sources, problems that end in different rounds, one
    1 km away.  Each with its result when run alone."""
    from glim_amd import api

    ((tp, tc, tg), (sp, sc, sg)), delta = pair(orc, ctx, (32, 384))
    owner = api.IntegratedGICPFactor(np.eye(4), 1, tg, sg, max_correspondence_distance=1.0)
    sizes = rigid_edge_sizes(ctx.device_info()["num_cus"])
    assert sizes[:4] == [1, 255, 256, 257]
    reps = -(-sizes[-1] // len(sp))  # the largest size from shifted copies of the scan (a millimetre apart: the same surfaces)
    big_p = np.concatenate([sp + 1e-3 * k for k in range(reps)])[: sizes[-1]]
    big_c = np.concatenate([sc] * reps)[: sizes[-1]]
    near = delta @ orc.se3_exp([0.004, -0.003, 0.002, 0.03, 0.02, -0.01])
    far = delta.copy()
    far[0, 3] += 1e3
    sources, keep = {}, []

    def subset(n):
        if n not in sources:
            sel = rigid_edge_subset(sp, n)
            sources[n] = api.PointCloudGPU.clone(sp[sel], covs=sc[sel], ctx=ctx)
        return sources[n]

    big = api.PointCloudGPU.clone(big_p, covs=big_c, ctx=ctx)
    tree = owner.target_tree
    plist = [
        (tree, sg, delta @ orc.se3_exp(PERT_A), 0.5),                                        # two accepted trials
        (tree, sg, delta @ orc.se3_exp([0.042, -0.04, 0.056, 0.148, 0.128, 0.565]), 0.3),    # every trial rejected: uses them all
        (tree, sg, far, 1.0),                                                                # no correspondences, between two that have them
        (tree, subset(1), near, 1.0),                                                        # rank-deficient
        (tree, subset(255), near, 1.0),
        (tree, subset(256), near, 1.0),
        (tree, subset(257), near, 1.0),
        (tree, big, near, 1.0),                                                              # one block more than a finaliser trip
        (tg, sg, near, 1.0),                                                                 # a target given as a cloud: an index of its own
        (tree, sg, delta @ orc.se3_exp(0.3 * np.array([0.004, -0.003, 0.002, 0.03, 0.02, -0.01])), 1.0),  # converges in round 1 (the error falls by 0.24)
    ]
    rng = np.random.default_rng(5)
    while len(plist) < 17:
        plist.append((tree, subset(int(rng.integers(300, 4000))), delta @ orc.se3_exp(rng.uniform(-1, 1, 6) * [0.02, 0.02, 0.02, 0.1, 0.1, 0.1]), 0.7))
    prm = api_params(SHAPE_PARAMS)
    alone = [api.gicp_align_batch([t], [s], [T], d, prm)[0] for t, s, T, d in plist]
    yield plist, alone, prm
    owner.close()


@pytest.mark.parametrize("B", [1, 2, 3, 17])
def test_a_problem_does_not_depend_on_its_batch(problems, B):
    from glim_amd import api

    plist, alone, prm = problems
    for first in ((0,) if B == 17 else (0, 1, 2, 7)):  # windows that put the far, the exhausted and the large problem next to others
        idx = [(first + k) % len(plist) for k in range(B)]
        got = api.gicp_align_batch([plist[i][0] for i in idx], [plist[i][1] for i in idx], [plist[i][2] for i in idx], [plist[i][3] for i in idx], prm)
        for i, r in zip(idx, got):
            assert same_result(r, alone[i]), (B, first, i, r.status_name, alone[i].status_name)


def test_the_batch_holds_the_cases_it_is_meant_to(problems):
    plist, alone, prm = problems
    print([(r.status_name, r.iterations, r.trials, r.num_inliers) for r in alone])
    for r in alone:
        assert r.status in range(1, 7) and np.all(np.isfinite(r.T_target_source)) and np.all(np.isfinite(r.compact)) and np.isfinite(r.error) and np.isfinite(r.lam)
    assert alone[1].trials == prm.resolved_max_trials() and alone[1].iterations == 0  # every trial used
    assert alone[2].status == lmr.NO_CORRESPONDENCES and np.array_equal(alone[2].T_target_source, plist[2][2]) and alone[2].trials == 0
    assert any(r.status == lmr.CONVERGED and r.trials == 1 for r in alone)  # converged in round 1
    assert len({r.trials for r in alone}) >= 3  # problems that finish at different rounds
    assert alone[3].num_inliers <= 1  # the 1-point problem: a defined status, finite output (checked above)
    assert alone[8].num_inliers > 1000


def test_two_calls_and_a_second_context_return_the_same_bytes(orc, ctx, problems):
    from glim_amd import api

    plist, alone, prm = problems
    ((tp, tc, tg), (sp, sc, sg)), delta = pair(orc, ctx, (32, 384))
    idx = [0, 1, 2, 9]
    args = lambda t, s: ([t] * len(idx), [s] * len(idx), [plist[i][2] for i in idx], [plist[i][3] for i in idx], prm)
    a = api.gicp_align_batch(*args(tg, sg))
    b = api.gicp_align_batch(*args(tg, sg))
    ctx2 = api.Context(0, 1)
    tg2, sg2 = api.PointCloudGPU.clone(tp, covs=tc, ctx=ctx2), api.PointCloudGPU.clone(sp, covs=sc, ctx=ctx2)
    c = api.gicp_align_batch(*args(tg2, sg2))
    for x, y, z in zip(a, b, c):
        assert same_result(x, y) and same_result(x, z)
    for c_ in (tg2, sg2):
        c_.close()
    ctx2.close()


def test_argument_errors_with_real_handles(orc, ctx):
    from glim_amd import api

    ((tp, tc, tg), (sp, sc, sg)), delta = pair(orc, ctx, (16, 128))
    owner = api.IntegratedGICPFactor(np.eye(4), 1, tg, sg, max_correspondence_distance=1.0)
    ivox = api.IncrementalVoxelMap(1.0, ctx=ctx).insert(tg)
    valid = lambda: api.gicp_align_batch([owner.target_tree], [sg], [delta], 1.0)[0]
    good = valid()
    assert good.num_inliers > 100

    def refused(code, targets, sources, dist=1.0):
        with pytest.raises(api.GlimAmdError) as e:
            api.gicp_align_batch(targets, sources, [delta] * len(sources), dist)
        assert e.value.code == code, e.value
        assert same_result(valid(), good)  # the next valid call still works

    refused(-1, [owner.target_tree, ivox], [sg, sg])  # mixed kinds
    ctx2 = api.Context(0, 1)
    other = api.PointCloudGPU.clone(sp, covs=sc, ctx=ctx2)
    refused(-1, [owner.target_tree], [other])  # clouds of two contexts
    refused(-1, [ivox], [other])
    bare = api.PointCloudGPU.clone(sp, ctx=ctx)
    refused(-5, [owner.target_tree, owner.target_tree], [sg, bare])  # a source without covariances
    refused(-5, [api.PointCloudGPU.clone(tp, ctx=ctx)], [sg])  # a target without covariances
    refused(-6, [owner.target_tree], [sg], 100.0)  # a radius beyond the ring walk of an index built for 1.0
    empty = api.PointCloudGPU.clone(np.zeros((0, 3)), covs=np.zeros((0, 3, 3)), ctx=ctx)
    refused(-1, [owner.target_tree], [empty])
    refused(-1, [empty], [sg])
    assert api.gicp_align_batch([], [], [], 1.0) == []
    assert ivox.info()["num_points"] > 0 and api.gicp_align_batch([ivox], [sg], [delta], 100.0)[0].num_inliers > 100  # a map takes any finite radius
    other.close()
    ctx2.close()
    owner.close()


def test_the_returned_record_is_the_linearisation_at_the_estimate(orc, ctx):
    from glim_amd import api

    ((tp, tc, tg), (sp, sc, sg)), delta = pair(orc, ctx, (24, 256))
    T0 = delta @ orc.se3_exp(PERT_A)
    f = api.IntegratedGICPFactor(np.eye(4), 1, tg, sg, max_correspondence_distance=0.5)
    b = api.IntegratedGICPFactor(0, 1, tg, sg, target_tree=f.target_tree, max_correspondence_distance=0.5)
    r = f.align(T0)
    T = r.T_target_source
    assert r.iterations >= 1 and same_record(r.compact, T, f.linearize({1: T}))
    assert r.error == r.compact[1] and r.num_inliers == int(r.compact[0]) and r.inlier_fraction == r.num_inliers / len(sp) == f.inlier_fraction()
    want, got = b.linearize({0: np.eye(4), 1: T}), r.linearized(api.FACTOR_BINARY)
    for k in ("H_tt", "H_ts", "H_ss", "b_t", "b_s"):
        assert np.array_equal(got[k], want[k]) and np.any(got[k]), k
    b.close()
    f.close()


def test_cpp_mirror_returns_the_python_result(orc, ctx, tmp_path):
    """tests/cpp/test_gicp_align.cpp calls glim_amd::align_gicp (batch and single form) on clouds it uploads itself from the dumped arrays"""
    from glim_amd import api

    ((tp, tc, _), (sp, sc, _)), delta = pair(orc, ctx, (16, 128))

    (tp4, tc16), (sp4, sc16) = packed(tp, tc), packed(sp, sc)
    tg, sg = api.PointCloudGPU.clone_packed(tp4, tc16, ctx=ctx), api.PointCloudGPU.clone_packed(sp4, sc16, ctx=ctx)
    T0 = [delta @ orc.se3_exp(PERT_A), delta]
    res = api.gicp_align_batch([tg, tg], [sg, sg], T0, 0.5)
    path = tmp_path / "case.bin"
    with open(path, "wb") as fh:
        fh.write(struct.pack("<iii", len(tp), len(sp), 2))
        for a in (tp4, tc16, sp4, sc16, np.array([0.5]), np.array([api.pose12(T) for T in T0])):
            fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        for r in res:
            row = np.concatenate([api.pose12(r.T_target_source), [r.error, r.inlier_fraction, r.iterations, r.trials, r.status], r.linearized()["H_ss"].reshape(-1)])
            assert row.shape == (53,)
            fh.write(row.astype(np.float64).tobytes())
    out = subprocess.run([build_cpp(tmp_path, "gicp_align"), str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and f"test_gicp_align OK ({len(tp)} x {len(sp)} points, 2 problems)" in out.stdout, out.stdout + out.stderr
