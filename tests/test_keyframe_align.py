"""Scan-to-keyframes VGICP registration (include/glim_amd.h "Scan-to-keyframes VGICP registration"), the part that needs no device: the ABI
surface, the default parameters, the argument errors that are answered before any HIP call, glim_amd/csrc/keyframe_lm_step.hpp under a plain C++
compiler against tests/keyframe_restatement.py, the restatement against lm_restatement, and the C++ mirror.

The scene (tests/keyframe_restatement.py): three scans of synth.arc_trajectory(3, 0.6, 3.0) at SMALL = (16, 128), 2 048 points each; keyframes
are scans 0 and 1 at their world poses with maps at 0.5 and 1.0 (M = 4), the source is scan 2, X_init = poses[2] Exp(pert).  With the oracle's
kNN covariances rounded to FP32 the oracle-driven loop ran (A accepted, r rejected; relative error change per trial):
  SMALL PERT_A  relative_error_tol 5e-2   AAA      -0.906 -0.0138                    CONVERGED, 2 iterations, 4 048 of 4 x 2 048 inliers
  SMALL PERT_C  relative_error_tol 5e-2   AAAA     -0.954 -0.057 -0.0088             CONVERGED, 3 iterations
  SMALL REJECT  max_iterations 3          AAArrrr  -0.657 -0.802 then +0.0097 x 4    MAX_TRIALS, 2 iterations, 6 trials"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import keyframe_restatement as kr
import lm_restatement as lmr
from align_cases import PERT_A, PERT_C, ROOT, SMALL, build_cpp, build_driver, check_against_restatement, check_symbols, moves, params_head
from test_gicp import POSE_TOL

NEW_STABLE = ["glim_amd_keyframe_align_default_params", "glim_amd_keyframe_align_batch"]
NEW_DIAG = ["glim_amd_debug_keyframe_align_trace"]
INVALID, UNSUPPORTED = -1, -6
MAX_TARGETS = 64


def test_new_symbols_are_declared_once_and_listed():
    from glim_amd import api

    mirror = check_symbols(NEW_STABLE, NEW_DIAG, "keyframe_align.hpp")
    assert "glim_amd_keyframe_align_batch(" in mirror and "align_to_keyframes" in mirror
    assert '#include "gicp_align.hpp"' in mirror  # LMParams and AlignResult are reused
    head = open(os.path.join(ROOT, "include", "glim_amd.h")).read()
    assert "#define GLIM_AMD_KEYFRAME_ALIGN_MAX_TARGETS %d" % MAX_TARGETS in head and api.KEYFRAME_ALIGN_MAX_TARGETS == MAX_TARGETS
    for n in ("vgicp_align_keyframes", "vgicp_align_keyframes_debug_trace"):
        assert callable(getattr(api, n))
    # the rule's header is included by vgicp_align.hip only (tests/test_build_layout.py: a touch of it recompiles that unit alone)
    csrc = os.path.join(ROOT, "glim_amd", "csrc")
    users = sorted(f for f in os.listdir(csrc) if f.endswith(".hip") and "keyframe_lm_step.hpp" in open(os.path.join(csrc, f)).read())
    assert users == ["vgicp_align.hip"]


def test_default_params_are_the_gicp_defaults():
    from glim_amd import _lib

    p, q = _lib.LMParams(), _lib.LMParams()
    assert _lib.lib().glim_amd_keyframe_align_default_params(C.byref(p)) == 0
    assert {k: getattr(p, k) for k, _ in _lib.LMParams._fields_} == lmr.DEFAULTS
    assert _lib.lib().glim_amd_gicp_align_default_params(C.byref(q)) == 0
    assert bytes(p) == bytes(q)
    assert _lib.lib().glim_amd_keyframe_align_default_params(None) == INVALID


def test_argument_errors_without_a_device():
    """every refusal that needs no live handle: the checks run before anything of a handle is read"""
    from glim_amd import _lib, api

    L = _lib.lib()
    fn = L.glim_amd_keyframe_align_batch
    out = (_lib.AlignResult * 2)()
    null2, null4 = (C.c_void_p * 2)(None, None), (C.c_void_p * 4)(None, None, None, None)
    eye12, eye36 = list(np.eye(4)[:3].reshape(-1)), list(np.eye(6).reshape(-1))
    P, X = np.tile(eye12, 4), np.tile(eye12, 2)
    idx = lambda *v: np.array(v, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def prior(*entries):
        p = (_lib.BundlePrior * max(1, len(entries)))()
        for c, (pose, T, info) in zip(p, entries):
            c.pose = pose
            c.T[:] = T
            c.information[:] = info
        return p

    def call(sh=null2, first=idx(0, 3, 4), th=null4, P=dp(P), X=dp(X), pr=None, npr=0, flags=0, count=2, prm=None, out=out, fc=None):
        return fn(sh, first, th, P, X, pr, npr, flags, count, prm, out, fc)

    assert call(count=0) == 0 and call(sh=None, first=None, th=None, P=None, X=None, out=None, count=0) == 0  # an empty batch
    assert api.vgicp_align_keyframes([]) == []
    assert call(count=-1) == INVALID and call(npr=-1) == INVALID
    for kw in (dict(sh=None), dict(first=None), dict(th=None), dict(P=None), dict(X=None), dict(out=None), dict(npr=1), dict()):  # null arrays, then null handles
        assert call(**kw) == INVALID, kw
    for first in (idx(1, 3, 4), idx(0, 3, 2), idx(0, 0, 4), idx(0, 4, 4), idx(0, -1, 4)):  # not from 0, descending, a problem with no target
        assert call(first=first) == INVALID
    assert call(first=idx(0, MAX_TARGETS + 1, MAX_TARGETS + 2)) == UNSUPPORTED and call(first=idx(0, 1, MAX_TARGETS + 2)) == UNSUPPORTED
    assert call(first=idx(0, MAX_TARGETS, MAX_TARGETS + 1)) == INVALID  # the cap itself is allowed: on to the null handles
    for flags in (api.FACTOR_BINARY, api.FACTOR_BINARY | api.FACTOR_SURFACE_VALIDATION, 4):
        assert call(flags=flags) == INVALID
    nan12, inf36 = [float("nan")] + eye12[1:], eye36[:7] + [float("inf")] + eye36[8:]
    for entries in ([(2, eye12, eye36)], [(-1, eye12, eye36)], [(0, eye12, eye36), (0, eye12, eye36)], [(1, nan12, eye36)], [(1, eye12, inf36)]):
        assert call(pr=prior(*entries), npr=len(entries)) == INVALID, entries
    for field, value in (("lambda_factor", 1.0), ("lambda_initial", float("nan")), ("lambda_initial", -1.0), ("error_scale", 0.0), ("max_iterations", -1),
                         ("max_trials", -1), ("max_trials", 4097), ("max_iterations", 4097), ("lambda_upper_bound", float("inf"))):
        bad = _lib.LMParams()
        L.glim_amd_keyframe_align_default_params(C.byref(bad))
        setattr(bad, field, value)
        assert call(prm=C.byref(bad)) == INVALID, field
    tr = L.glim_amd_debug_keyframe_align_trace
    rounds = (_lib.AlignTraceEntry * 64)()
    tp, tT, tc = np.zeros((2, 32, 28)), np.zeros((32, 4, 12)), np.zeros((32, 4, 29))
    base = (null2, idx(0, 3, 4), null4, dp(P), dp(X), None, 0, 0, 2, None, out, None)
    assert tr(*base, rounds, dp(tp), dp(tT), dp(tc)) == INVALID  # null handles
    for missing in range(4):  # a trace without one of its arrays
        arrays = [rounds, dp(tp), dp(tT), dp(tc)]
        arrays[missing] = None
        assert tr(*base, *arrays) == INVALID
    assert tr(*(base[:8] + (0,) + base[9:]), None, None, None, None) == 0  # an empty batch
    assert tr(*(base[:7] + (api.FACTOR_BINARY,) + base[8:]), rounds, dp(tp), dp(tT), dp(tc)) == INVALID


# ---- keyframe_lm_step.hpp on the host, fed the oracle's records of the scene ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def step_exe(tmp_path_factory):
    return build_driver(tmp_path_factory, "keyframe_lm_step", "-Wno-unknown-pragmas")


@pytest.fixture(scope="module")
def scene(orc):
    """the oracle's factors of the scene at SMALL (kNN covariances rounded to FP32), and the world poses"""
    poses, pts = kr.scans(SMALL)
    clouds = []
    for p in pts:
        _, covs = orc.covariances(p, orc.knn(p, 10))
        clouds.append((p, covs.astype(np.float32).astype(np.float64)))
    return poses, kr.oracle_factors(orc, clouds, (0, 1), 2, poses)


def pose12(T):
    return np.asarray(T)[:3].reshape(-1)


def pose44(v):
    return np.vstack([np.asarray(v).reshape(3, 4), [0, 0, 0, 1]])


def run_cpp_step(exe, tmp_path, p, Ps, X_init, rounds, prior=None):
    """rounds: per round the M compact records -> per round a dict"""
    M = len(Ps)
    head = params_head(p) + [float(M), 1.0 if prior is not None else 0.0]
    term = [pose12(prior[0]), np.asarray(prior[1], dtype=np.float64).reshape(-1)] if prior is not None else []
    data = np.concatenate([head] + [pose12(P) for P in Ps] + term + [pose12(X_init), [float(len(rounds))]] + [np.asarray(c).reshape(-1) for c in rounds])
    fin, fout = str(tmp_path / "step.in"), str(tmp_path / "step.out")
    np.asarray(data, dtype=np.float64).tofile(fin)
    out = subprocess.run([exe, "step", fin, fout], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "test_keyframe_lm_step OK" in out.stdout, out.stdout + out.stderr
    rows = np.fromfile(fout).reshape(len(rounds), 12 * M + 29 + 28 + 36)
    o = 12 * M + 57
    return [{"Tf": [pose44(v) for v in r[:12 * M].reshape(M, 12)], "compact": r[12 * M:12 * M + 29], "prior": r[12 * M + 29:o], "T": pose44(r[o:o + 12]),
             "cand": pose44(r[o + 12:o + 24]), "delta": r[o + 24:o + 30], "lam": r[o + 30], "solve_ok": bool(r[o + 31]), "iterations": int(r[o + 32]),
             "trials": int(r[o + 33]), "status": int(r[o + 34]), "accepted": bool(r[o + 35])} for r in rows]


CASES = {
    "pert_a": (PERT_A, dict(relative_error_tol=5e-2), "AA", lmr.CONVERGED),
    "pert_c": (PERT_C, dict(relative_error_tol=5e-2), "AAA", lmr.CONVERGED),
    "reject": (kr.REJECT_PERT, dict(max_iterations=3), "AArrrr", lmr.MAX_TRIALS),
}


def information(seed):
    A = np.random.default_rng(seed).normal(0, 1, (6, 6))
    return 30.0 * (A @ A.T) + 5.0 * np.eye(6)


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_step_header_on_the_oracle_records_of_the_scene(orc, scene, step_exe, tmp_path, name, with_prior):
    poses, factors = scene
    pert, kw, decisions, status = CASES[name]
    p = lmr.params(**kw)
    X_init = poses[2] @ orc.se3_exp(pert)
    # a prior that pulls on the pose without deciding the loop: at the truth, a full information some 1e-2 of the factors' H_ss
    prior = (poses[2], information(7)) if with_prior else None
    final, trace = kr.run(factors, X_init, p, prior)
    got = "".join("A" if e["accepted"] else "r" for e in trace[1:])
    print(name, "prior" if with_prior else "no prior", "A" + got, ["%.4f" % m for m in moves(trace)], final["status"], final["iterations"], final["trials"],
          final["rec"]["num_inliers"])
    if not with_prior:  # the sequences the docstring records
        assert (got, final["status"]) == (decisions, status)
        assert min(moves(trace)) >= 40 * 2e-4 if name == "reject" else final["iterations"] >= 2
    rows = run_cpp_step(step_exe, tmp_path, p, [P for _, P in factors], X_init, [e["factor_compact"] for e in trace], prior)
    check_against_restatement(rows, [e["state"] for e in trace])
    for k, (row, e) in enumerate(zip(rows, trace)):
        # the ordered sum, bit for bit: NumPy's one-at-a-time sum of the same records, the header's own prior contribution added last
        want = kr.sum_compact(e["factor_compact"])
        if with_prior:
            assert np.abs(row["prior"] - e["prior"]).max() <= 1e-12 * np.abs(e["prior"]).max(), k
            want = kr.add_prior(want, row["prior"])
        else:
            assert not row["prior"].any()
        assert row["compact"].tobytes() == want.tobytes(), k
        assert row["compact"][0] == e["factor_compact"][:, 0].sum()  # the inliers: the factors' alone
        # The factor poses of the round, T_f = P_f^-1 X, against the restatement's.  The two candidates X agree within
        # lm_restatement.pose_gate (check_against_restatement above; in round 0 both are X_init, bit for bit).  An entry of T_f is a row of the
        # rotation of P_f^-1 times a column of X (plus, in the last column, the translation of P_f^-1, which both sides share): the row has
        # 2-norm 1, so its three entries sum to at most sqrt(3), and the candidates' difference reaches T_f times sqrt(3) at most.  On top comes
        # the rounding of the two ways to form the product (numpy's inverse and matmul there, se3_inverse and se3_compose here): four products
        # and three sums after the inverse's own three, under 16 roundings of the largest term (the bound tests/test_keyframe_align_gpu.py uses).
        gate = np.sqrt(3.0) * lmr.pose_gate(trace[k - 1]["state"]) if k else 0.0
        for (_, P), Tf, ref in zip(factors, row["Tf"], e["Tf"]):
            product = 16 * lmr.EPS * max(1.0, np.abs(np.linalg.inv(P)).max()) * max(1.0, np.abs(e["T"]).max())
            assert np.abs(Tf - ref).max() <= gate + product, (k, np.abs(Tf - ref).max(), gate, product)


def test_a_factor_pose_that_is_not_finite_is_numeric(orc, scene, step_exe, tmp_path):
    poses, factors = scene
    p = lmr.params()
    Ps = [P.copy() for _, P in factors]
    Ps[2][1, 3] = np.nan
    recs = np.stack([lmr.compact_of_record(lin(np.linalg.inv(P) @ poses[2])) for lin, P in factors])
    rows = run_cpp_step(step_exe, tmp_path, p, Ps, poses[2], [recs, recs])
    assert [r["status"] for r in rows] == [lmr.NUMERIC, lmr.NUMERIC] and not rows[0]["accepted"] and rows[0]["trials"] == 0
    assert np.array_equal(rows[1]["T"], poses[2])
    rows = run_cpp_step(step_exe, tmp_path, p, [P for _, P in factors], poses[2], [recs])
    assert rows[0]["status"] == lmr.RUNNING and rows[0]["accepted"]


def test_the_header_is_clean_under_the_sanitizers(orc, scene, tmp_path):
    """the stand-alone program once more with AddressSanitizer and UndefinedBehaviorSanitizer, over the rejected-trial case with a prior"""
    exe = str(tmp_path / "test_keyframe_lm_step_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "cpp", "test_keyframe_lm_step.cpp"), "-o", exe])
    poses, factors = scene
    p = lmr.params(max_iterations=3)
    X_init = poses[2] @ orc.se3_exp(kr.REJECT_PERT)
    prior = (poses[2], information(7))
    _, trace = kr.run(factors, X_init, p, prior)
    rows = run_cpp_step(exe, tmp_path, p, [P for _, P in factors], X_init, [e["factor_compact"] for e in trace], prior)
    assert [r["accepted"] for r in rows] == [e["accepted"] for e in trace]


# ---- the restatement itself ------------------------------------------------------------------------------------------------------------------------
def test_one_target_at_the_identity_is_the_single_factor_loop(orc, scene):
    poses, factors = scene
    seen = {}

    def lin(T):
        """one record per pose: the oracle sums in threads, so two evaluations of one pose differ in the last bits; and the loop sees a factor
        through its compact record, the upper triangle of the oracle's H_ss"""
        key = np.asarray(T, dtype=np.float64).tobytes()
        if key not in seen:
            seen[key] = lmr.record_of_compact(lmr.compact_of_record(factors[0][0](T)))
        return seen[key]

    p = lmr.params(relative_error_tol=5e-2)
    T0 = np.linalg.inv(poses[0]) @ poses[2] @ orc.se3_exp(PERT_A)
    a, ta = kr.run([(lin, np.eye(4))], T0, p)
    b, tb = lmr.run(lin, T0, p)
    assert len(seen) == len(ta)  # the second run asked for the poses of the first, bit for bit
    assert len(ta) == len(tb) >= 3 and (a["status"], a["iterations"], a["trials"]) == (b["status"], b["iterations"], b["trials"])
    assert np.array_equal(a["T"], b["T"]) and a["lam"] == b["lam"]
    for x, y in zip(ta, tb):
        assert np.array_equal(x["T"], y["T"]) and x["compact"].tobytes() == lmr.compact_of_record(y["record"]).tobytes() and x["accepted"] == y["accepted"]


def test_a_rigid_motion_of_the_world_moves_the_answer_with_it(orc, scene):
    """Left-multiplying every P_f and X_init by one G leaves every T_f = P_f^-1 X where it was, up to the rounding of the products: the same
    decisions, and G X within POSE_TOL per accepted iteration."""
    poses, factors = scene
    p = lmr.params(relative_error_tol=5e-2)
    X_init = poses[2] @ orc.se3_exp(PERT_A)
    G = orc.se3_exp([0.4, -0.3, 0.8, 25.0, -40.0, 3.0])
    a, ta = kr.run(factors, X_init, p)
    b, tb = kr.run([(lin, G @ P) for lin, P in factors], G @ X_init, p)
    assert [e["accepted"] for e in ta] == [e["accepted"] for e in tb] and (a["status"], a["iterations"], a["trials"]) == (b["status"], b["iterations"], b["trials"])
    assert min(moves(ta)) > 5e-3  # no trial of the case is within reach of the products' rounding
    d = np.abs(G @ a["T"] - b["T"]).max()
    print("|G X - X'|", d)
    assert a["iterations"] >= 2 and d <= a["iterations"] * POSE_TOL


# ---- the C++ mirror ------------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_compiles_links_and_answers_an_empty_batch(tmp_path):
    """include/glim_amd/keyframe_align.hpp: compiled with -Wall -Werror, linked, and run without a case (the defaults and an empty batch: no
    device call)"""
    out = subprocess.run([build_cpp(tmp_path, "keyframe_align")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "test_keyframe_align OK (no case given: nothing run)" in out.stdout, out.stdout + out.stderr
