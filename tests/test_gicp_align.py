"""GICP fine registration (include/glim_amd.h "GICP fine registration"), the part that needs no device: the ABI surface, the default parameters,
the argument errors, and the step rule of glim_amd/csrc/lm_step.hpp compiled with g++ against the NumPy restatement (tests/lm_restatement.py)
over oracle-driven runs."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import lm_restatement as lmr
from align_cases import build_driver, check_against_restatement, check_symbols, params_head

NEW_STABLE = ["glim_amd_gicp_align_default_params", "glim_amd_gicp_align_batch", "glim_amd_gicp_align_batch_incremental"]
NEW_DIAG = ["glim_amd_debug_gicp_align_trace"]


def test_new_symbols_are_declared_once_and_listed():
    from glim_amd import _lib

    check_symbols(NEW_STABLE, NEW_DIAG, "gicp_align.hpp")
    # the structures as the headers lay them out
    assert C.sizeof(_lib.LMParams) == 6 * 8 + 2 * 4 + 8
    assert C.sizeof(_lib.AlignResult) == 12 * 8 + 8 + 8 + 4 * 4 + 8 + 29 * 8
    assert C.sizeof(_lib.AlignTraceEntry) == (12 + 1 + 29) * 8 + 8


def test_default_params():
    from glim_amd import _lib, api

    p = _lib.LMParams()
    assert _lib.lib().glim_amd_gicp_align_default_params(C.byref(p)) == 0
    got = {k: getattr(p, k) for k, _ in _lib.LMParams._fields_}
    assert got == lmr.DEFAULTS
    assert _lib.lib().glim_amd_gicp_align_default_params(None) == -1
    q = api.LMParams()
    assert {k: getattr(q, k) for k in lmr.DEFAULTS} == lmr.DEFAULTS and q.resolved_max_trials() == 20
    assert lmr.params()["max_trials"] == 20 and lmr.params(max_trials=7)["max_trials"] == 7


def test_argument_errors_without_a_device():
    from glim_amd import _lib

    L = _lib.lib()
    INVALID = -1
    out = (_lib.AlignResult * 2)()
    trace = (_lib.AlignTraceEntry * 64)()
    null2 = (C.c_void_p * 2)(None, None)
    T = np.tile(np.eye(4)[:3].reshape(-1), 2)
    d = np.array([1.0, 1.0])
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    for fn in (L.glim_amd_gicp_align_batch, L.glim_amd_gicp_align_batch_incremental):
        assert fn(null2, null2, dp(T), dp(d), 0, None, out) == 0  # an empty batch
        assert fn(None, None, None, None, 0, None, None) == 0
        assert fn(null2, null2, dp(T), dp(d), -1, None, out) == INVALID
        assert fn(null2, null2, dp(T), dp(d), 2, None, out) == INVALID  # null handles
        assert fn(None, null2, dp(T), dp(d), 2, None, out) == INVALID
        assert fn(null2, null2, dp(T), dp(d), 2, None, None) == INVALID
        nan = np.array([1.0, np.nan])
        assert fn(null2, null2, dp(T), dp(nan), 2, None, out) == INVALID
        neg = np.array([-1.0, 1.0])
        assert fn(null2, null2, dp(T), dp(neg), 2, None, out) == INVALID
        bad = _lib.LMParams()
        L.glim_amd_gicp_align_default_params(C.byref(bad))
        bad.lambda_factor = 1.0
        assert fn(null2, null2, dp(T), dp(d), 2, C.byref(bad), out) == INVALID
    for ivox in (0, 1):
        assert L.glim_amd_debug_gicp_align_trace(ivox, null2, null2, dp(T), dp(d), 2, None, out, trace) == INVALID
        assert L.glim_amd_debug_gicp_align_trace(ivox, null2, null2, dp(T), dp(d), -1, None, out, trace) == INVALID
        assert L.glim_amd_debug_gicp_align_trace(ivox, null2, null2, dp(T), dp(d), 0, None, out, None) == 0


# ---- lm_step.hpp on the host ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lm_step_exe(tmp_path_factory):
    return build_driver(tmp_path_factory, "lm_step")


def run_cpp(exe, tmp_path, p, T_init, records):
    """the C++ step rule over `records` (teacher-forced: record k is what round k evaluated) -> one dict per round"""
    data = np.concatenate([params_head(p), np.asarray(T_init)[:3].reshape(-1), [float(len(records))]] + [lmr.compact_of_record(L) for L in records])
    fin, fout = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    data.astype(np.float64).tofile(fin)
    out = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "test_lm_step OK" in out.stdout, out.stdout + out.stderr
    rows = np.fromfile(fout).reshape(len(records), 36)
    pose = lambda v: np.vstack([v.reshape(3, 4), [0, 0, 0, 1]])
    return [{"T": pose(r[0:12]), "cand": pose(r[12:24]), "delta": r[24:30], "lam": r[30], "solve_ok": bool(r[31]), "iterations": int(r[32]),
             "trials": int(r[33]), "status": int(r[34]), "accepted": bool(r[35])} for r in rows]


def oracle_linearize(orc, pair, max_d):
    t, s = pair["target"], pair["source"]
    return lambda T: orc.gicp_linearize(t["points"], t["covs"], s["points"], s["covs"], T, max_d)


PERTURBATION = [0.01, -0.02, 0.005, 0.05, 0.02, -0.01]


def test_lm_step_follows_the_restatement_over_an_oracle_driven_run(orc, small_pair, lm_step_exe, tmp_path):
    lin = oracle_linearize(orc, small_pair, 1.0)
    T0 = small_pair["delta"] @ orc.se3_exp(PERTURBATION)
    for kw in ({}, {"lambda_initial": 1e-12, "max_iterations": 3}, {"max_trials": 2}):
        p = lmr.params(**kw)
        final, trace = lmr.run(lin, T0, p)
        rows = run_cpp(lm_step_exe, tmp_path, p, T0, [e["record"] for e in trace])
        check_against_restatement(rows, [e["state"] for e in trace])
        assert final["status"] in (lmr.CONVERGED, lmr.MAX_ITERATIONS, lmr.MAX_TRIALS, lmr.LAMBDA_BOUND) and final["iterations"] >= 1
    # the default run ends near the planted motion (at the lambda bound: once the steps are too small to lower the error, every trial is rejected)
    final, trace = lmr.run(lin, T0)
    err = np.linalg.inv(small_pair["delta"]) @ final["T"]
    assert final["status"] == lmr.LAMBDA_BOUND and not trace[-1]["accepted"] and final["iterations"] >= 2
    assert np.linalg.norm(err[:3, 3]) < 0.02 and np.abs(err[:3, :3] - np.eye(3)).max() < 2e-3


def rising(lin, rounds):
    """the oracle's records with the error of the listed rounds (0 = the initial pose) made to rise"""
    state = {"k": -1}

    def f(T):
        state["k"] += 1
        L = dict(lin(T))
        if state["k"] in rounds:
            L["error"] = L["error"] * 1e3 + 1.0
        return L

    return f


def test_lm_step_rejects_and_stops_at_the_lambda_bound(orc, small_pair, lm_step_exe, tmp_path):
    lin = oracle_linearize(orc, small_pair, 1.0)
    T0 = small_pair["delta"] @ orc.se3_exp(PERTURBATION)
    # one rejected trial, then on: lambda 1e3 -> 1e4 (rejected) -> accepted trials
    p = lmr.params(lambda_initial=1e3)
    final, trace = lmr.run(rising(lin, {1}), T0, p)
    assert [e["accepted"] for e in trace[:3]] == [True, False, True] and trace[1]["state"]["lam"] == 1e4 and final["iterations"] >= 1
    assert np.array_equal(trace[1]["state"]["T"], T0) and trace[2]["lam"] == 1e4
    check_against_restatement(run_cpp(lm_step_exe, tmp_path, p, T0, [e["record"] for e in trace]), [e["state"] for e in trace])
    # every trial rises: 1e3 -> 1e4 -> 1e5 -> 1e6 > the bound
    final, trace = lmr.run(rising(lin, set(range(1, 30))), T0, p)
    assert final["status"] == lmr.LAMBDA_BOUND and final["trials"] == 3 and final["iterations"] == 0 and np.array_equal(final["T"], T0)
    rows = run_cpp(lm_step_exe, tmp_path, p, T0, [e["record"] for e in trace])
    check_against_restatement(rows, [e["state"] for e in trace])
    assert rows[-1]["status"] == lmr.LAMBDA_BOUND and np.array_equal(rows[-1]["T"][:3], T0[:3])


def test_lm_step_failed_solve_is_a_rejected_trial(orc, small_pair, lm_step_exe, tmp_path):
    """Cholesky of a singular H with lambda = 0 has a pivot that is not > 0: a failed solve, the trial is rejected whatever its error"""
    lin = oracle_linearize(orc, small_pair, 1.0)
    T0 = small_pair["delta"] @ orc.se3_exp(PERTURBATION)
    base = lin(T0)

    def singular(T):
        L = dict(base)
        L["H_ss"] = np.zeros((6, 6))
        L["error"] = base["error"] * 0.5 if not np.array_equal(T, T0) else base["error"]
        return L

    p = lmr.params(lambda_initial=0.0, max_iterations=2)
    records = [singular(T0)] + [dict(singular(T0), error=base["error"] * 0.5)] * 4  # lower errors: only the failed solve can reject them
    s, trace = lmr.new_state(T0, p), []
    for L in records:
        T, lam = s["cand"], s["lam"]
        s = lmr.step(p, s, L)
        trace.append({"T": T, "lam": lam, "record": L, "accepted": s["accepted"], "status": s["status"], "state": s})
    assert not lmr.solve(records[0]["H_ss"], records[0]["b_s"], 0.0)[0]
    assert [e["accepted"] for e in trace] == [True, False, False, False, False] and s["status"] == lmr.MAX_TRIALS and s["iterations"] == 0
    rows = run_cpp(lm_step_exe, tmp_path, p, T0, records)
    check_against_restatement(rows, [e["state"] for e in trace])
    assert all(not r["solve_ok"] for r in rows[:-1]) and all(np.array_equal(r["cand"][:3], T0[:3]) for r in rows)


def test_lm_step_special_inputs(lm_step_exe, tmp_path):
    """zero inliers at the initial pose, and a non-finite record: defined statuses, the initial pose kept"""
    T0 = np.eye(4)
    zero = {"num_inliers": 0, "error": 0.0, "H_ss": np.zeros((6, 6)), "b_s": np.zeros(6)}
    p = lmr.params()
    rows = run_cpp(lm_step_exe, tmp_path, p, T0, [zero, zero])
    assert [r["status"] for r in rows] == [lmr.NO_CORRESPONDENCES] * 2 and np.array_equal(rows[-1]["T"], T0)
    assert lmr.step(p, lmr.new_state(T0, p), zero)["status"] == lmr.NO_CORRESPONDENCES
    bad = dict(zero, num_inliers=5, error=np.nan)
    rows = run_cpp(lm_step_exe, tmp_path, p, T0, [bad])
    assert rows[0]["status"] == lmr.NUMERIC and np.array_equal(rows[0]["T"], T0)
    assert lmr.step(p, lmr.new_state(T0, p), bad)["status"] == lmr.NUMERIC
