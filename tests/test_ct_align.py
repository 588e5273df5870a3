"""CT-GICP frame alignment (include/glim_amd.h "CT-GICP frame alignment"), the part that needs no device: the ABI surface, the default parameters,
the argument errors, the step rule of glim_amd/csrc/ct_lm_step.hpp and the pose table of ct_se3.hpp compiled with g++ against the NumPy
restatements (tests/ct_lm_restatement.py, tests/ct_restatement.py) over oracle-driven runs, and the restated terms against finite differences."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import ct_lm_restatement as ctl
from align_cases import ROOT, build_driver, check_against_restatement, check_symbols, params_head
from ct_align_cases import CASES, case_inputs, cpu_scene, pose_table_cases
from ct_restatement import ct_poses, expmap, np_ct_linearize, sweep_poses, time_table

NEW_STABLE = ["glim_amd_ct_align_default_params", "glim_amd_ct_align"]
NEW_DIAG = ["glim_amd_debug_ct_align_trace", "glim_amd_debug_ct_align_poses"]


def test_new_symbols_are_declared_once_and_listed():
    from glim_amd import _lib

    mirror = check_symbols(NEW_STABLE, NEW_DIAG, "ct_align.hpp")
    for n in NEW_STABLE + NEW_DIAG:  # the counts tests/test_ct_gicp.py and tests/test_ivox.py pin
        assert "ivox" not in n and "ct_gicp" not in n, n
    assert re.search(r"glim_amd_ct_align\s*\(", mirror)
    for f in (os.path.join("adapters", "gtsam", "glim_amd_gtsam.hpp"), os.path.join("include", "glim_amd", "gtsam_points_compat.hpp")):
        assert re.search(r"\balign\s*\(", open(os.path.join(ROOT, f)).read()) and "align_ct" in open(os.path.join(ROOT, f)).read(), f
    # the structures as the headers lay them out
    assert C.sizeof(_lib.CtAlignTerms) == 26 * 8
    assert C.sizeof(_lib.CtAlignResult) == 24 * 8 + C.sizeof(_lib.CtLinearized) + 4 * 8 + 4 * 4
    assert C.sizeof(_lib.CtAlignTraceEntry) == (24 + 1 + 92 + 1) * 8 + 8
    # ... and as a C compiler does
    src = '#include <stdio.h>\n#include "glim_amd_diag.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(glim_amd_ct_align_terms), ' \
          "sizeof(glim_amd_ct_align_result), sizeof(glim_amd_ct_align_trace_entry)); return 0; }\n"
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), os.path.join(tmp, "s.c"), "-o", os.path.join(tmp, "s")])
        sizes = [int(x) for x in subprocess.run([os.path.join(tmp, "s")], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(_lib.CtAlignTerms), C.sizeof(_lib.CtAlignResult), C.sizeof(_lib.CtAlignTraceEntry)]


def test_default_params_and_argument_errors_without_a_device():
    from glim_amd import _lib, api

    L = _lib.lib()
    INVALID = -1
    p = _lib.LMParams()
    assert L.glim_amd_ct_align_default_params(C.byref(p)) == 0
    assert {k: getattr(p, k) for k, _ in _lib.LMParams._fields_} == ctl.DEFAULTS
    assert L.glim_amd_ct_align_default_params(None) == INVALID
    q = api.ct_align_params()
    assert {k: getattr(q, k) for k in ctl.DEFAULTS} == ctl.DEFAULTS and q.resolved_max_trials() == 16 == ctl.params()["max_trials"]
    # without a device there is no factor: every call below is refused, whichever argument is looked at first
    X = np.eye(4)[:3].reshape(12).copy()
    dp = X.ctypes.data_as(C.POINTER(C.c_double))
    out = _lib.CtAlignResult()
    trace = (_lib.CtAlignTraceEntry * 17)()
    fake = C.c_void_p(0)
    assert L.glim_amd_ct_align(None, dp, dp, None, None, C.byref(out)) == INVALID
    assert L.glim_amd_ct_align(fake, None, dp, None, None, C.byref(out)) == INVALID
    assert L.glim_amd_ct_align(fake, dp, None, None, None, C.byref(out)) == INVALID
    assert L.glim_amd_ct_align(fake, dp, dp, None, None, None) == INVALID
    for kp, kb, bad_pose in ((np.nan, 0.0, False), (-1.0, 0.0, False), (0.0, np.nan, False), (0.0, -1e-3, False), (1e-3, 0.0, True)):
        t = _lib.CtAlignTerms()
        t.T_location[:] = list(X)
        t.T_between[:] = list(X)
        if bad_pose:
            t.T_location[3] = np.inf
        t.location_precision, t.between_precision = kp, kb
        assert L.glim_amd_ct_align(None, dp, dp, C.byref(t), None, C.byref(out)) == INVALID
    bad = _lib.LMParams()
    L.glim_amd_ct_align_default_params(C.byref(bad))
    bad.lambda_factor = 1.0
    assert L.glim_amd_ct_align(None, dp, dp, None, C.byref(bad), C.byref(out)) == INVALID
    assert L.glim_amd_debug_ct_align_trace(None, dp, dp, None, None, C.byref(out), None) == INVALID
    assert L.glim_amd_debug_ct_align_trace(None, dp, dp, None, None, C.byref(out), trace) == INVALID
    assert L.glim_amd_debug_ct_align_poses(None, dp, dp, None, 0, None, None, None) == INVALID


# ---- ct_lm_step.hpp and ct_se3.hpp on the host ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ct_step_exe(tmp_path_factory):
    return build_driver(tmp_path_factory, "ct_lm_step")


def pose12(T):
    return np.asarray(T)[:3].reshape(-1)


def run_cpp_step(exe, tmp_path, p, tm, X_init, Y_init, records):
    """the C++ step rule over `records` (teacher-forced: record k is what round k evaluated) -> one dict per round"""
    P, kp = tm["location"] if tm["location"] is not None else (np.eye(4), 0.0)
    D, kb = tm["between"] if tm["between"] is not None else (np.eye(4), 0.0)
    data = np.concatenate([params_head(p), pose12(X_init), pose12(Y_init), pose12(P), [kp], pose12(D), [kb], [float(len(records))]] + [ctl.row_of_record(L) for L in records])
    fin, fout = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    data.astype(np.float64).tofile(fin)
    out = subprocess.run([exe, "step", fin, fout], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "test_ct_lm_step OK" in out.stdout, out.stdout + out.stderr
    rows = np.fromfile(fout).reshape(len(records), 67)
    pose = lambda v: np.vstack([v.reshape(3, 4), [0, 0, 0, 1]])
    return [{"X": pose(r[0:12]), "Y": pose(r[12:24]), "candX": pose(r[24:36]), "candY": pose(r[36:48]), "delta": r[48:60], "lam": r[60], "solve_ok": bool(r[61]),
             "iterations": int(r[62]), "trials": int(r[63]), "status": int(r[64]), "accepted": bool(r[65]), "cost": r[66]} for r in rows]


PAIR = dict(cand=("candX", "candY"), kept=("X", "Y"))  # the poses of a state, for check_against_restatement


@pytest.fixture(scope="module")
def oracle_runs(orc):
    """cases A-D run once with the oracle: name -> (terms, X0, Y0, final state, trace)"""
    runs = {}
    for name in CASES:
        tp, tc, sp, sc, times = cpu_scene(orc, CASES[name]["points"])
        X0, Y0, tm, max_d = case_inputs(name)
        lin = lambda X, Y: np_ct_linearize(orc, tp, tc, sp, sc, times, X, Y, max_d)
        final, trace = ctl.run(lin, X0, Y0, tm, ctl.params())
        runs[name] = (tm, X0, Y0, final, trace)
    return runs


def cost_changes(trace):
    """per trial, (e_cur - e_new) / e_cur against the cost kept before it"""
    out, kept = [], trace[0]["cost"]
    for e in trace[1:]:
        out.append((kept - e["cost"]) / kept)
        if e["accepted"]:
            kept = e["cost"]
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_ct_lm_step_follows_the_restatement_over_an_oracle_driven_run(oracle_runs, ct_step_exe, tmp_path, name):
    tm, X0, Y0, final, trace = oracle_runs[name]
    rows = run_cpp_step(ct_step_exe, tmp_path, ctl.params(), tm, X0, Y0, [e["record"] for e in trace])
    check_against_restatement(rows, [e["state"] for e in trace], **PAIR)
    changes = cost_changes(trace)
    print(name, "status", final["status"], "iterations", final["iterations"], "trials", final["trials"], "cost changes", ["%.3g" % c for c in changes])
    # no trial is decided by the last bits of the cost: the decisions above cannot flip between two correct implementations
    kept = trace[0]["cost"]
    for e in trace[1:]:
        assert abs(e["cost"] - kept) > 1e-12 * kept
        if e["accepted"]:
            kept = e["cost"]
    # the first two trials move the cost by >= 1.4e-2 of itself, 70 x the record tolerance 2e-4
    assert trace[1]["accepted"] and trace[2]["accepted"] and min(changes[:2]) >= 1.4e-2
    acc = [e["accepted"] for e in trace[1:]]
    if name == "A":
        assert acc[:2] == [True, True] and not any(acc[2:]) and final["status"] == ctl.MAX_TRIALS and final["trials"] == 16
        np.testing.assert_allclose(changes[:2], [0.94, 0.023], rtol=0.05)
    if name == "B":
        np.testing.assert_allclose(changes[:2], [0.97, 0.066], rtol=0.05)
    if name == "C":
        assert acc == [True] * 3 + [False] * 13
        assert (final["status"], final["iterations"], final["trials"]) == (ctl.MAX_TRIALS, 3, 16)
        np.testing.assert_allclose(changes[:3], [0.875, 0.0147, 2.6e-4], rtol=0.05)
        assert all(-2e-6 < c < 0 for c in changes[3:])
    if name == "D":
        assert acc == [True] * 5 and (final["status"], final["iterations"], final["trials"]) == (ctl.CONVERGED, 5, 5)


def test_ct_lm_step_special_inputs(ct_step_exe, tmp_path):
    """zero inliers at the initial pair, a non-finite record, a failed solve: defined statuses, the initial pair kept"""
    T0, T1 = sweep_poses()
    tm = ctl.terms((T0, 1e-3), (np.eye(4), 1e3))
    zero = ctl.record_of_row(np.zeros(92))
    p = ctl.params()
    rows = run_cpp_step(ct_step_exe, tmp_path, p, tm, T0, T1, [zero, zero])
    assert [r["status"] for r in rows] == [ctl.NO_CORRESPONDENCES] * 2 and np.array_equal(rows[-1]["X"], T0) and np.array_equal(rows[-1]["Y"], T1)
    assert ctl.step(p, tm, ctl.new_state(T0, T1, p), zero)["status"] == ctl.NO_CORRESPONDENCES
    bad = dict(zero, num_inliers=5, error=np.nan)
    rows = run_cpp_step(ct_step_exe, tmp_path, p, tm, T0, T1, [bad])
    assert rows[0]["status"] == ctl.NUMERIC and np.array_equal(rows[0]["X"], T0)
    assert ctl.step(p, tm, ctl.new_state(T0, T1, p), bad)["status"] == ctl.NUMERIC
    # no terms and a zero H with lambda = 0: the Cholesky pivot is not > 0, every trial is rejected whatever its error
    none = ctl.terms()
    p0 = ctl.params(lambda_initial=0.0, max_iterations=2)
    first = dict(zero, num_inliers=5, error=2.0)
    records = [first] + [dict(first, error=1.0)] * 4
    s, trace = ctl.new_state(T0, T1, p0), []
    for L in records:
        s = ctl.step(p0, none, s, L)
        trace.append({"state": s})
    assert [e["state"]["accepted"] for e in trace] == [True, False, False, False, False] and s["status"] == ctl.MAX_TRIALS
    rows = run_cpp_step(ct_step_exe, tmp_path, p0, none, T0, T1, records)
    check_against_restatement(rows, [e["state"] for e in trace], **PAIR)
    assert all(not r["solve_ok"] for r in rows[:-1]) and all(np.array_equal(r["candX"], T0) and np.array_equal(r["candY"], T1) for r in rows)


@pytest.mark.parametrize("name", list(pose_table_cases()))
def test_host_compiled_pose_table_matches_the_restatement(ct_step_exe, tmp_path, name):
    from ct_restatement import moving_source

    table, X, Y = pose_table_cases()[name]
    if table is None:
        table, _ = time_table(moving_source(16, 256)[1][:4001])
        assert 80 <= len(table) <= 90
    fin, fout = str(tmp_path / "poses.bin"), str(tmp_path / "table.bin")
    np.concatenate([pose12(X), pose12(Y), [float(len(table))], table]).tofile(fin)
    out = subprocess.run([ct_step_exe, "poses", fin, fout], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "test_ct_lm_step OK" in out.stdout, out.stdout + out.stderr
    got = np.fromfile(fout).reshape(len(table), 84)
    T, D0, D1 = ct_poses(table, X, Y)
    if name == "series":
        from ct_restatement import logmap

        assert 0 < np.linalg.norm(logmap(np.linalg.inv(X) @ Y)[:3]) < 0.02
    assert np.abs(got[:, :12].reshape(-1, 3, 4) - T[:, :3]).max() < 1e-12
    assert np.abs(got[:, 12:48].reshape(-1, 6, 6) - D0).max() < 1e-12
    assert np.abs(got[:, 48:].reshape(-1, 6, 6) - D1).max() < 1e-12


def test_restated_terms_match_finite_differences():
    """the gradient of a term's cost along right perturbations is 2 b (the convention of tests/test_ct_gicp.py: e = r^T M r without 1/2), and its
    H is the Gauss-Newton J^T J of the same residual"""
    T0, T1 = sweep_poses()
    X = T0 @ expmap([0.01, -0.02, 0.03, 0.1, -0.05, 0.02])
    Y = T1 @ expmap([-0.02, 0.01, 0.05, -0.03, 0.08, 0.01])
    P = T0 @ expmap([0.0, 0.0, 0.004, 0.03, -0.02, 0.0])
    D = expmap(0.7 * np.array([0.001, 0.002, 0.08, 0.9, 0.05, 0.02]))
    eps = 1e-6

    def moved(j, h):
        d = np.zeros(6)
        d[j % 6] = h
        return (X @ expmap(d), Y) if j < 6 else (X, Y @ expmap(d))

    Hp, bp, cp = ctl.location_term(X, P, 1e-3)
    g = np.array([(ctl.location_term(moved(j, eps)[0], P, 1e-3)[2] - ctl.location_term(moved(j, -eps)[0], P, 1e-3)[2]) / (2 * eps) for j in range(6)])
    np.testing.assert_allclose(g, 2 * bp, rtol=1e-6, atol=1e-9 * np.abs(bp).max())
    Hb, bb, cb = ctl.between_term(X, Y, D, 1e3)
    g = np.array([(ctl.between_term(*moved(j, eps), D, 1e3)[2] - ctl.between_term(*moved(j, -eps), D, 1e3)[2]) / (2 * eps) for j in range(12)])
    np.testing.assert_allclose(g, 2 * bb, rtol=1e-6, atol=1e-9 * np.abs(bb).max())
    # H: the derivative of b along the same perturbations, up to the second-order part a Gauss-Newton H leaves out (O(|r|) of H)
    Hn = np.array([(ctl.between_term(*moved(j, eps), D, 1e3)[1] - ctl.between_term(*moved(j, -eps), D, 1e3)[1]) / (2 * eps) for j in range(12)]).T
    r_norm = np.sqrt(cb / 1e3)
    assert np.abs(Hn - Hb).max() <= 2.0 * r_norm * np.abs(Hb).max()
    # the assembled system is the record plus the two terms, the cost (e + c_p) + c_b
    L = ctl.record_of_row(np.concatenate([[7.0, 3.5], np.arange(78.0), np.arange(12.0)]))
    S = ctl.assemble(ctl.terms((P, 1e-3), (D, 1e3)), X, Y, L)
    Hf, bf = np.zeros((12, 12)), np.arange(12.0)
    Hf[np.triu_indices(12)] = np.arange(78.0)
    Hf = Hf + np.triu(Hf, 1).T
    Hf[:6, :6] += Hp
    bf[:6] += bp
    np.testing.assert_allclose(S["H"], Hf + Hb, rtol=1e-15)
    np.testing.assert_allclose(S["b"], bf + bb, rtol=1e-15)
    assert S["cost"] == (3.5 + cp) + cb
    off = ctl.assemble(ctl.terms((P, 0.0), None), X, Y, L)
    assert off["cost"] == 3.5 and off["cost_p"] == 0.0 and off["cost_b"] == 0.0
