"""NumPy restatement of the step rule of the CT-GICP frame alignment (glim_amd/csrc/ct_lm_step.hpp, include/glim_amd.h "CT-GICP frame
alignment"): Levenberg-Marquardt in fixed-lambda-factor mode over the two poses of a sweep, X (begin) and Y (end), on the continuous-time GICP
factor plus a location prior on X and a between term on X^-1 Y.  12 DoF, tangent order [X: omega v | Y: omega v], right perturbation; the
conventions of tests/ct_restatement.py.  Driven by a `linearize(X, Y) -> record` callable; a record is the dict np_ct_linearize and
IntegratedCT_GICPFactor.linearize return (num_inliers, error, H_00, H_01, H_11, b_0, b_1).  The rule itself -- round 0, accept / reject, the
lambda updates, the statuses, the budgets -- is lm_restatement.decide, called; so are the solve and the pose gate.  A plain module: it holds no
tests."""
import numpy as np

from ct_restatement import _prior, adjoint, expmap_derivative, full_system, logmap
from lm_restatement import (CONVERGED, EPS, LAMBDA_BOUND, MAX_ITERATIONS, MAX_TRIALS, NO_CORRESPONDENCES, NUMERIC, RUNNING, expmap)  # noqa: F401
import lm_restatement as lmr

# the GICP defaults with GLIM's three CT values (odometry_estimation_ct.cpp:176-183)
DEFAULTS = dict(lmr.DEFAULTS, lambda_initial=1e-10, absolute_error_tol=1e-2, max_iterations=8)
ROW = 92


def params(**kw):
    return lmr.params(DEFAULTS, **kw)


def terms(location=None, between=None):
    """(P, k_p) on X and (D, k_b) on X^-1 Y; None or a precision of 0: the term is off"""
    return {"location": location if location is not None and location[1] > 0 else None,
            "between": between if between is not None and between[1] > 0 else None}


def record_of_row(c):
    """the 92 doubles [num_inliers, error, 78 upper entries of H (row-major), 12 of b] -> a record"""
    c = np.asarray(c, dtype=np.float64)
    H = np.zeros((12, 12))
    H[np.triu_indices(12)] = c[2:80]
    H = H + np.triu(H, 1).T
    return {"num_inliers": int(round(c[0])), "error": float(c[1]), "H_00": H[:6, :6].copy(), "H_01": H[:6, 6:].copy(), "H_11": H[6:, 6:].copy(),
            "b_0": c[80:86].copy(), "b_1": c[86:92].copy()}


def row_of_record(L):
    H, b = full_system(L)
    return np.concatenate([[float(L["num_inliers"]), float(L["error"])], H[np.triu_indices(12)], b])


def location_term(X, P, k):
    """-> (H 6 x 6 for [X, X], b 6 for [X], cost)"""
    return _prior(X, P, k)


def between_term(X, Y, D, k):
    """r = Log(D^-1 X^-1 Y), J = [-J_r(r)^-1 Ad((X^-1 Y)^-1) | J_r(r)^-1] -> (H 12 x 12, b 12, cost)"""
    XY = np.linalg.inv(X) @ Y
    r = logmap(np.linalg.inv(D) @ XY)
    Jinv = np.linalg.inv(expmap_derivative(r))
    J = np.hstack([-Jinv @ adjoint(np.linalg.inv(XY)), Jinv])
    return k * J.T @ J, k * J.T @ r, k * r @ r


def assemble(tm, X, Y, L):
    """the system at (X, Y): the record with the terms added -> {H, b, cost, cost_p, cost_b}"""
    H, b = full_system(L)
    H, b = H.copy(), b.copy()
    cp = cb = 0.0
    if tm["location"] is not None:
        Hp, bp, cp = location_term(X, *tm["location"])
        H[:6, :6] += Hp
        b[:6] += bp
    if tm["between"] is not None:
        Hb, bb, cb = between_term(X, Y, *tm["between"])
        H += Hb
        b += bb
    return {"H": H, "b": b, "cost": (L["error"] + cp) + cb, "cost_p": cp, "cost_b": cb}


def _finite(L, X, Y):
    return all(np.all(np.isfinite(np.asarray(x, dtype=np.float64))) for x in (L["error"], full_system(L)[0], full_system(L)[1], X, Y, float(L["num_inliers"])))


def new_state(X_init, Y_init, p):
    X, Y = np.array(X_init, dtype=np.float64), np.array(Y_init, dtype=np.float64)
    return {"X": X, "Y": Y, "rec": None, "sys": None, "lam": p["lambda_initial"], "candX": X.copy(), "candY": Y.copy(), "delta": np.zeros(12), "gate": 0.0,
            "solve_ok": True, "started": False, "iterations": 0, "trials": 0, "status": RUNNING, "accepted": False}


def step(p, tm, s, L):
    """One round: L is the factor's record evaluated at (s['candX'], s['candY']).  Returns the new state (the argument is left alone)."""
    s = dict(s)
    if s["status"] != RUNNING:
        return s
    s["accepted"] = False
    if not _finite(L, s["candX"], s["candY"]):
        s["status"] = NUMERIC
        return s
    S = assemble(tm, s["candX"], s["candY"], L)
    if not (np.all(np.isfinite(S["H"])) and np.all(np.isfinite(S["b"])) and np.isfinite(S["cost"])):
        s["status"] = NUMERIC
        return s
    if lmr.decide(p, s, s["sys"]["cost"] if s["started"] else None, S["cost"], L["num_inliers"] >= 1):
        s["X"], s["Y"], s["rec"], s["sys"] = s["candX"], s["candY"], L, S
    if s["status"] != RUNNING:
        return s
    s["solve_ok"], s["delta"], s["gate"] = lmr.solve(s["sys"]["H"], s["sys"]["b"], s["lam"])
    if s["solve_ok"]:
        s["candX"], s["candY"] = s["X"] @ expmap(s["delta"][:6]), s["Y"] @ expmap(s["delta"][6:])
    else:
        s["candX"], s["candY"] = s["X"], s["Y"]
    if not (np.all(np.isfinite(s["candX"])) and np.all(np.isfinite(s["candY"]))):
        s["status"] = NUMERIC
    return s


def pose_gate(s):
    """lm_restatement.pose_gate over the two retractions X Exp(delta[:6]) and Y Exp(delta[6:])"""
    return lmr.pose_gate(s, ("candX", "candY"))


def run(linearize, X_init, Y_init, tm, p=None):
    """The whole loop -> (final state, trace): one trace entry per round with the pair evaluated (X, Y), the lambda of its step (lam), the
    record, the total cost there, accepted, the status after the round, and `state`, the state after it."""
    p = p or params()
    s = new_state(X_init, Y_init, p)
    trace = []
    for _ in range(1 + p["max_trials"]):
        if s["status"] != RUNNING:
            break
        X, Y, lam = s["candX"], s["candY"], s["lam"]
        L = linearize(X, Y)
        s = step(p, tm, s, L)
        trace.append({"X": X, "Y": Y, "lam": lam, "record": L, "cost": assemble(tm, X, Y, L)["cost"], "accepted": s["accepted"], "status": s["status"],
                      "state": s})
    return s, trace
