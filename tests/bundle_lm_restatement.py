"""NumPy restatement of the rule of the sub-map bundle optimisation (glim_amd/csrc/bundle_lm_step.hpp, include/glim_amd.h "Sub-map bundle
optimisation"): Levenberg-Marquardt in fixed-lambda-factor mode over N poses on F binary VGICP factors (evaluated at T_f = X_t^-1 X_s), prior
and between terms.  6N DoF, tangent order [X_0: omega v | X_1: omega v | ...], right perturbation; the conventions of tests/ct_restatement.py.
Driven by a `linearize(Tf) -> records` callable: F relative poses (4 x 4) in, F records out (the dicts of tests/lm_restatement.py: num_inliers,
error, H_ss, b_s).  The rule itself -- round 0, accept / reject, the lambda updates, the statuses, the budgets -- is lm_restatement.decide, called
with the error read as the total cost and the inliers as the factors' sum; so are the solve and the pose gate.  A plain module: it holds no tests."""
import numpy as np

from ct_restatement import adjoint, expmap_derivative, logmap
from lm_restatement import (CONVERGED, EPS, LAMBDA_BOUND, MAX_ITERATIONS, MAX_TRIALS, NO_CORRESPONDENCES, NUMERIC, RUNNING, expmap)  # noqa: F401
import lm_restatement as lmr

DEFAULTS = dict(lmr.DEFAULTS, max_iterations=20)  # the GICP defaults with sub_mapping.cpp:431


def params(**kw):
    return lmr.params(DEFAULTS, **kw)


def graph(N, factors=(), priors=(), betweens=()):
    """factors: (t, s); priors: (pose, P 4 x 4, information 6 x 6); betweens: (i, j, D 4 x 4, information 6 x 6)"""
    return {"N": N, "factors": [tuple(f) for f in factors], "priors": list(priors), "betweens": list(betweens)}


def graph_doubles(g):
    """the graph as tests/cpp/test_bundle_lm_step.cpp reads it"""
    out = [float(g["N"]), float(len(g["factors"])), float(len(g["priors"])), float(len(g["betweens"]))]
    for t, s in g["factors"]:
        out += [float(t), float(s)]
    for k, P, L in g["priors"]:
        out += [float(k)] + list(np.asarray(P)[:3].reshape(-1)) + list(np.asarray(L, dtype=np.float64).reshape(-1))
    for i, j, D, L in g["betweens"]:
        out += [float(i), float(j)] + list(np.asarray(D)[:3].reshape(-1)) + list(np.asarray(L, dtype=np.float64).reshape(-1))
    return np.array(out, dtype=np.float64)


def information(L):
    """only the upper triangle of an information matrix is read"""
    L = np.asarray(L, dtype=np.float64).reshape(6, 6)
    return np.triu(L) + np.triu(L, 1).T


def relative_poses(g, X):
    return [np.linalg.inv(X[t]) @ X[s] for t, s in g["factors"]]


def expand(rec, Tf):
    """the blocks of a binary factor at T_f: glim_amd_expand_compact with GLIM_AMD_FACTOR_BINARY"""
    Ad = adjoint(np.linalg.inv(Tf))
    H_ss, b_s = np.asarray(rec["H_ss"], dtype=np.float64), np.asarray(rec["b_s"], dtype=np.float64)
    H_tt = Ad.T @ H_ss @ Ad
    return {"H_ss": H_ss, "b_s": b_s, "H_tt": 0.5 * (H_tt + H_tt.T), "H_ts": -Ad.T @ H_ss, "b_t": -Ad.T @ b_s}


def prior_term(X, P, L):
    """r = Log(P^-1 X), J = J_r(r)^-1 -> (J^T L J, J^T L r, r^T L r)"""
    L = information(L)
    r = logmap(np.linalg.inv(P) @ X)
    J = np.linalg.inv(expmap_derivative(r))
    return J.T @ L @ J, J.T @ L @ r, r @ L @ r


def between_term(Xi, Xj, D, L):
    """r = Log(D^-1 X_i^-1 X_j), J = [-J_r(r)^-1 Ad((X_i^-1 X_j)^-1) | J_r(r)^-1] -> (H 12 x 12, b 12, cost)"""
    L = information(L)
    XY = np.linalg.inv(Xi) @ Xj
    r = logmap(np.linalg.inv(D) @ XY)
    Jinv = np.linalg.inv(expmap_derivative(r))
    J = np.hstack([-Jinv @ adjoint(np.linalg.inv(XY)), Jinv])
    return J.T @ L @ J, J.T @ L @ r, r @ L @ r


def assemble(g, X, recs):
    """the system at the poses X, recs evaluated at relative_poses(g, X) -> {H, b, cost, fcost, pcost, bcost, inliers}"""
    n = 6 * g["N"]
    H, b = np.zeros((n, n)), np.zeros(n)
    fcost = pcost = bcost = 0.0
    inliers = 0
    for (t, s), rec, Tf in zip(g["factors"], recs, relative_poses(g, X)):
        E = expand(rec, Tf)
        T, S = slice(6 * t, 6 * t + 6), slice(6 * s, 6 * s + 6)
        H[T, T] += E["H_tt"]
        H[S, S] += E["H_ss"]
        H[T, S] += E["H_ts"]
        H[S, T] += E["H_ts"].T
        b[T] += E["b_t"]
        b[S] += E["b_s"]
        fcost += float(rec["error"])
        inliers += int(rec["num_inliers"])
    for k, P, L in g["priors"]:
        Hp, bp, c = prior_term(X[k], P, L)
        K = slice(6 * k, 6 * k + 6)
        H[K, K] += Hp
        b[K] += bp
        pcost += c
    for i, j, D, L in g["betweens"]:
        Hb, bb, c = between_term(X[i], X[j], D, L)
        idx = np.r_[6 * i:6 * i + 6, 6 * j:6 * j + 6]
        H[np.ix_(idx, idx)] += Hb
        b[idx] += bb
        bcost += c
    return {"H": H, "b": b, "cost": (fcost + pcost) + bcost, "fcost": fcost, "pcost": pcost, "bcost": bcost, "inliers": inliers}


def packed(S):
    """the system as bundle_lm_step.hpp keeps it: the lower triangle of H by rows, then b"""
    return np.concatenate([S["H"][np.tril_indices(len(S["b"]))], S["b"]])


def _finite(recs, X):
    return all(np.all(np.isfinite(np.asarray(x, dtype=np.float64)))
               for x in [X] + [v for L in recs for v in (L["error"], L["H_ss"], L["b_s"], float(L["num_inliers"]))])


def new_state(X_init, p):
    X = np.array(X_init, dtype=np.float64)
    return {"X": X, "recs": None, "sys": None, "lam": p["lambda_initial"], "cand": X.copy(), "delta": np.zeros(6 * len(X)), "gate": 0.0, "solve_ok": True,
            "started": False, "iterations": 0, "trials": 0, "status": RUNNING, "accepted": False}


def step(p, g, s, recs):
    """One round: recs are the records evaluated at relative_poses(g, s['cand']).  Returns the new state (the argument is left alone)."""
    s = dict(s)
    if s["status"] != RUNNING:
        return s
    s["accepted"] = False
    if not _finite(recs, s["cand"]):
        s["status"] = NUMERIC
        return s
    S = assemble(g, s["cand"], recs)
    if not (np.all(np.isfinite(S["H"])) and np.all(np.isfinite(S["b"])) and np.isfinite(S["cost"])):
        s["status"] = NUMERIC
        return s
    seen = not g["factors"] or S["inliers"] >= 1
    if lmr.decide(p, s, s["sys"]["cost"] if s["started"] else None, S["cost"], seen):
        s["X"], s["recs"], s["sys"] = s["cand"], recs, S
    if s["status"] != RUNNING:
        return s
    s["solve_ok"], s["delta"], s["gate"] = lmr.solve(s["sys"]["H"], s["sys"]["b"], s["lam"])
    if s["solve_ok"]:
        s["cand"] = np.stack([Xk @ expmap(s["delta"][6 * k:6 * k + 6]) for k, Xk in enumerate(s["X"])])
    else:
        s["cand"] = s["X"]
    if not np.all(np.isfinite(s["cand"])):
        s["status"] = NUMERIC
    return s


def run(linearize, g, X_init, p=None):
    """The whole loop -> (final state, trace): one trace entry per round with the poses evaluated (X), the lambda of its step (lam), the records,
    the total cost there, accepted, the status after the round, and `state`, the state after it."""
    p = p or params()
    s = new_state(X_init, p)
    trace = []
    for _ in range(1 + p["max_trials"]):
        if s["status"] != RUNNING:
            break
        X, lam = s["cand"], s["lam"]
        recs = linearize(relative_poses(g, X))
        s = step(p, g, s, recs)
        trace.append({"X": X, "lam": lam, "records": recs, "cost": assemble(g, X, recs)["cost"], "accepted": s["accepted"], "status": s["status"], "state": s})
    return s, trace
