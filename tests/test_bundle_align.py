"""Sub-map bundle optimisation (include/glim_amd.h "Sub-map bundle optimisation"), the part that needs no device: the ABI surface, the default
parameters, the argument errors that are answered before any HIP call, glim_amd/csrc/bundle_lm_step.hpp under a plain C++ compiler against
tests/bundle_lm_restatement.py, numpy.linalg and glim_amd_expand_compact, and the C++ mirror."""
import ctypes as C
import os
import re
import subprocess
from functools import partial

import numpy as np
import pytest

import bundle_lm_restatement as blr
import lm_restatement as lmr
from align_cases import ROOT, build_cpp, build_driver, check_symbols, params_head
from align_cases import check_against_restatement as check_rounds
from glim_amd import se3

NEW_STABLE = ["glim_amd_bundle_align_default_params", "glim_amd_bundle_align"]
NEW_DIAG = ["glim_amd_debug_bundle_align_trace"]
INVALID, STATE, UNSUPPORTED = -1, -3, -6
MAX_POSES = 32
EPS = lmr.EPS


def test_new_symbols_are_declared_once_and_listed():
    from glim_amd import _lib, api

    mirror = check_symbols(NEW_STABLE, NEW_DIAG, "bundle_align.hpp")
    assert "glim_amd_bundle_align(" in mirror
    assert '#include "gicp_align.hpp"' in mirror  # LMParams is reused
    head = open(os.path.join(ROOT, "include", "glim_amd.h")).read()
    caps = {k: int(v) for k, v in re.findall(r"#define GLIM_AMD_BUNDLE_(MAX_[A-Z]+) (\d+)", head)}
    assert caps == {"MAX_POSES": _lib.BUNDLE_MAX_POSES, "MAX_FACTORS": _lib.BUNDLE_MAX_FACTORS, "MAX_TERMS": _lib.BUNDLE_MAX_TERMS}
    assert caps["MAX_POSES"] == MAX_POSES >= 20 and caps["MAX_FACTORS"] >= 380
    for n in ("bundle_align", "bundle_align_debug_trace", "bundle_align_params"):
        assert callable(getattr(api, n))
    assert callable(api.NonlinearFactorSetGPU.optimize)
    assert C.sizeof(_lib.BundlePrior) == 8 + 48 * 8 and C.sizeof(_lib.BundleBetween) == 8 + 48 * 8 and C.sizeof(_lib.BundleResult) == 64
    # the rule's header stands alone and is included directly by bundle_align.hip only (tests/test_build_layout.py: what a touch of it recompiles)
    csrc = os.path.join(ROOT, "glim_amd", "csrc")
    users = sorted(f for f in os.listdir(csrc) if f.endswith(".hip") and "bundle_lm_step.hpp" in open(os.path.join(csrc, f)).read())
    assert users == ["bundle_align.hip"]


def test_default_params_are_the_gicp_defaults_with_twenty_iterations():
    from glim_amd import _lib, api

    p, q = _lib.LMParams(), _lib.LMParams()
    assert _lib.lib().glim_amd_bundle_align_default_params(C.byref(p)) == 0
    assert {k: getattr(p, k) for k, _ in _lib.LMParams._fields_} == blr.DEFAULTS == dict(lmr.DEFAULTS, max_iterations=20)
    assert _lib.lib().glim_amd_gicp_align_default_params(C.byref(q)) == 0
    q.max_iterations = 20
    assert bytes(p) == bytes(q)
    assert bytes(api.bundle_align_params()._c()) == bytes(p)
    assert _lib.lib().glim_amd_bundle_align_default_params(None) == INVALID


def test_argument_errors_without_a_device():
    """every refusal that needs no live handle: the checks run before anything of a context or a handle is read"""
    from glim_amd import _lib, api

    L = _lib.lib()
    fn = L.glim_amd_bundle_align
    ctx = C.cast(C.create_string_buffer(64), C.c_void_p)  # never read: every call below is refused (or empty) before the context is used
    out = _lib.BundleResult()
    null2 = (C.c_void_p * 2)(None, None)
    X = np.tile(np.eye(4)[:3].reshape(-1), (3, 1))
    Xo = np.zeros((3, 12))
    idx = lambda *v: np.array(v, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    eye12, eye36 = list(np.eye(4)[:3].reshape(-1)), list(np.eye(6).reshape(-1))

    def prior(pose=0, T=eye12, info=eye36):
        p = (_lib.BundlePrior * 1)()
        p[0].pose = pose
        p[0].T[:] = T
        p[0].information[:] = info
        return p

    def between(i=0, j=1, T=eye12, info=eye36):
        b = (_lib.BundleBetween * 1)()
        b[0].pose_i, b[0].pose_j = i, j
        b[0].T[:] = T
        b[0].information[:] = info
        return b

    def call(ctx=ctx, th=null2, sh=null2, ti=idx(0, 1), si=idx(1, 2), F=0, flags=0, pr=prior(), P=1, be=between(), Q=1, X=dp(X), N=3, prm=None, Xo=dp(Xo), out=out):
        return fn(ctx, th, sh, ti, si, F, flags, pr, P, be, Q, X, N, prm, Xo, None, C.byref(out) if out is not None else None)

    assert call(N=0) == 0 and call(ctx=None, X=None, Xo=None, out=None, pr=None, be=None, N=0) == 0  # no poses: OK
    for kw in (dict(N=-1), dict(F=-1), dict(P=-1), dict(Q=-1)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(ctx=None), dict(X=None), dict(Xo=None), dict(out=None), dict(pr=None), dict(be=None), dict(P=0, Q=0)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(th=None), dict(sh=None), dict(ti=None), dict(si=None), dict()):  # null arrays, then null handles
        assert call(F=2, **kw) == INVALID, kw
    for flags in (api.FACTOR_BINARY, api.FACTOR_BINARY | api.FACTOR_SURFACE_VALIDATION, 4):
        assert call(flags=flags) == INVALID
    for kw in (dict(pr=prior(pose=3)), dict(pr=prior(pose=-1)), dict(be=between(0, 3)), dict(be=between(-1, 1)), dict(be=between(1, 1))):
        assert call(**kw) == INVALID
    nan12, nan36 = [float("nan")] + eye12[1:], eye36[:7] + [float("inf")] + eye36[8:]
    for kw in (dict(pr=prior(T=nan12)), dict(pr=prior(info=nan36)), dict(be=between(T=nan12)), dict(be=between(info=nan36))):
        assert call(**kw) == INVALID
    Xbad = X.copy()
    Xbad[2, 5] = np.nan
    assert call(X=dp(Xbad)) == INVALID
    for field, value in (("lambda_factor", 1.0), ("lambda_initial", float("nan")), ("lambda_initial", -1.0), ("error_scale", 0.0), ("max_iterations", -1),
                         ("max_trials", -1), ("max_trials", 4097), ("max_iterations", 4097), ("lambda_upper_bound", float("inf"))):
        bad = _lib.LMParams()
        L.glim_amd_bundle_align_default_params(C.byref(bad))
        setattr(bad, field, value)
        assert call(prm=C.byref(bad)) == INVALID, field
    # the caps, and a target pose equal to the source pose / out of range (the handles are looked at after the indices of the same factor)
    big = np.tile(np.eye(4)[:3].reshape(-1), (MAX_POSES + 1, 1))
    assert call(X=dp(big), Xo=dp(np.zeros_like(big)), N=MAX_POSES + 1) == UNSUPPORTED
    assert call(F=_lib.BUNDLE_MAX_FACTORS + 1) == UNSUPPORTED and call(P=_lib.BUNDLE_MAX_TERMS + 1) == UNSUPPORTED and call(Q=_lib.BUNDLE_MAX_TERMS + 1) == UNSUPPORTED
    tr = L.glim_amd_debug_bundle_align_trace
    rounds = (_lib.BundleTraceRound * 64)()
    tX = np.zeros((64, 3, 12))
    base = (ctx, null2, null2, idx(0, 1), idx(1, 2), 0, 0, prior(), 1, between(), 1, dp(X), 3, None, dp(Xo), None, C.byref(out), 0)
    assert tr(*base, dp(tX), None, None, None) == INVALID  # a trace without its rounds
    assert tr(*base, None, None, None, rounds) == INVALID
    assert tr(*(base[:12] + (0,) + base[13:]), None, None, None, None) == 0  # no poses
    assert tr(*(base[:6] + (api.FACTOR_BINARY,) + base[7:]), dp(tX), None, None, rounds) == INVALID


# ---- bundle_lm_step.hpp on the host --------------------------------------------------------------------------------------------------------------
CPP = os.path.join(ROOT, "tests", "cpp", "test_bundle_lm_step.cpp")


@pytest.fixture(scope="module")
def step_exe(tmp_path_factory):
    return build_driver(tmp_path_factory, "bundle_lm_step", "-Wno-unknown-pragmas")


def run_cpp(exe, tmp_path, mode, data):
    fin, fout = str(tmp_path / (mode + ".in")), str(tmp_path / (mode + ".out"))
    np.asarray(data, dtype=np.float64).tofile(fin)
    out = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "test_bundle_lm_step OK" in out.stdout, out.stdout + out.stderr
    return np.fromfile(fout)


def pose12(T):
    return np.asarray(T)[:3].reshape(-1)


def pose44(v):
    return np.vstack([np.asarray(v).reshape(3, 4), [0, 0, 0, 1]])


def random_pose(rng, rot=0.5, trans=2.0):
    return lmr.expmap(np.concatenate([rng.normal(0, rot, 3), rng.normal(0, trans, 3)]))


def random_record(rng, error=None, inliers=None):
    A = rng.normal(0, 1, (6, 6))
    H = 40.0 * (A @ A.T) + 10.0 * np.eye(6)
    return {"num_inliers": int(rng.integers(100, 2000)) if inliers is None else inliers, "error": float(rng.uniform(1, 100)) if error is None else error, "H_ss": H,
            "b_s": rng.normal(0, 0.5, 6)}


def random_information(rng):
    A = rng.normal(0, 1, (6, 6))
    L = 30.0 * (A @ A.T) + 5.0 * np.eye(6)
    return L


def test_expansion_equals_expand_compact_bit_for_bit(step_exe, tmp_path):
    from glim_amd import _lib, api

    rng = np.random.default_rng(5)
    n = 64
    recs = np.stack([lmr.compact_of_record(random_record(rng)) * (10.0 ** rng.integers(-3, 4)) for _ in range(n)])
    recs[:, 0] = np.round(rng.uniform(0, 5000, n))
    poses = np.stack([pose12(random_pose(rng, 1.0, 10.0)) for _ in range(n)])
    poses[0] = pose12(np.eye(4))
    got = run_cpp(step_exe, tmp_path, "expand", np.concatenate([[float(n)], np.hstack([recs, poses]).reshape(-1)])).reshape(n, 122)
    for k in range(n):
        want = _lib.Linearized6()
        assert _lib.lib().glim_amd_expand_compact(recs[k].ctypes.data_as(C.POINTER(C.c_double)), poses[k].ctypes.data_as(C.POINTER(C.c_double)), api.FACTOR_BINARY,
                                                  C.byref(want)) == 0
        assert got[k].tobytes() == bytes(want), k


def random_graph(rng, N, lone=None, between_only=None):
    """all pairs i < j but for the poses `lone` (nothing touches it) and `between_only` (between terms only), a prior on pose 0 with a full
    information, a between chain with full informations"""
    skip = {lone, between_only} - {None}
    factors = [(i, j) if (i + j) % 3 else (j, i) for i in range(N) for j in range(i + 1, N) if not ({i, j} & skip)]
    priors = [(0, random_pose(rng, 0.01, 0.01), random_information(rng) * 1e4)]
    chain = [k for k in range(N) if k != lone]
    betweens = [(a, b, random_pose(rng, 0.2, 1.0), random_information(rng)) if q % 2 else (b, a, random_pose(rng, 0.2, 1.0), random_information(rng))
                for q, (a, b) in enumerate(zip(chain[:-1], chain[1:]))]
    return blr.graph(N, factors, priors, betweens)


def cpp_assemble(exe, tmp_path, g, X, recs):
    data = np.concatenate([blr.graph_doubles(g), np.concatenate([pose12(x) for x in X])] + [lmr.compact_of_record(r) for r in recs])
    out = run_cpp(exe, tmp_path, "assemble", data)
    n = 6 * g["N"]
    H = np.zeros((n, n))
    H[np.tril_indices(n)] = out[:n * (n + 1) // 2]
    H = H + np.tril(H, -1).T
    return H, out[n * (n + 1) // 2:n * (n + 1) // 2 + n], out[-5:]


@pytest.mark.parametrize("N,lone,between_only", [(2, None, None), (4, 2, None), (5, 1, 3), (7, None, 6)])
def test_assembly_and_costs_against_the_restatement(step_exe, tmp_path, N, lone, between_only):
    """Both sides run the same FP64 formulas; an entry is a sum of at most 2 N items, each a chain of fewer than 100 roundings of relative size
    EPS against the block's largest entry: 1e-12 of the largest magnitude (the cost gate of tests/test_ct_align.py) holds with two decades to
    spare.  The untouched pose's rows are exact zeros."""
    rng = np.random.default_rng(100 + N)
    g = random_graph(rng, N, lone, between_only)
    X = [random_pose(rng, 0.4, 3.0) for _ in range(N)]
    recs = [random_record(rng) for _ in g["factors"]]
    H, b, tail = cpp_assemble(step_exe, tmp_path, g, X, recs)
    S = blr.assemble(g, np.stack(X), recs)
    assert np.abs(H - S["H"]).max() <= 1e-12 * np.abs(S["H"]).max()
    assert np.abs(b - S["b"]).max() <= 1e-12 * max(np.abs(S["b"]).max(), np.abs(S["H"]).max() * 1e-3)
    for got, key in zip(tail, ("cost", "fcost", "pcost", "bcost", "inliers")):
        assert abs(got - S[key]) <= 1e-12 * abs(S[key]), key
    assert np.array_equal(H, H.T)
    if lone is not None:
        rows = slice(6 * lone, 6 * lone + 6)
        assert not H[rows].any() and not b[rows].any() and not np.signbit(H[rows]).any() and not np.signbit(b[rows]).any()
    if between_only is not None:
        rows = slice(6 * between_only, 6 * between_only + 6)
        assert np.linalg.eigvalsh(H[rows, rows]).min() > 0
        assert all(between_only not in f for f in g["factors"])


def spd_system(rng, n, cond_exp):
    Q, _ = np.linalg.qr(rng.normal(0, 1, (n, n)))
    H = (Q * np.logspace(0, cond_exp, n)) @ Q.T
    return {"H": 0.5 * (H + H.T), "b": rng.normal(0, 1, n)}


@pytest.mark.parametrize("n", [12, 30, 66, 6 * MAX_POSES])
def test_cholesky_solve_against_numpy(step_exe, tmp_path, n):
    rng = np.random.default_rng(n)
    for cond_exp, lam in ((2, 0.0), (6, 1e-5), (9, 1e-3)):
        S = spd_system(rng, n, cond_exp)
        out = run_cpp(step_exe, tmp_path, "solve", np.concatenate([[float(n), lam], blr.packed(S)]))
        ok, d, gate = lmr.solve(S["H"], S["b"], lam)
        assert ok and out[0] == 1.0
        assert np.abs(out[1:] - d).max() <= gate, (n, cond_exp, np.abs(out[1:] - d).max(), gate)


def test_a_pivot_that_is_not_positive_is_a_failed_solve(step_exe, tmp_path):
    rng = np.random.default_rng(3)
    n = 12
    S = spd_system(rng, n, 2)
    for spoil in ("negative", "zero", "nan", "inf"):
        T = {"H": S["H"].copy(), "b": S["b"]}
        if spoil == "negative":
            T["H"][7, 7] = -1.0
        elif spoil == "zero":
            T["H"][0, :] = T["H"][:, 0] = 0.0
        elif spoil == "nan":
            T["H"][5, 5] = np.nan
        else:
            T["H"][5, 5] = np.inf
        out = run_cpp(step_exe, tmp_path, "solve", np.concatenate([[float(n), 0.0], blr.packed(T)]))
        assert out[0] == 0.0 and not out[1:].any(), spoil
    # an untouched pose: a zero block is a failed solve without lambda, and lambda I with a zero step with it
    T = {"H": S["H"].copy(), "b": S["b"].copy()}
    T["H"][6:, :] = T["H"][:, 6:] = 0.0
    T["b"][6:] = 0.0
    assert run_cpp(step_exe, tmp_path, "solve", np.concatenate([[float(n), 0.0], blr.packed(T)]))[0] == 0.0
    out = run_cpp(step_exe, tmp_path, "solve", np.concatenate([[float(n), 1e-5], blr.packed(T)]))
    assert out[0] == 1.0 and not out[7:].any() and out[1:7].any()


def run_cpp_step(exe, tmp_path, p, g, X_init, rounds):
    data = np.concatenate([params_head(p), blr.graph_doubles(g), np.concatenate([pose12(x) for x in X_init]), [float(len(rounds))]] +
                          [lmr.compact_of_record(r) for recs in rounds for r in recs])
    N = g["N"]
    rows = run_cpp(exe, tmp_path, "step", data).reshape(len(rounds), 30 * N + 7)
    poses = lambda v: np.stack([pose44(x) for x in v.reshape(N, 12)])
    return [{"X": poses(r[:12 * N]), "cand": poses(r[12 * N:24 * N]), "delta": r[24 * N:30 * N], "lam": r[30 * N], "solve_ok": bool(r[30 * N + 1]),
             "iterations": int(r[30 * N + 2]), "trials": int(r[30 * N + 3]), "status": int(r[30 * N + 4]), "accepted": bool(r[30 * N + 5]), "cost": r[30 * N + 6]}
            for r in rows]


# align_cases.check_against_restatement over N poses.  Unlike the single-factor loops the two sides ASSEMBLE their systems themselves, and these
# agree to 1e-12 of their scale (the assembly test above), which a solve carries into the step times cond: 1e-12 cond max|delta| =
# gate / (100 EPS) * 1e-12 on top of the gate
check_against_restatement = partial(check_rounds, kept=("X",), gate_scale=1.0 + 1e-12 / (100.0 * EPS))


# scripted sequences: the factors' errors per round (the same for every factor), the parameters, and how the loop must end
SCRIPTS = {
    "accept_then_converged": ([1000.0, 500.0, 450.0], dict(relative_error_tol=0.3), blr.CONVERGED, "AA"),
    "reject_then_accept": ([1000.0, 2000.0, 3000.0, 500.0, 400.0], dict(relative_error_tol=0.3), blr.CONVERGED, "rrAA"),
    "max_iterations": ([1000.0, 500.0, 250.0], dict(max_iterations=2), blr.MAX_ITERATIONS, "AA"),
    "max_trials": ([1000.0, 2000.0, 2000.0, 2000.0], dict(max_trials=3), blr.MAX_TRIALS, "rrr"),
    "lambda_bound": ([1000.0, 2000.0, 2000.0, 2000.0], dict(lambda_initial=1e3), blr.LAMBDA_BOUND, "rrr"),
    "no_correspondences": ([1000.0], dict(), blr.NO_CORRESPONDENCES, ""),
    "numeric": ([1000.0, 500.0, float("nan")], dict(), blr.NUMERIC, "A"),
    "stays_finished": ([1000.0, 500.0, 250.0, 10.0, 5.0], dict(max_iterations=2), blr.MAX_ITERATIONS, "AA"),
}


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_step_decisions_equal_the_restatement(step_exe, tmp_path, name):
    errors, kw, status, decisions = SCRIPTS[name]
    rng = np.random.default_rng(sorted(SCRIPTS).index(name))
    N = 4
    g = random_graph(rng, N, lone=None if name == "numeric" else 2)
    g["priors"] = [(0, np.eye(4), np.eye(6) * 1e4)]
    truth = [random_pose(rng, 0.3, 2.0) for _ in range(N)]
    g["betweens"] = [(i, j, np.linalg.inv(truth[i]) @ truth[j], L) for i, j, _, L in g["betweens"]]
    X0 = [np.linalg.inv(truth[0]) @ x @ lmr.expmap(rng.normal(0, 1e-3, 6)) for x in truth]
    p = blr.params(**kw)
    F = len(g["factors"])
    rounds = [[random_record(rng, error=e / F, inliers=0 if name == "no_correspondences" else None) for _ in range(F)] for e in errors]
    s = blr.new_state(np.stack(X0), p)
    states = []
    for recs in rounds:
        s = blr.step(p, g, s, recs)
        states.append(s)
    assert states[-1]["status"] == status
    assert "".join("A" if t["accepted"] else "r" for t in states[1:len(decisions) + 1]) == decisions
    if name == "stays_finished":
        assert states[2]["status"] == status and states[4]["X"] is states[2]["X"]
    check_against_restatement(run_cpp_step(step_exe, tmp_path, p, g, X0, rounds), states)


def test_terms_alone_converge_to_their_minimum(step_exe, tmp_path):
    """F = 0: there are no inliers to ask for.  A prior and a chain of betweens that agree have their minimum, cost 0, at the chain's poses."""
    rng = np.random.default_rng(11)
    N = 3
    truth = [np.eye(4)] + [random_pose(rng, 0.3, 2.0) for _ in range(N - 1)]
    g = blr.graph(N, [], [(0, truth[0], np.eye(6) * 1e4)], [(k, k + 1, np.linalg.inv(truth[k]) @ truth[k + 1], random_information(rng)) for k in range(N - 1)])
    X0 = [x @ lmr.expmap(rng.normal(0, 0.05, 6)) for x in truth]
    p = blr.params()
    s, trace = blr.run(lambda Tf: [], g, np.stack(X0), p)
    # the last accepted step moved the cost by <= 1e-5 (absolute_error_tol) under quadratic convergence: what is left is far below 1e-8, and
    # with informations >= 5 the poses are within sqrt(1e-8 / 5) < 1e-4
    assert s["status"] == blr.CONVERGED and s["sys"]["cost"] < 1e-8 and np.abs(s["X"] - np.stack(truth)).max() < 1e-4
    rows = run_cpp_step(step_exe, tmp_path, p, g, X0, [[] for _ in trace])
    # a residual is a difference of O(1) pose entries, known to a few EPS; a cost L r^2 with L <= 1e4 and |r| <= 0.1 is then known to
    # 2 * 1e4 * 0.1 * 4 EPS < 1e-12, however small the cost itself has become
    check_against_restatement(rows, [t["state"] for t in trace], cost_floor=1e-12)


def test_the_header_is_clean_under_the_sanitizers(tmp_path):
    """the stand-alone program once more with AddressSanitizer and UndefinedBehaviorSanitizer, over an assembly with an untouched pose, a solve
    at the cap and a scripted loop"""
    exe = str(tmp_path / "test_bundle_lm_step_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-Wno-unknown-pragmas", CPP, "-o", exe])
    rng = np.random.default_rng(2)
    g = random_graph(rng, 5, 1, 3)
    X = [random_pose(rng, 0.4, 3.0) for _ in range(5)]
    recs = [random_record(rng) for _ in g["factors"]]
    cpp_assemble(exe, tmp_path, g, X, recs)
    n = 6 * MAX_POSES
    S = spd_system(rng, n, 3)
    assert run_cpp(exe, tmp_path, "solve", np.concatenate([[float(n), 1e-5], blr.packed(S)]))[0] == 1.0
    p = blr.params(max_iterations=2)
    run_cpp_step(exe, tmp_path, p, g, X, [[random_record(rng, error=e) for _ in g["factors"]] for e in (100.0, 50.0, 60.0, 25.0)])
    run_cpp(exe, tmp_path, "expand", np.concatenate([[1.0], lmr.compact_of_record(recs[0]), pose12(X[0])]))


# ---- the C++ mirror ------------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_compiles_links_and_answers_an_empty_problem(tmp_path):
    """include/glim_amd/bundle_align.hpp: compiled, linked, and run on an empty problem (no device call)"""
    exe = build_cpp(tmp_path, "bundle_align")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "test_bundle_align OK" in out.stdout, out.stdout + out.stderr


def test_se3_module_agrees_with_the_restatement_helpers():
    """the restatement's Log is glim_amd.se3's: Log(Exp(xi)) = xi"""
    xi = np.array([0.3, -0.2, 0.1, 1.0, 2.0, -3.0])
    assert np.abs(se3.se3_log(lmr.expmap(xi)) - xi).max() < 1e-12
