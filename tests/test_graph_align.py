"""Global-graph optimisation (include/glim_amd.h "Global-graph optimisation"), the part that needs no device: the ABI surface, the caps, the
default parameters, the argument errors that are answered before any HIP call, the blocked solve of glim_amd/csrc/graph_solve.hpp against
bundle_lm::solve byte for byte under a plain C++ compiler, bundle_lm::step beyond the bundle's cap against tests/bundle_lm_restatement.py, and
the C++ mirror."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bundle_lm_restatement as blr
import lm_restatement as lmr
from align_cases import ROOT, build_cpp, build_driver, check_symbols, params_head
from test_bundle_align import check_against_restatement, pose12, pose44, random_information, random_pose, random_record

NEW_STABLE = ["glim_amd_graph_align_default_params", "glim_amd_graph_align"]
NEW_DIAG = ["glim_amd_debug_graph_align_trace", "glim_amd_debug_graph_solve"]
INVALID, UNSUPPORTED = -1, -6
MAX_POSES, MAX_FACTORS = 256, 32768
TILES = (16, 32, 64)  # graph_solve::tile_ok: the widths the device code can be built with
SIZES = (6, 30, 66, 192, 198, 270, 1536)
CPP = os.path.join(ROOT, "tests", "cpp", "test_graph_solve.cpp")


def test_new_symbols_are_declared_once_and_listed():
    from glim_amd import _lib, api

    mirror = check_symbols(NEW_STABLE, NEW_DIAG, "graph_align.hpp")
    assert "glim_amd_graph_align(" in mirror and '#include "bundle_align.hpp"' in mirror  # the graph, the result and LMParams are reused
    for name in ("BundleGraph", "BundleResult"):
        assert not re.search(r"struct\s+" + name, mirror)
    head = open(os.path.join(ROOT, "include", "glim_amd.h")).read()
    caps = {k: int(v) for k, v in re.findall(r"#define GLIM_AMD_GRAPH_(MAX_[A-Z]+) (\d+)", head)}
    assert caps == {"MAX_POSES": _lib.GRAPH_MAX_POSES, "MAX_FACTORS": _lib.GRAPH_MAX_FACTORS, "MAX_TERMS": _lib.GRAPH_MAX_TERMS}
    assert caps["MAX_POSES"] == MAX_POSES and caps["MAX_FACTORS"] == MAX_FACTORS >= MAX_POSES * (MAX_POSES - 1) // 2 and caps["MAX_TERMS"] >= 1024
    # the device code: the solve's dimension is the cap's, and the unit that checks the arguments ties the header's caps to it
    csrc = os.path.join(ROOT, "glim_amd", "csrc")
    solve = open(os.path.join(csrc, "graph_solve.hpp")).read()
    assert re.search(r"constexpr int MAX_DIM = 6 \* (\d+);", solve).group(1) == str(MAX_POSES)
    assert "static_assert(GLIM_AMD_GRAPH_MAX_POSES * 6 == graph_solve::MAX_DIM" in open(os.path.join(csrc, "bundle_align.hip")).read()
    assert sorted(int(t) for t in re.search(r"TILE == (\d+) \|\| TILE == (\d+) \|\| TILE == (\d+)", solve).groups()) == list(TILES)
    assert os.path.exists(os.path.join(csrc, "graph_solve.hip"))
    for n in ("graph_align", "graph_align_debug_trace", "graph_align_params", "graph_solve_debug"):
        assert callable(getattr(api, n))
    assert callable(api.NonlinearFactorSetGPU.optimize_graph)
    # the bundle keeps its caps
    assert (_lib.BUNDLE_MAX_POSES, _lib.BUNDLE_MAX_FACTORS, _lib.BUNDLE_MAX_TERMS) == (32, 1024, 1024)


def test_default_params_are_the_bundles():
    from glim_amd import _lib, api

    p, q = _lib.LMParams(), _lib.LMParams()
    assert _lib.lib().glim_amd_graph_align_default_params(C.byref(p)) == 0 and _lib.lib().glim_amd_bundle_align_default_params(C.byref(q)) == 0
    assert bytes(p) == bytes(q) and {k: getattr(p, k) for k, _ in _lib.LMParams._fields_} == blr.DEFAULTS
    assert bytes(api.graph_align_params()._c()) == bytes(p)
    assert _lib.lib().glim_amd_graph_align_default_params(None) == INVALID


def test_argument_errors_without_a_device():
    """the refusals of glim_amd_bundle_align with the graph's caps: the checks run before anything of a context or a handle is read"""
    from glim_amd import _lib, api

    L = _lib.lib()
    ctx = C.cast(C.create_string_buffer(64), C.c_void_p)  # never read: every call below is refused (or empty) before the context is used
    out = _lib.BundleResult()
    null2 = (C.c_void_p * 2)(None, None)
    idx = lambda *v: np.array(v, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    eye12, eye36 = list(np.eye(4)[:3].reshape(-1)), list(np.eye(6).reshape(-1))
    poses = lambda n: np.tile(np.eye(4)[:3].reshape(-1), (n, 1))
    X, Xo = poses(3), np.zeros((3, 12))

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

    def call(fn=L.glim_amd_graph_align, ctx=ctx, th=null2, sh=null2, ti=idx(0, 1), si=idx(1, 2), F=0, flags=0, pr=prior(), P=1, be=between(), Q=1, X=dp(X), N=3, prm=None,
             Xo=dp(Xo), out=out):
        return fn(ctx, th, sh, ti, si, F, flags, pr, P, be, Q, X, N, prm, Xo, None, C.byref(out) if out is not None else None)

    assert call(N=0) == 0 and call(ctx=None, X=None, Xo=None, out=None, pr=None, be=None, N=0) == 0  # no poses: OK
    for kw in (dict(N=-1), dict(F=-1), dict(P=-1), dict(Q=-1)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(ctx=None), dict(X=None), dict(Xo=None), dict(out=None), dict(pr=None), dict(be=None), dict(P=0, Q=0)):  # (the last: neither factor nor term)
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
        L.glim_amd_graph_align_default_params(C.byref(bad))
        setattr(bad, field, value)
        assert call(prm=C.byref(bad)) == INVALID, field
    # the caps.  They are looked at before the handles, so with two null handles a size within the caps is refused as INVALID (its arguments
    # were accepted as far as the caps go) and a size over them as UNSUPPORTED
    big = lambda n: dict(X=dp(poses(n)), Xo=dp(np.zeros((n, 12))), N=n)
    assert call(**big(MAX_POSES + 1)) == UNSUPPORTED and call(F=2, **big(MAX_POSES + 1)) == UNSUPPORTED
    for n in (33, MAX_POSES):
        assert call(F=2, **big(n)) == INVALID  # accepted by the caps; the null handles are refused after them
    assert call(fn=L.glim_amd_bundle_align, F=2, **big(33)) == UNSUPPORTED and call(fn=L.glim_amd_bundle_align, F=1025) == UNSUPPORTED  # the bundle keeps its own
    assert call(F=MAX_FACTORS + 1) == UNSUPPORTED and call(P=_lib.GRAPH_MAX_TERMS + 1) == UNSUPPORTED and call(Q=_lib.GRAPH_MAX_TERMS + 1) == UNSUPPORTED
    assert call(F=MAX_FACTORS) == INVALID and call(F=1025) == INVALID  # (null arrays' handles)
    tr = L.glim_amd_debug_graph_align_trace
    rounds = (_lib.BundleTraceRound * 64)()
    tX = np.zeros((64, 3, 12))
    base = (ctx, null2, null2, idx(0, 1), idx(1, 2), 0, 0, prior(), 1, between(), 1, dp(X), 3, None, dp(Xo), None, C.byref(out), 0)
    assert tr(*base, dp(tX), None, None, None, 0) == INVALID  # a trace without its rounds
    assert tr(*base, None, None, None, rounds, 0) == INVALID
    assert tr(*(base[:12] + (0,) + base[13:]), None, None, None, None, 0) == 0  # no poses
    assert tr(*(base[:12] + (0,) + base[13:]), None, None, None, None, -1) == INVALID  # a negative chunk length
    assert tr(*(base[:6] + (api.FACTOR_BINARY,) + base[7:]), dp(tX), None, None, rounds, 0) == INVALID
    assert tr(*(base[:12] + (MAX_POSES + 1,) + base[13:]), None, None, None, None, 0) == UNSUPPORTED
    sv = L.glim_amd_debug_graph_solve
    S, d, ok = np.ones(9), np.zeros(3), C.c_int32()
    for args in ((None, dp(S), 3, 0.0, dp(d), C.byref(ok)), (ctx, None, 3, 0.0, dp(d), C.byref(ok)), (ctx, dp(S), 0, 0.0, dp(d), C.byref(ok)),
                 (ctx, dp(S), 6 * MAX_POSES + 1, 0.0, dp(d), C.byref(ok)), (ctx, dp(S), 3, float("nan"), dp(d), C.byref(ok)), (ctx, dp(S), 3, 0.0, None, C.byref(ok)),
                 (ctx, dp(S), 3, 0.0, dp(d), None)):
        assert sv(*args) == INVALID


# ---- graph_solve.hpp on the host ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solve_exe(tmp_path_factory):
    return build_driver(tmp_path_factory, "graph_solve", "-Wno-unknown-pragmas")


def run_cpp(exe, tmp_path, mode, data):
    fin, fout = str(tmp_path / (mode + ".in")), str(tmp_path / (mode + ".out"))
    np.asarray(data, dtype=np.float64).tofile(fin)
    out = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "test_graph_solve OK" in out.stdout, out.stdout + out.stderr
    return np.fromfile(fout)


def spd_system(rng, n):
    """H = A A^T / n + I / 2 (eigenvalues within [0.5, about 4.5]) and b: the shape of H + lambda I, -b the loop solves"""
    A = rng.normal(0, 1, (n, n))
    return {"H": A @ A.T / n + 0.5 * np.eye(n), "b": rng.normal(0, 1, n)}


def blocked_solve(exe, tmp_path, S, n, lam, tile):
    """-> (ok of bundle_lm::solve, ok of the blocked solve, the same bytes of L / y / delta, the blocked delta)"""
    out = run_cpp(exe, tmp_path, "solve", np.concatenate([[float(n), lam, float(tile)], blr.packed(S)]))
    return bool(out[0]), bool(out[1]), bool(out[2]), bool(out[3]), bool(out[4]), out[5:]


@pytest.mark.parametrize("n", SIZES)
def test_the_blocked_solve_is_the_serial_solve_byte_for_byte(solve_exe, tmp_path, n):
    """the driver walks the panels in the launch order; L, y and delta are compared with memcmp inside it, at every tile width"""
    rng = np.random.default_rng(n)
    S = spd_system(rng, n)
    for tile in TILES:
        ref_ok, ok, same_L, same_y, same_delta, delta = blocked_solve(solve_exe, tmp_path, S, n, 1e-5, tile)
        assert ref_ok and ok and same_L and same_y and same_delta, (n, tile)
        if tile == TILES[0]:  # and the solve solves: the residual of a system whose condition is below 10
            r = (S["H"] + 1e-5 * np.eye(n)) @ delta + S["b"]
            assert np.abs(r).max() <= 1e-9 * max(1.0, np.abs(delta).max()), n


@pytest.mark.parametrize("n", [198, 270])  # an interior tile at every width
def test_a_failed_pivot_anywhere_is_a_failed_solve_with_a_zero_step(solve_exe, tmp_path, n):
    """a zero pivot in the first tile, in an interior tile and in the last, partial tile, and a NaN pivot: ok is false on both
    sides and delta is +0.0 throughout, at every tile width"""
    rng = np.random.default_rng(1000 + n)
    S = spd_system(rng, n)
    for tile in TILES:
        last = ((n - 1) // tile) * tile
        spots = {"first": 3, "interior": tile + tile // 2, "last": last + (n - last) // 2}
        assert spots["interior"] < last < spots["last"] < n
        for name, k in list(spots.items()) + [("nan", spots["interior"])]:
            T = {"H": S["H"].copy(), "b": S["b"]}
            if name == "nan":
                T["H"][k, k] = np.nan
            else:
                T["H"][k, :] = T["H"][:, k] = 0.0
            ref_ok, ok, _, _, same_delta, delta = blocked_solve(solve_exe, tmp_path, T, n, 0.0, tile)
            assert not ref_ok and not ok and same_delta, (n, tile, name)
            assert not delta.any() and not np.signbit(delta).any(), (n, tile, name)
        # with lambda the zeroed row is lambda I: solved, and still the serial solve's bytes
        T = {"H": S["H"].copy(), "b": S["b"].copy()}
        k = spots["interior"]
        T["H"][k, :] = T["H"][:, k] = 0.0
        T["b"][k] = 0.0
        ref_ok, ok, same_L, same_y, same_delta, delta = blocked_solve(solve_exe, tmp_path, T, n, 1e-5, tile)
        assert ref_ok and ok and same_L and same_y and same_delta and delta[k] == 0.0 and delta.any()


# ---- bundle_lm::step beyond the bundle's cap --------------------------------------------------------------------------------------------------
def banded_graph(rng, N, band, lone=()):
    """the factors (i, j), 0 < j - i <= band, every third one with target and source swapped, but for the poses `lone` (nothing touches them); a
    full prior on pose 0; a between chain over the others with full informations"""
    factors = [(i, j) if (i + j) % 3 else (j, i) for i in range(N) for j in range(i + 1, min(N, i + band + 1)) if not ({i, j} & set(lone))]
    chain = [k for k in range(N) if k not in lone]
    betweens = [(a, b, None, random_information(rng)) if q % 2 else (b, a, None, random_information(rng)) for q, (a, b) in enumerate(zip(chain[:-1], chain[1:]))]
    return blr.graph(N, factors, [(0, np.eye(4), np.eye(6) * 1e4)], betweens)


def run_cpp_step(exe, tmp_path, p, g, X_init, rounds):
    data = np.concatenate([params_head(p), blr.graph_doubles(g), np.concatenate([pose12(x) for x in X_init]), [float(len(rounds))]] +
                          [lmr.compact_of_record(r) for recs in rounds for r in recs])
    N = g["N"]
    rows = run_cpp(exe, tmp_path, "step", data).reshape(len(rounds), 30 * N + 7)
    poses = lambda v: np.stack([pose44(x) for x in v.reshape(N, 12)])
    return [{"X": poses(r[:12 * N]), "cand": poses(r[12 * N:24 * N]), "delta": r[24 * N:30 * N], "lam": r[30 * N], "solve_ok": bool(r[30 * N + 1]),
             "iterations": int(r[30 * N + 2]), "trials": int(r[30 * N + 3]), "status": int(r[30 * N + 4]), "accepted": bool(r[30 * N + 5]), "cost": r[30 * N + 6]}
            for r in rows]


@pytest.mark.parametrize("N", [33, 45])
def test_the_step_beyond_the_bundles_cap_equals_the_restatement(solve_exe, tmp_path, N):
    """bundle_lm::step takes N from the graph: the scripted reject-reject-accept-accept loop of tests/test_bundle_align.py at 198 and 270
    rows, with an untouched pose, against the restatement under the same gates"""
    rng = np.random.default_rng(N)
    g = banded_graph(rng, N, 2, lone=(20,))
    truth = [random_pose(rng, 0.3, 2.0) for _ in range(N)]
    g["betweens"] = [(i, j, np.linalg.inv(truth[i]) @ truth[j], L) for i, j, _, L in g["betweens"]]
    X0 = [np.linalg.inv(truth[0]) @ x @ lmr.expmap(rng.normal(0, 1e-3, 6)) for x in truth]
    p = blr.params(relative_error_tol=0.3)
    F = len(g["factors"])
    rounds = [[random_record(rng, error=e / F) for _ in range(F)] for e in (1000.0, 2000.0, 3000.0, 500.0, 400.0)]
    s = blr.new_state(np.stack(X0), p)
    states = []
    for recs in rounds:
        s = blr.step(p, g, s, recs)
        states.append(s)
    assert states[-1]["status"] == blr.CONVERGED and "".join("A" if t["accepted"] else "r" for t in states[1:]) == "rrAA"
    rows = run_cpp_step(solve_exe, tmp_path, p, g, X0, rounds)
    check_against_restatement(rows, states)
    assert not rows[0]["delta"][6 * 20:6 * 21].any() and rows[0]["delta"].any()  # the untouched pose: a zero step


def test_the_driver_is_clean_under_the_sanitizers(tmp_path):
    """the stand-alone program once more with AddressSanitizer and UndefinedBehaviorSanitizer: solves at full, ragged and tiny last tiles, a
    failed pivot, and a step beyond the bundle's cap"""
    exe = str(tmp_path / "test_graph_solve_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-Wno-unknown-pragmas", CPP, "-o", exe])
    rng = np.random.default_rng(4)
    for n, tile in ((6, 64), (66, 16), (192, 64), (198, 32), (270, 64), (270, 16)):
        S = spd_system(rng, n)
        assert all(blocked_solve(exe, tmp_path, S, n, 1e-5, tile)[:5])
        S["H"][n // 2, :] = S["H"][:, n // 2] = 0.0
        out = blocked_solve(exe, tmp_path, S, n, 0.0, tile)
        assert out[:2] == (False, False) and out[4] and not out[5].any()
    N = 33
    g = banded_graph(rng, N, 2, lone=(20, 32))
    g["betweens"] = [(i, j, random_pose(rng, 0.01, 0.01), L) for i, j, _, L in g["betweens"]]
    X = [random_pose(rng, 0.01, 0.01) for _ in range(N)]
    run_cpp_step(exe, tmp_path, blr.params(max_iterations=2), g, X, [[random_record(rng, error=e) for _ in g["factors"]] for e in (100.0, 50.0, 60.0, 25.0)])


# ---- the C++ mirror ------------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_compiles_links_and_answers_an_empty_problem(tmp_path):
    """include/glim_amd/graph_align.hpp: compiled, linked, and run on an empty problem (no device call)"""
    exe = build_cpp(tmp_path, "graph_align")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "test_graph_align OK" in out.stdout, out.stdout + out.stderr
