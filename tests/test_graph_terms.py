"""Damping terms and Huber between terms of the two pose optimisers (include/glim_amd.h "Damping terms and Huber between terms"), the part that
needs no device: the surface, every refusal that is answered before any HIP call, glim_amd/csrc/bundle_lm_step.hpp under a plain C++ compiler
(tests/cpp/test_graph_terms_step.cpp) against tests/graph_terms_restatement.py round by round, against the bytes of the driver from before the
terms (tests/cpp/test_bundle_lm_step.cpp) on graphs without them, and against what the two terms are defined to do."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import graph_terms_restatement as gtr
import lm_restatement as lmr
from align_cases import ROOT, build_cpp, build_driver, check_symbols, params_head
from test_bundle_align import check_against_restatement, pose12, pose44, random_graph, random_information, random_pose, random_record

NEW_STABLE = ["glim_amd_bundle_align_terms", "glim_amd_graph_align_terms"]
NEW_DIAG = ["glim_amd_debug_bundle_align_terms_trace", "glim_amd_debug_graph_align_terms_trace"]
INVALID, UNSUPPORTED = -1, -6
CPP = os.path.join(ROOT, "tests", "cpp", "test_graph_terms_step.cpp")
COND_MAX, WIDTH_MARGIN = 1e9, 1e-6  # the conditions of a comparison between two implementations on the pose-graph scene


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_structs_and_mirrors(tmp_path):
    from glim_amd import _lib, api

    mirror = check_symbols(NEW_STABLE, NEW_DIAG, "bundle_align.hpp")
    for text in ("glim_amd_bundle_align_terms(", "add_damping(int index, double scale)", "add_damping(int index, const std::array<double, 6>& diagonal)",
                 "double huber_width = 0.0", "between_weights"):
        assert text in mirror, text
    graph_mirror = open(os.path.join(ROOT, "include", "glim_amd", "graph_align.hpp")).read()
    assert "glim_amd_graph_align_terms(" in graph_mirror
    # the structs, against the C compiler
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "glim_amd.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(glim_amd_graph_damping), ' \
          "sizeof(glim_amd_graph_terms), offsetof(glim_amd_graph_damping, diagonal), offsetof(glim_amd_graph_terms, between_huber_width)); return 0; }\n"
    (tmp_path / "sizes.c").write_text(src)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "sizes.c"), "-o", str(tmp_path / "sizes")])
    sizes = [int(v) for v in subprocess.check_output([str(tmp_path / "sizes")], text=True).split()]
    assert sizes == [C.sizeof(_lib.GraphDamping), C.sizeof(_lib.GraphTerms), _lib.GraphDamping.diagonal.offset, _lib.GraphTerms.between_huber_width.offset] == [56, 24, 8, 16]
    # the Python mirror
    for n in ("bundle_align", "graph_align", "bundle_align_debug_trace", "graph_align_debug_trace"):
        assert inspect.signature(getattr(api, n)).parameters["dampings"].default == ()
    for n in ("optimize", "optimize_graph"):
        assert inspect.signature(getattr(api.NonlinearFactorSetGPU, n)).parameters["dampings"].default == ()
    assert api.BundleResult(_lib.BundleResult(), np.zeros((0, 4, 4)), np.zeros((0, 29))).between_weights is None
    # what is out of scope now, and what no longer is
    texts = {n: open(os.path.join(ROOT, *n.split("/"))).read() for n in ("include/glim_amd.h", "include/glim_amd/graph_align.hpp", "include/glim_amd/bundle_align.hpp",
                                                                        "README.md", "glim_amd/csrc/bundle_lm_step.hpp")}
    for n, text in texts.items():
        assert "robust kernels" not in text and "LinearDampingFactor, robust" not in text, n
        assert "LinearDampingFactor" in text, n
    for n in ("include/glim_amd.h", "include/glim_amd/graph_align.hpp", "include/glim_amd/bundle_align.hpp", "README.md"):
        assert "pose marginals" in texts[n] and "robust priors" in texts[n], n
    # the rule's header is still included directly by bundle_align.hip alone
    csrc = os.path.join(ROOT, "glim_amd", "csrc")
    users = sorted(f for f in os.listdir(csrc) if f.endswith(".hip") and "bundle_lm_step.hpp" in open(os.path.join(csrc, f)).read())
    assert users == ["bundle_align.hip"]


# ---- the refusals --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,max_terms", [("glim_amd_bundle_align_terms", 1024), ("glim_amd_graph_align_terms", 1024)])
def test_argument_errors_without_a_device(entry, max_terms):
    """every refusal of the new terms: the checks run before anything of a context or a handle is read"""
    from glim_amd import _lib

    fn = getattr(_lib.lib(), entry)
    ctx = C.cast(C.create_string_buffer(64), C.c_void_p)  # never read: every call below is refused before the context is used
    out = _lib.BundleResult()
    null2 = (C.c_void_p * 2)(None, None)
    X = np.tile(np.eye(4)[:3].reshape(-1), (3, 1))
    Xo, wo = np.zeros((3, 12)), np.zeros(1)
    idx = lambda *v: np.array(v, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    be = (_lib.BundleBetween * 1)()
    be[0].pose_i, be[0].pose_j = 0, 1
    be[0].T[:] = list(np.eye(4)[:3].reshape(-1))
    be[0].information[:] = list(np.eye(6).reshape(-1))
    keep = []

    def terms(pose=0, diagonal=(1.0,) * 6, D=1, null=False, width=None):
        d = (_lib.GraphDamping * 1)()
        d[0].pose = pose
        d[0].diagonal[:] = list(diagonal)
        w = np.array([width], dtype=np.float64) if width is not None else None
        keep.extend([d, w])
        return _lib.GraphTerms(None if null else C.cast(d, C.POINTER(_lib.GraphDamping)), D, 0, dp(w) if w is not None else None)

    def call(more, Q=1, N=3):
        return fn(ctx, null2, null2, idx(0, 1), idx(1, 2), 0, 0, None, 0, be, Q, dp(X), N, None, dp(Xo), None, C.byref(out), C.byref(more) if more is not None else None,
                  dp(wo))

    assert call(terms(), N=0) == 0  # no poses: OK, as without the terms
    assert call(None, Q=0) == INVALID  # more == NULL: the refusals of the entry point without the terms
    assert call(terms(D=-1)) == INVALID
    assert call(terms(null=True)) == INVALID
    assert call(terms(pose=3)) == INVALID and call(terms(pose=-1)) == INVALID
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        for m in (0, 5):
            diag = [1.0] * 6
            diag[m] = bad
            assert call(terms(diagonal=diag)) == INVALID, (bad, m)
        assert call(terms(width=bad)) == INVALID, bad
        assert call(terms(D=0, null=True, width=bad)) == INVALID, bad
    assert call(terms(), Q=0) == INVALID  # dampings, but no factor, prior or between: nothing to optimise over
    assert call(terms(D=max_terms + 1)) == UNSUPPORTED  # (answered before a damping is read)
    tr = getattr(_lib.lib(), entry.replace("glim_amd_", "glim_amd_debug_") + "_trace")
    more = terms(pose=3)
    base = (ctx, null2, null2, idx(0, 1), idx(1, 2), 0, 0, None, 0, be, 1, dp(X), 3, None, dp(Xo), None, C.byref(out), C.byref(more), dp(wo), 0, None, None, None, None)
    assert tr(*base, *((0,) if "graph" in entry else ())) == INVALID
    if "graph" in entry:
        assert tr(*base[:17], None, None, 0, None, None, None, None, -1) == INVALID  # a negative chunk length


# ---- bundle_lm_step.hpp on the host --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def step_exe(tmp_path_factory):
    return build_driver(tmp_path_factory, "graph_terms_step", "-Wno-unknown-pragmas")


@pytest.fixture(scope="module")
def old_exe(tmp_path_factory):
    return build_driver(tmp_path_factory, "bundle_lm_step", "-Wno-unknown-pragmas")


def run_cpp(exe, tmp_path, mode, data, name="test_graph_terms_step"):
    fin, fout = str(tmp_path / (mode + ".in")), str(tmp_path / (mode + ".out"))
    np.asarray(data, dtype=np.float64).tofile(fin)
    out = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and name + " OK" in out.stdout, out.stdout + out.stderr
    return np.fromfile(fout)


def cpp_assemble(exe, tmp_path, g, X, recs=()):
    """-> H, b, the five costs, the weights, the betweens' stored contributions (Q x 157)"""
    data = np.concatenate([gtr.graph_doubles(g), np.concatenate([pose12(x) for x in X])] + [lmr.compact_of_record(r) for r in recs])
    out = run_cpp(exe, tmp_path, "assemble_terms", data)
    n, Q = 6 * g["N"], len(g["betweens"])
    nt = n * (n + 1) // 2
    H = np.zeros((n, n))
    H[np.tril_indices(n)] = out[:nt]
    H = H + np.tril(H, -1).T
    assert len(out) == nt + n + 5 + 158 * Q
    return H, out[nt:nt + n], out[nt + n:nt + n + 5], out[nt + n + 5:nt + n + 5 + Q], out[nt + n + 5 + Q:].reshape(Q, 157)


def cpp_step(exe, tmp_path, p, g, X_init, rounds):
    data = np.concatenate([params_head(p), gtr.graph_doubles(g), np.concatenate([pose12(x) for x in X_init]), [float(len(rounds))]] +
                          [lmr.compact_of_record(r) for recs in rounds for r in recs])
    N, Q = g["N"], len(g["betweens"])
    rows = run_cpp(exe, tmp_path, "step_terms", data).reshape(len(rounds), 30 * N + 7 + Q)
    poses = lambda v: np.stack([pose44(x) for x in v.reshape(N, 12)])
    return [{"X": poses(r[:12 * N]), "cand": poses(r[12 * N:24 * N]), "delta": r[24 * N:30 * N], "lam": r[30 * N], "solve_ok": bool(r[30 * N + 1]),
             "iterations": int(r[30 * N + 2]), "trials": int(r[30 * N + 3]), "status": int(r[30 * N + 4]), "accepted": bool(r[30 * N + 5]), "cost": r[30 * N + 6],
             "weights": r[30 * N + 7:]} for r in rows]


def check_weights(got, want):
    """exactly 1.0 where the reference says 1.0; elsewhere w = k / s with s a square root of a sum both sides know to 1e-12: 1e-9 is the gate"""
    want = np.asarray(want)
    assert np.array_equal(got[want == 1.0], want[want == 1.0]) and np.abs(got - want).max() <= 1e-9, (got, want)


@pytest.mark.parametrize("N", [8, 33])  # within the bundle's cap, and the first size beyond it
def test_the_header_follows_the_restatement_on_the_pose_graph_scene(step_exe, tmp_path, N):
    """Round by round, with the tolerances tests/test_bundle_align.py has for the same comparison.  What the comparison rests on is asserted on
    the restatement's own run: no between within 1e-6 (relative) of its width at any trial -- the two sides would otherwise be free to
    down-weight it or not -- and cond(H) <= 1e9 at the kept system."""
    g, _, _, X0, _ = gtr.ring_scene(N)
    p = gtr.params()
    s, trace = gtr.run(lambda Tf: [], g, X0, p)
    print("N", N, "status", s["status"], "accepted", s["iterations"], "trials", s["trials"], "weights", s["sys"]["weights"][N - 1:], "margin", gtr.width_margin(g, trace),
          "cond", np.linalg.cond(s["sys"]["H"]), "pose 0 moves", np.abs(s["X"][0] - X0[0]).max())
    assert gtr.width_margin(g, trace) > WIDTH_MARGIN and all(np.linalg.cond(e["state"]["sys"]["H"]) <= COND_MAX for e in trace)
    assert s["status"] == gtr.CONVERGED and s["sys"]["weights"][N].item() < 0.5 and np.count_nonzero(s["sys"]["weights"] != 1.0) == 1
    assert np.abs(s["X"][0] - X0[0]).max() < 1e-9
    rows = cpp_step(step_exe, tmp_path, p, g, X0, [[] for _ in trace])
    check_against_restatement(rows, [e["state"] for e in trace], cost_floor=1e-12)
    for k, (row, e) in enumerate(zip(rows, trace)):
        check_weights(row["weights"], e["state"]["sys"]["weights"])  # the weights of the KEPT evaluation
    assert np.abs(rows[-1]["X"][0] - X0[0]).max() < 1e-9


def test_without_a_new_term_the_bytes_are_those_of_the_driver_from_before(step_exe, old_exe, tmp_path):
    """the same graph, poses and records through tests/cpp/test_bundle_lm_step.cpp: `assemble` and `step`, with no term array at all and with
    a width array of zeros"""
    rng = np.random.default_rng(21)
    g = random_graph(rng, 5, 1, 3)
    X = [random_pose(rng, 0.4, 3.0) for _ in range(5)]
    recs = [random_record(rng) for _ in g["factors"]]
    Q = len(g["betweens"])
    tails = {"none": [0.0, 0.0], "zero widths": [0.0, 1.0] + [0.0] * Q}
    old = np.concatenate([gtr.blr.graph_doubles(g), np.concatenate([pose12(x) for x in X])] + [lmr.compact_of_record(r) for r in recs])
    want = run_cpp(old_exe, tmp_path, "assemble", old, "test_bundle_lm_step")
    for name, tail in tails.items():
        new = np.concatenate([gtr.blr.graph_doubles(g), tail, np.concatenate([pose12(x) for x in X])] + [lmr.compact_of_record(r) for r in recs])
        assert run_cpp(step_exe, tmp_path, "assemble", new).tobytes() == want.tobytes(), name
    p = gtr.params(max_iterations=2)
    rounds = [[random_record(rng, error=e) for _ in g["factors"]] for e in (100.0, 50.0, 60.0, 25.0)]
    body = [np.concatenate([pose12(x) for x in X]), [float(len(rounds))]] + [lmr.compact_of_record(r) for rs in rounds for r in rs]
    want = run_cpp(old_exe, tmp_path, "step", np.concatenate([params_head(p), gtr.blr.graph_doubles(g)] + body), "test_bundle_lm_step")
    assert len(want) == len(rounds) * (30 * 5 + 7) and want.any()
    for name, tail in tails.items():
        got = run_cpp(step_exe, tmp_path, "step", np.concatenate([params_head(p), gtr.blr.graph_doubles(g), tail] + body))
        assert got.tobytes() == want.tobytes(), name


def small_graph(rng, widths, dampings=()):
    """three poses, a prior, two betweens with full informations whose residuals are large: s is about 13 and 9"""
    truth = [random_pose(rng, 0.3, 2.0) for _ in range(3)]
    betweens = [(0, 1, np.linalg.inv(truth[0]) @ truth[1], random_information(rng)), (2, 1, np.linalg.inv(truth[2]) @ truth[1], random_information(rng))]
    X = [x @ lmr.expmap(rng.normal(0, 0.2, 6)) for x in truth]
    return gtr.graph(3, [], [(0, truth[0], random_information(rng))], [b + (w,) for b, w in zip(betweens, widths)], dampings), X


def test_a_between_under_its_width_is_the_gaussian_between_and_over_it_is_w_times_it(step_exe, tmp_path):
    seed = 4
    g0, X = small_graph(np.random.default_rng(seed), (0.0, 0.0))
    H0, b0, c0, w0, bc0 = cpp_assemble(step_exe, tmp_path, g0, X)
    s = np.sqrt(bc0[:, 156])
    print("s", s)
    assert np.array_equal(w0, [1.0, 1.0]) and s.min() > 2.0
    # s <= k (the second at s == k exactly): the bits of the Gaussian between
    g1, _ = small_graph(np.random.default_rng(seed), (1e3, s[1]))
    H1, b1, c1, w1, bc1 = cpp_assemble(step_exe, tmp_path, g1, X)
    assert np.array_equal(w1, [1.0, 1.0]) and bc1.tobytes() == bc0.tobytes() and H1.tobytes() == H0.tobytes() and b1.tobytes() == b0.tobytes() and c1.tobytes() == c0.tobytes()
    # s > k on the first, Gaussian on the second
    k = 1.5
    g2, _ = small_graph(np.random.default_rng(seed), (k, 0.0))
    H2, b2, c2, w2, bc2 = cpp_assemble(step_exe, tmp_path, g2, X)
    w = k / s[0]
    assert np.array_equal(w2, [w, 1.0]) and w < 0.5
    assert np.array_equal(bc2[0, :156], w * bc0[0, :156]) and bc2[0, 156] == k * ((s[0] + s[0]) - k)  # each stored value once times w
    assert bc2[1].tobytes() == bc0[1].tobytes()
    assert c2[3] == (0.0 + bc2[0, 156]) + bc2[1, 156] and c2[0] == (c2[1] + c2[2]) + c2[3] and c2[2] == c0[2]
    S = gtr.assemble(g2, np.stack(X), [])
    assert np.abs(H2 - S["H"]).max() <= 1e-12 * np.abs(S["H"]).max() and np.abs(b2 - S["b"]).max() <= 1e-12 * max(np.abs(S["b"]).max(), np.abs(S["H"]).max() * 1e-3)
    assert abs(c2[0] - S["cost"]) <= 1e-12 * S["cost"] and abs(w2[0] - S["weights"][0]) <= 1e-12


def test_the_robust_cost_has_the_gradient_two_b(step_exe, tmp_path):
    """A central difference of the total cost along each tangent direction (right perturbation, step h = 1e-5) against 2 b.  The difference's
    truncation error is h^2 / 6 times a third derivative, of the size of |b| itself for these O(1) residuals: 2e-11 |b|; its rounding error is
    EPS cost / h = 2.2e-11 cost, with cost < 20 |b|max here (printed): under 1e-9 |b|max together.  The gate is 1e-6 |b|max: a term left
    unweighted, or a weight applied twice, moves an entry by more than 0.1 |b|."""
    g, X = small_graph(np.random.default_rng(4), (1.5, 0.0), [(1, 3.0)])
    _, b, c, w, _ = cpp_assemble(step_exe, tmp_path, g, X)
    assert w[0] < 0.5 and w[1] == 1.0
    h = 1e-5
    grad = np.zeros(18)
    for u in range(18):
        e = np.zeros(6)
        e[u % 6] = h
        cost = []
        for sign in (1.0, -1.0):
            Y = list(X)
            Y[u // 6] = X[u // 6] @ lmr.expmap(sign * e)
            cost.append(cpp_assemble(step_exe, tmp_path, g, Y)[2][0])
        grad[u] = (cost[0] - cost[1]) / (2 * h)
    print("cost", c[0], "|b|max", np.abs(b).max(), "worst", np.abs(grad - 2 * b).max())
    assert c[0] < 20 * np.abs(b).max()
    assert np.abs(grad - 2 * b).max() <= 1e-6 * np.abs(b).max()


def test_a_damping_changes_six_diagonal_entries_and_nothing_else(step_exe, tmp_path):
    rng = np.random.default_rng(9)
    g0, X = small_graph(np.random.default_rng(9), (1.5, 0.0))
    d1, d2 = rng.uniform(0.5, 2.0, 6) * 1e3, 7.0
    g1, _ = small_graph(np.random.default_rng(9), (1.5, 0.0), [(1, d1), (1, d2)])  # two on one pose
    g1["N"] = g0["N"] = 4  # and a pose that only a damping touches
    g1["dampings"].append((3, gtr.diagonal(5.0)))
    X = X + [random_pose(rng)]
    H0, b0, c0, w0, bc0 = cpp_assemble(step_exe, tmp_path, g0, X)
    H1, b1, c1, w1, bc1 = cpp_assemble(step_exe, tmp_path, g1, X)
    want = H0.copy()
    for m in range(6):
        want[6 + m, 6 + m] = (H0[6 + m, 6 + m] + d1[m]) + d2  # after the betweens, by ascending index
        want[18 + m, 18 + m] = 5.0
    assert H1.tobytes() == want.tobytes() and b1.tobytes() == b0.tobytes() and c1.tobytes() == c0.tobytes() and bc1.tobytes() == bc0.tobytes()
    assert not b1[18:].any() and not np.signbit(b1[18:]).any() and not np.signbit(H1[18:]).any()
    # the lone damped pose: a zero step, its bits unchanged in every candidate
    p = gtr.params(max_iterations=3)
    rows = cpp_step(step_exe, tmp_path, p, g1, X, [[]] * 4)
    assert rows[-1]["iterations"] >= 2 and all(np.array_equal(r["cand"][3], X[3]) and np.array_equal(r["X"][3], X[3]) and not r["delta"][18:].any() for r in rows)
    s = gtr.blr.new_state(np.stack(X), p)
    states = []
    for _ in range(4):
        s = gtr.step(p, g1, s, [])
        states.append(s)
    check_against_restatement(rows, states)


def test_the_header_with_the_terms_is_clean_under_the_sanitizers(tmp_path):
    """the stand-alone program once more with AddressSanitizer and UndefinedBehaviorSanitizer, over the N = 8 scene and a damped graph"""
    exe = str(tmp_path / "test_graph_terms_step_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-Wno-unknown-pragmas", CPP, "-o", exe])
    g, _, _, X0, _ = gtr.ring_scene(8)
    rows = cpp_step(exe, tmp_path, gtr.params(max_iterations=3), g, X0, [[]] * 4)
    assert rows[-1]["iterations"] == 3 and rows[-1]["weights"][8] < 1.0
    cpp_assemble(exe, tmp_path, g, X0)
    rng = np.random.default_rng(2)
    gf = random_graph(rng, 5, 1, 3)
    gf = gtr.graph(5, gf["factors"], gf["priors"], [b + (2.0,) for b in gf["betweens"]], [(1, 10.0), (4, [1, 2, 3, 4, 5, 6])])
    X = [random_pose(rng, 0.4, 3.0) for _ in range(5)]
    cpp_assemble(exe, tmp_path, gf, X, [random_record(rng) for _ in gf["factors"]])


# ---- the C++ mirror ------------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_records_the_terms_and_answers_an_empty_problem(tmp_path):
    """include/glim_amd/bundle_align.hpp and graph_align.hpp: add_damping in both forms, add_between's width, the choice of the entry point;
    compiled, linked, and run on an empty problem (no device call)"""
    exe = build_cpp(tmp_path, "graph_terms_mirror")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "test_graph_terms_mirror OK" in out.stdout, out.stdout + out.stderr
