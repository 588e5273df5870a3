"""Velocity and bias variables, vector priors, vector betweens and IMU terms of the graph optimiser (include/glim_amd.h "Graph optimisation with
velocity and bias variables"), the part that needs no device: the surface, every refusal that is answered before any HIP call, the IMU term of
glim_amd/csrc/nav_terms.hpp against a 200-bit restatement (residual and Jacobian), the gradient of the assembled cost, the header-driven loop
(tests/cpp/test_nav_graph_step.cpp, a plain C++ compiler) against tests/nav_graph_restatement.py round by round, the bytes of graphs without a
new term against the driver from before the terms, and the stand-alone driver under the sanitizers."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import graph_terms_restatement as gtr
import lm_restatement as lmr
import nav_graph_restatement as nr
from align_cases import PERT_A, ROOT, build_cpp, build_driver, check_against_restatement, check_symbols, params_head
from test_bundle_align import pose12, random_graph, random_pose, random_record
from test_gicp import POSE_TOL
from test_graph_terms import COND_MAX

NEW_STABLE = ["glim_amd_graph_align_nav"]
NEW_DIAG = ["glim_amd_debug_graph_align_nav_trace"]
INVALID, UNSUPPORTED = -1, -6
CPP = os.path.join(ROOT, "tests", "cpp", "test_nav_graph_step.cpp")
# the worst errors of the IMU term against the 200-bit restatement over reference_cases(), measured on the host (see the two tests)
RESIDUAL_WORST, JACOBIAN_WORST = 3.4e-16, 3.6e-16


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_structs_and_mirrors(tmp_path):
    from glim_amd import _lib, api

    mirror = check_symbols(NEW_STABLE, NEW_DIAG, "graph_align.hpp")
    for text in ("glim_amd_graph_align_nav(", "struct NavGraph", "struct ImuTerm", "optimize_nav_graph(const NavGraph& g", "add_velocity_prior", "add_bias_between",
                 "add_imu(const ImuTerm& t)"):
        assert text in mirror, text
    names = ["glim_amd_nav_vector_prior", "glim_amd_nav_vector_between", "glim_amd_nav_imu_term", "glim_amd_nav_terms", "glim_amd_nav_result"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "glim_amd.h"\nint main(void) { printf("' + "%zu " * 10 + '\\n", ' + \
          ", ".join("sizeof(%s)" % n for n in names) + ", offsetof(glim_amd_nav_imu_term, dt), offsetof(glim_amd_nav_imu_term, information), " \
          "offsetof(glim_amd_nav_terms, num_vector_priors), offsetof(glim_amd_nav_result, num_inliers), offsetof(glim_amd_nav_result, lambda)); return 0; }\n"
    (tmp_path / "sizes.c").write_text(src)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "sizes.c"), "-o", str(tmp_path / "sizes")])
    sizes = [int(v) for v in subprocess.check_output([str(tmp_path / "sizes")], text=True).split()]
    mine = [C.sizeof(_lib.NavVectorPrior), C.sizeof(_lib.NavVectorBetween), C.sizeof(_lib.NavImuTerm), C.sizeof(_lib.NavTerms), C.sizeof(_lib.NavResult),
            _lib.NavImuTerm.dt.offset, _lib.NavImuTerm.information.offset, _lib.NavTerms.num_vector_priors.offset, _lib.NavResult.num_inliers.offset,
            _lib.NavResult.lam.offset]
    assert sizes == mine == [344, 344, 1256, 48, 88, 24, 608, 32, 56, 80]
    header = open(os.path.join(ROOT, "include", "glim_amd.h")).read()
    for name, value in (("NODE_POSE", 0), ("NODE_BIAS", 1), ("NODE_VELOCITY", 2), ("IMU_TANGENT", 0), ("IMU_MANIFOLD", 1)):
        assert "#define GLIM_AMD_%s %d\n" % (name, value) in header and getattr(api, name) == getattr(_lib, name) == getattr(nr, name.split("_", 1)[1]) == value
    # the Python mirror
    sig = inspect.signature(api.graph_align_nav).parameters
    assert list(sig)[:5] == ["factors", "priors", "betweens", "nodes_init", "kinds"]
    for n in ("vector_priors", "vector_betweens", "imu_terms", "dampings"):
        assert sig[n].default == ()
    assert inspect.signature(api.graph_align_nav_debug_trace).parameters["one_thread"].default is False
    assert "imu_terms" in inspect.signature(api.NonlinearFactorSetGPU.optimize_nav_graph).parameters
    t = api.ImuTerm(0, 1, 3, 4, 2, 0.1, nr.GRAVITY, np.zeros(6), np.zeros(9), np.zeros((9, 6)), np.eye(9), api.IMU_MANIFOLD)
    c = _lib.NavImuTerm()
    t._fill(c)
    assert (c.pose_i, c.velocity_i, c.pose_j, c.velocity_j, c.bias, c.mode, c.dt, c.gravity[2], c.information[80]) == (0, 1, 3, 4, 2, 1, 0.1, -9.81, 1.0)
    # what is out of scope now, where the definition is upstream recall, and the call sites of the entry point's comment
    texts = {n: open(os.path.join(ROOT, *n.split("/"))).read() for n in ("include/glim_amd.h", "include/glim_amd/graph_align.hpp", "README.md",
                                                                        "glim_amd/csrc/bundle_lm_step.hpp", "glim_amd/csrc/nav_terms.hpp", "INTEGRATION.md")}
    for n in ("include/glim_amd.h", "include/glim_amd/graph_align.hpp", "README.md", "glim_amd/csrc/bundle_lm_step.hpp", "glim_amd/csrc/nav_terms.hpp"):
        assert "CombinedImuFactor" in texts[n], n
        assert "IMU variables" not in texts[n] and "IMU graphs (V, B variables, ImuFactor)" not in texts[n], n
    for n in ("include/glim_amd.h", "glim_amd/csrc/nav_terms.hpp"):
        assert "UPSTREAM RECALL" in texts[n], n
    assert "unverified against gtsam" in texts["INTEGRATION.md"]
    assert "32 blocks hold only ten frames" in texts["include/glim_amd.h"]
    for site in ("sub_mapping.cpp:218-243", "global_mapping.cpp:168-216", "odometry_estimation_imu.cpp:218-220", "loose_initial_state_estimation.cpp:105-124"):
        assert site in texts["include/glim_amd.h"], site
    csrc = os.path.join(ROOT, "glim_amd", "csrc")
    users = sorted(f for f in os.listdir(csrc) if f.endswith(".hip") and "bundle_lm_step.hpp" in open(os.path.join(csrc, f)).read())
    assert users == ["bundle_align.hip"]


# ---- the refusals --------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_without_a_device():
    """every refusal of the node kinds and the new terms: the checks run before anything of a context or a handle is read"""
    from glim_amd import _lib

    fn = _lib.lib().glim_amd_graph_align_nav
    ctx = C.cast(C.create_string_buffer(64), C.c_void_p)  # never read: every call below is refused before the context is used
    out = _lib.NavResult()
    null2 = (C.c_void_p * 2)(None, None)
    idx = lambda *v: np.array(v, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    eye12 = np.eye(4)[:3].reshape(-1)
    KINDS = [0, 2, 1, 0, 2, 1]  # X V B X V B
    keep = []

    def rows(kinds, velocity_tail=0.0, bias_tail=0.0, at=3):
        X = np.zeros((len(kinds), 12))
        for k, kind in enumerate(kinds):
            if kind == 0:
                X[k] = eye12
            elif kind == 2:
                X[k, :3], X[k, at] = [1.0, 2.0, 3.0], velocity_tail
            else:
                X[k, :6], X[k, 6 + (at - 3)] = np.arange(6) * 0.01, bias_tail
        return X

    def call(kinds=KINDS, X=None, vp=None, vb=None, imu=None, counts=None, nav_null=False, F=0, Q=0, between=(0, 3), prior=None, factor=(0, 3), D=0, damp_node=2,
             result=True, null_arrays=False):
        X = rows(kinds) if X is None else X
        N = len(X)
        Xo = np.zeros((N, 12))
        ck = np.array(kinds, dtype=np.int32)
        cp, cb, ci = (_lib.NavVectorPrior * 1)(), (_lib.NavVectorBetween * 1)(), (_lib.NavImuTerm * 1)()
        cp[0].node = 2
        cp[0].information[:] = list(np.eye(6).reshape(-1))
        cb[0].node_i, cb[0].node_j = 2, 5
        cb[0].information[:] = list(np.eye(6).reshape(-1))
        ci[0].pose_i, ci[0].velocity_i, ci[0].pose_j, ci[0].velocity_j, ci[0].bias, ci[0].mode, ci[0].dt = 0, 1, 3, 4, 2, 0, 0.1
        ci[0].information[:] = list(np.eye(9).reshape(-1))
        for struct, changes in ((cp[0], vp), (cb[0], vb), (ci[0], imu)):
            for name, value in (changes or {}).items():
                if isinstance(value, tuple):  # (index, value) into an array member
                    getattr(struct, name)[value[0]] = value[1]
                else:
                    setattr(struct, name, value)
        n = counts if counts is not None else (1 if vp is not None else 0, 1 if vb is not None else 0, 1 if imu is not None else 0)
        nav = _lib.NavTerms(ck.ctypes.data_as(C.POINTER(C.c_int32)), None if null_arrays else C.cast(cp, C.POINTER(_lib.NavVectorPrior)),
                            None if null_arrays else C.cast(cb, C.POINTER(_lib.NavVectorBetween)), None if null_arrays else C.cast(ci, C.POINTER(_lib.NavImuTerm)),
                            n[0], n[1], n[2], 0)
        be = (_lib.BundleBetween * 1)()
        be[0].pose_i, be[0].pose_j = between
        be[0].T[:], be[0].information[:] = list(eye12), list(np.eye(6).reshape(-1))
        pr = (_lib.BundlePrior * 1)()
        pr[0].pose = prior if prior is not None else 0
        pr[0].T[:], pr[0].information[:] = list(eye12), list(np.eye(6).reshape(-1))
        d = (_lib.GraphDamping * 1)()
        d[0].pose = damp_node
        d[0].diagonal[:] = [1e6] * 6
        more = _lib.GraphTerms(C.cast(d, C.POINTER(_lib.GraphDamping)), D, 0, None)
        keep.extend([X, Xo, ck, cp, cb, ci, be, pr, d])
        return fn(ctx, null2, null2, idx(*factor), idx(factor[1], factor[0]), F, 0, pr, 1 if prior is not None else 0, be, Q, dp(X), N, None, dp(Xo), None,
                  C.byref(out) if result else None, C.byref(more), None, None if nav_null else C.byref(nav))

    ok = dict(vp={}, vb={}, imu={})
    # an unknown kind or mode
    assert call(kinds=[0, 2, 3, 0, 2, 1], vp={"node": 5}) == INVALID and call(kinds=[0, -1, 1, 0, 2, 1], vp={}) == INVALID
    assert call(imu={"mode": 2}) == INVALID and call(imu={"mode": -1}) == INVALID
    # a term naming a node of the wrong kind, or out of range
    for node in (0, 6, -1):
        assert call(vp={"node": node}) == INVALID, node
    assert call(vb={"node_i": 1}) == INVALID and call(vb={"node_j": 0}) == INVALID and call(vb={"node_j": 6}) == INVALID  # V with B, a pose, out of range
    for field, bad in (("pose_i", 1), ("pose_j", 2), ("velocity_i", 0), ("velocity_j", 5), ("bias", 4), ("bias", 6), ("pose_i", -1)):
        assert call(imu={field: bad}) == INVALID, (field, bad)
    assert call(Q=1, between=(0, 1)) == INVALID and call(Q=1, between=(2, 3), vp={}) == INVALID  # a pose between on a velocity, on a bias
    assert call(prior=1, vp={}) == INVALID  # a pose prior on a vector node (a factor on one: tests/test_nav_graph_gpu.py, it needs handles)
    # repeated nodes in one term
    assert call(vb={"node_j": 2}) == INVALID and call(imu={"pose_j": 0}) == INVALID and call(imu={"velocity_j": 1}) == INVALID
    # dt
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        assert call(imu={"dt": bad}) == INVALID, bad
    # any input that is not finite
    for bad in (float("nan"), float("inf"), -float("inf")):
        for field, n in (("gravity", 3), ("bias_hat", 6), ("delta", 9), ("H_bias", 54), ("information", 81)):
            assert call(imu={field: (n - 1, bad)}) == INVALID, (field, bad)
        assert call(vp={"value": (5, bad)}) == INVALID and call(vp={"information": (35, bad)}) == INVALID
        assert call(vb={"measurement": (0, bad)}) == INVALID and call(vb={"information": (7, bad)}) == INVALID
        X = rows(KINDS)
        X[4, 1] = bad
        assert call(X=X, vp={}) == INVALID
    # a VELOCITY row whose entries 3..11, or a BIAS row whose entries 6..11, are not +0.0
    for at in (3, 8):
        for bad in (1.0, -0.0, 1e-300):
            assert call(X=rows(KINDS, velocity_tail=bad, at=at), vp={}) == INVALID, (at, bad)
            assert call(X=rows(KINDS, bias_tail=bad, at=at), vp={}) == INVALID, (at, bad)
    # counts and arrays; a graph with nothing but dampings
    assert call(counts=(-1, 0, 0)) == INVALID and call(counts=(0, -1, 0)) == INVALID and call(counts=(0, 0, -1)) == INVALID
    assert call(counts=(1, 0, 0), null_arrays=True) == INVALID and call(counts=(0, 0, 1), null_arrays=True) == INVALID
    assert call(counts=(0, 0, 0), D=1) == INVALID and call(counts=(0, 0, 0)) == INVALID and call(nav_null=True, D=1) == INVALID
    assert call(vp={}, result=False) == INVALID
    # more new terms than the cap, answered before a term is read
    for which in range(3):
        counts = [0, 0, 0]
        counts[which] = _lib.GRAPH_MAX_TERMS + 1
        assert call(counts=tuple(counts)) == UNSUPPORTED, which
    # a damping may name any node, a pose-only graph is still refused what graph_align_terms refuses, and no node is OK
    assert call(vp={}, D=1, damp_node=6) == INVALID
    assert call(kinds=[], X=np.zeros((0, 12)), counts=(0, 0, 0)) == 0
    tr = _lib.lib().glim_amd_debug_graph_align_nav_trace
    X, Xo = rows(KINDS), np.zeros((6, 12))
    nav = _lib.NavTerms(idx(*KINDS), None, None, None, 1, 0, 0, 0)
    base = (ctx, null2, null2, idx(0), idx(3), 0, 0, None, 0, None, 0, dp(X), 6, None, dp(Xo), None, C.byref(out), None, None, C.byref(nav), 0, None, None, None, None)
    assert tr(*base, 0) == INVALID and tr(*base, -1) == INVALID


# ---- the header on the host ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def step_exe(tmp_path_factory):
    return build_driver(tmp_path_factory, "nav_graph_step", "-Wno-unknown-pragmas")


@pytest.fixture(scope="module")
def old_exe(tmp_path_factory):
    return build_driver(tmp_path_factory, "graph_terms_step", "-Wno-unknown-pragmas")


def run_cpp(exe, tmp_path, mode, data, name="test_nav_graph_step"):
    fin, fout = str(tmp_path / (mode + ".in")), str(tmp_path / (mode + ".out"))
    np.asarray(data, dtype=np.float64).tofile(fin)
    out = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and name + " OK" in out.stdout, out.stdout + out.stderr
    return np.fromfile(fout)


def cpp_assemble(exe, tmp_path, g, X, recs=()):
    """-> H, b, the eight sums (cost, factor, prior, between, inliers, vector prior, vector between, IMU)"""
    out = run_cpp(exe, tmp_path, "assemble", np.concatenate([nr.graph_doubles(g), np.asarray(X).reshape(-1)] + [lmr.compact_of_record(r) for r in recs]))
    n = 6 * g["N"]
    nt = n * (n + 1) // 2
    assert len(out) == nt + n + 8
    H = np.zeros((n, n))
    H[np.tril_indices(n)] = out[:nt]
    return H + np.tril(H, -1).T, out[nt:nt + n], out[nt + n:]


def cpp_step(exe, tmp_path, p, g, X_init, rounds):
    data = np.concatenate([params_head(p), nr.graph_doubles(g), np.asarray(X_init).reshape(-1), [float(len(rounds))]] +
                          [lmr.compact_of_record(r) for recs in rounds for r in recs])
    N = g["N"]
    rows = run_cpp(exe, tmp_path, "step", data).reshape(len(rounds), 30 * N + 7)
    return [{"X": r[:12 * N].reshape(N, 12), "cand": r[12 * N:24 * N].reshape(N, 12), "delta": r[24 * N:30 * N], "lam": r[30 * N], "solve_ok": bool(r[30 * N + 1]),
             "iterations": int(r[30 * N + 2]), "trials": int(r[30 * N + 3]), "status": int(r[30 * N + 4]), "accepted": bool(r[30 * N + 5]), "cost": r[30 * N + 6]}
            for r in rows]


def reference_cases():
    """200 IMU terms, both modes in turn: random poses, velocities, biases, deltas and H_bias of physical size; every fifth term has theta_c and
    r_rot below 1e-8, every fifth (offset 1) theta_c within 1e-3 of pi, every fifth (offset 2) r_rot within 1e-3 of pi.
    -> [(X_i, v_i, X_j, v_j, b, term)]"""
    rng = np.random.default_rng(2024)
    unit = lambda: (lambda v: v / np.linalg.norm(v))(rng.normal(size=3))
    cases = []
    for k in range(200):
        mode = k % 2
        Xi, Xj = random_pose(rng, 1.0, 5.0), random_pose(rng, 1.0, 5.0)
        vi, vj = rng.normal(0, 3.0, 3), rng.normal(0, 3.0, 3)
        b = np.concatenate([rng.normal(0, 0.1, 3), rng.normal(0, 0.01, 3)])
        t = nr.imu_term(rng, (0, 1, 2, 3, 4), Xi, vi, Xj, vj, b, mode, dt=rng.uniform(0.02, 0.5))
        t["bias_hat"] = b + np.concatenate([rng.normal(0, 0.05, 3), rng.normal(0, 0.005, 3)])
        t["delta"] = np.concatenate([rng.normal(0, 0.3, 3), rng.normal(0, 0.5, 3), rng.normal(0, 1.0, 3)])
        kind = k // 2 % 5
        if kind == 0:
            t["bias_hat"] = b.copy()  # db = 0: theta_c is delta's
            t["delta"][:3] = rng.uniform(1e-10, 1e-8) * unit()
        elif kind == 1:
            t["delta"][:3] = (np.pi - rng.uniform(1e-6, 1e-3)) * unit()
            t["bias_hat"][3:] = b[3:]
        th_c = nr.corrected_delta(t, b)[0]
        if kind in (0, 2):  # R_j = R_i Exp(theta_c) Exp(-e): r_rot = e
            e = rng.uniform(1e-10, 1e-8) * unit() if kind == 0 else (np.pi - rng.uniform(1e-6, 1e-3)) * unit()
            Xj[:3, :3] = Xi[:3, :3] @ nr.so3_exp(th_c) @ nr.so3_exp(e).T
        cases.append((Xi, vi, Xj, vj, b, t))
    return cases


@pytest.fixture(scope="module")
def reference_table(step_exe, tmp_path_factory):
    """the header's r and J and the 200-bit restatement's, computed once for the two tests below"""
    cases = reference_cases()
    data = [[float(len(cases))]]
    for Xi, vi, Xj, vj, b, t in cases:
        data += [Xi[:3].reshape(-1), vi, Xj[:3].reshape(-1), vj, b, [float(t["mode"])], nr.imu_data(t)]
    out = run_cpp(step_exe, tmp_path_factory.mktemp("imu"), "imu", np.concatenate(data)).reshape(len(cases), 9 + 9 * 24)
    ref = [nr.imu_reference(*c) for c in cases]
    return cases, out[:, :9], out[:, 9:].reshape(-1, 9, 24), ref


def test_the_imu_residual_is_the_200_bit_restatements(reference_table):
    """The header's residual against tests/nav_graph_restatement.imu_reference (mpmath, 200 bits, tests/se3_reference.py's maps; no code in
    common with the header).  Error of a term: max |r - r_ref| over max(1, |r_ref|max, |p_i|max, |p_j|max, |v_i|max, |v_j|max) -- the residual is
    a difference of those.  Measured worst over the 200 terms: 3.3e-16 (RESIDUAL_WORST rounds it up); the gate is 8 times that, 2.7e-15.
    tests/golden/se3_range.npz gates Log's rotation at 3.9e-15 (median; up to 5.6e-15) over the same range of angles: the gate here does not exceed it.  A wrong
    formula misses by many orders of magnitude."""
    cases, r, _, ref = reference_table
    worst, small, near_pi = 0.0, 0, 0
    for (Xi, vi, Xj, vj, b, t), got, (want, _) in zip(cases, r, ref):
        scale = max(1.0, np.abs(want).max(), np.abs(Xi[:3, 3]).max(), np.abs(Xj[:3, 3]).max(), np.abs(vi).max(), np.abs(vj).max())
        worst = max(worst, np.abs(got - want).max() / scale)
        small += np.linalg.norm(want[:3]) < 1e-8 and np.linalg.norm(nr.corrected_delta(t, b)[0]) < 1e-8
        near_pi += np.pi - np.linalg.norm(want[:3]) < 1e-3 or np.pi - np.linalg.norm(nr.corrected_delta(t, b)[0]) < 1e-3
    print("worst relative residual error", worst, "terms below 1e-8", small, "terms within 1e-3 of pi", near_pi)
    assert small >= 30 and near_pi >= 60
    assert worst <= 8 * RESIDUAL_WORST


def test_the_imu_jacobian_is_the_200_bit_restatements_derivative(reference_table):
    """The header's J against the central difference of the 200-bit residual (h = 1e-30) through the retractions X Exp(delta), v + delta,
    b + delta.  Error of a term: max |J - J_ref| over max(1, |J_ref|max).  Measured worst over the 200 terms: 3.6e-16 (JACOBIAN_WORST); the gate is
    8 times that, 2.9e-15, which does not exceed what tests/golden/se3_range.npz allows the rotation block of J_r^-1 (up to 3.9e-15).  A wrong
    sign or a missing J_r is an error of order 1."""
    cases, _, J, ref = reference_table
    worst = 0.0
    for got, (_, want) in zip(J, ref):
        worst = max(worst, np.abs(got - want).max() / max(1.0, np.abs(want).max()))
    print("worst relative Jacobian error", worst)
    assert worst <= 8 * JACOBIAN_WORST


def test_the_assembled_cost_has_the_gradient_two_b(step_exe, tmp_path):
    """A central difference of the total cost along every tangent direction (through each node's retraction, h = 1e-5) against 2 b, on the
    K = 4 sub-map graph at the perturbed values.  As test_the_robust_cost_has_the_gradient_two_b derives: the difference's truncation error is
    h^2 / 6 times a third derivative, of the size of |b| for residuals whose second derivatives are O(1) of the first: 2e-11 |b|; its rounding
    error is EPS cost / h = 2.2e-11 cost, with cost < 20 |b|max (asserted).  The gate is 1e-6 |b|max: a block with a wrong sign or a missing
    factor moves an entry by more than 0.1 |b|.  A VELOCITY's rows 3..5 have b = +0.0 and no direction."""
    sc = nr.submap_scene(4, PERT_A)
    g, X = sc["g"], sc["X0"]
    H, b, c = cpp_assemble(step_exe, tmp_path, g, X)
    h, n = 1e-5, 6 * g["N"]
    grad = np.zeros(n)
    for u in nr.active_rows(g):
        e = np.zeros(6)
        e[u % 6] = h
        cost = []
        for sign in (1.0, -1.0):
            Y = X.copy()
            Y[u // 6] = nr.retract(g["kinds"][u // 6], X[u // 6], sign * e)
            cost.append(cpp_assemble(step_exe, tmp_path, g, Y)[2][0])
        grad[u] = (cost[0] - cost[1]) / (2 * h)
    print("cost", c[0], "parts", c[1:], "|b|max", np.abs(b).max(), "worst", np.abs(grad - 2 * b).max())
    assert c[0] < 20 * np.abs(b).max() and c[5] > 0 and c[6] > 0 and c[7] > 0
    assert np.abs(grad - 2 * b).max() <= 1e-6 * np.abs(b).max()
    idle = np.setdiff1d(np.arange(n), nr.active_rows(g))
    assert len(idle) == 12 and not b[idle].any() and not np.signbit(b[idle]).any() and not H[idle].any() and not np.signbit(H[idle]).any()


SCENES = {"sub-map 4": lambda mode: nr.submap_scene(4, PERT_A, mode), "sub-map 20": lambda mode: nr.submap_scene(20, PERT_A, mode),
          "global 5": lambda mode: nr.global_scene(5, PERT_A, mode)}


@pytest.mark.parametrize("scene,mode", [("sub-map 4", nr.TANGENT), ("sub-map 4", nr.MANIFOLD), ("sub-map 20", nr.TANGENT), ("global 5", nr.TANGENT),
                                        ("global 5", nr.MANIFOLD)])
def test_the_header_follows_the_restatement_on_both_graph_shapes(step_exe, tmp_path, scene, mode):
    """Round by round, with the tolerances tests/test_bundle_align.py has for the same comparison (check_against_restatement; the step's gate is
    that of the active rows).  Asserted on the restatement's own run: cond(H) <= 1e9 on the active rows of every kept system, the cost at the
    truth is zero to rounding, the final nodes are within POSE_TOL of the truth (velocities in m/s and biases in their units by the same
    number).  Then the header's final nodes are too.
    The loops run with absolute_error_tol = 1.0 (nr.LOOP): with the default 1e-5 each takes one more step, of 1e-9, from a right-hand side that is
    the rounding of residuals cancelling to zero (its relative error is 1e-6, not eps), and the self-scaled gate of the comparison, which
    assumes two right-hand sides that agree to rounding, does not apply to such a step: measured there 1.8e-15 against a gate of 5.3e-16 on
    the global shape.  Stopped one step earlier the nodes are within 1e-6 of the truth."""
    sc = SCENES[scene](mode)
    g, p = sc["g"], nr.params(**nr.LOOP)
    s, trace = nr.run(lambda Tf: [], g, sc["X0"], p)
    conds = [nr.active_cond(g, e["state"]["sys"]["H"]) for e in trace]
    print(scene, "status", s["status"], "accepted", s["iterations"], "trials", s["trials"], "cost", s["sys"]["cost"], "cond", max(conds), "initial error",
          nr.node_error(sc["kinds"], sc["X0"], sc["truth"]), "final error", nr.node_error(sc["kinds"], s["X"], sc["truth"]))
    assert max(conds) <= COND_MAX and nr.assemble(g, sc["truth"], [])["cost"] < 1e-20
    assert s["status"] == nr.CONVERGED and s["iterations"] >= 2 and nr.node_error(sc["kinds"], sc["X0"], sc["truth"]) > 0.05
    assert nr.node_error(sc["kinds"], s["X"], sc["truth"]) <= POSE_TOL
    rows = cpp_step(step_exe, tmp_path, p, g, sc["X0"], [[] for _ in trace])
    check_against_restatement(rows, [e["state"] for e in trace], kept=("X",), cost_floor=1e-12)
    assert nr.node_error(sc["kinds"], rows[-1]["X"], sc["truth"]) <= POSE_TOL
    tails = np.array([k != nr.POSE for k in sc["kinds"]])[:, None] & (np.arange(12)[None, :] >= np.array([nr.dim(k) for k in sc["kinds"]])[:, None])
    for r in rows:  # what a vector kind does not use stays +0.0
        assert not r["X"][tails].any() and not np.signbit(r["X"][tails]).any() and not r["cand"][tails].any() and not np.signbit(r["cand"][tails]).any()


def test_without_a_new_term_the_bytes_are_those_of_the_driver_from_before(step_exe, old_exe, tmp_path):
    """Every node a POSE and no new term: the same graph, poses and records through tests/cpp/test_graph_terms_step.cpp, the driver of the rule
    as it was before the node kinds (`assemble` and `step`), with dampings and widths and without."""
    rng = np.random.default_rng(21)
    gb = random_graph(rng, 5, 1, 3)
    X = np.stack([pose12(random_pose(rng, 0.4, 3.0)) for _ in range(5)])
    recs = [random_record(rng) for _ in gb["factors"]]
    p = nr.params(max_iterations=2)
    rounds = [[random_record(rng, error=e) for _ in gb["factors"]] for e in (100.0, 50.0, 60.0, 25.0)]
    for name, (betweens, dampings) in {"plain": (gb["betweens"], []), "terms": ([b + (2.0,) for b in gb["betweens"]], [(1, 10.0), (4, [1, 2, 3, 4, 5, 6])])}.items():
        g = nr.graph(5, [nr.POSE] * 5, gb["factors"], gb["priors"], betweens, dampings)
        body = [X.reshape(-1)] + [lmr.compact_of_record(r) for r in recs]
        want = run_cpp(old_exe, tmp_path, "assemble", np.concatenate([gtr.graph_doubles(g)] + body), "test_graph_terms_step")
        got = run_cpp(step_exe, tmp_path, "assemble", np.concatenate([nr.graph_doubles(g)] + body))
        assert got[:len(want)].tobytes() == want.tobytes() and not got[len(want):].any() and want.any(), name
        body = [X.reshape(-1), [float(len(rounds))]] + [lmr.compact_of_record(r) for rs in rounds for r in rs]
        want = run_cpp(old_exe, tmp_path, "step", np.concatenate([params_head(p), gtr.graph_doubles(g)] + body), "test_graph_terms_step")
        got = run_cpp(step_exe, tmp_path, "step", np.concatenate([params_head(p), nr.graph_doubles(g)] + body))
        assert len(want) == len(rounds) * (30 * 5 + 7) and want.any() and got.tobytes() == want.tobytes(), name


def test_a_velocity_nodes_unused_rows_change_nothing_but_their_own_diagonal(step_exe, tmp_path):
    """The K = 4 sub-map graph: rows and columns 3..5 of every VELOCITY block of the assembled system are +0.0 everywhere, the right-hand side
    there is +0.0, and through the loop (where the solve puts lambda on those diagonals) the step there is zero in every round."""
    sc = nr.submap_scene(4, PERT_A)
    g = sc["g"]
    H, b, _ = cpp_assemble(step_exe, tmp_path, g, sc["X0"])
    idle = np.array([6 * k + m for k, kind in enumerate(g["kinds"]) if kind == nr.VELOCITY for m in (3, 4, 5)])
    assert not H[idle].any() and not H[:, idle].any() and not b[idle].any() and not np.signbit(H[idle]).any() and not np.signbit(b[idle]).any()
    S = nr.assemble(g, sc["X0"], [])
    a = nr.active_rows(g)
    assert np.abs(H - S["H"]).max() <= 1e-12 * np.abs(S["H"]).max() and np.abs(b - S["b"]).max() <= 1e-12 * np.abs(S["b"]).max()
    rows = cpp_step(step_exe, tmp_path, nr.params(), g, sc["X0"], [[]] * 4)
    assert rows[-1]["iterations"] >= 3 and all(not r["delta"][idle].any() and not np.signbit(r["delta"][idle]).any() for r in rows)
    assert all(np.abs(r["delta"][a]).max() > 0 for r in rows[:2])


def test_the_header_with_the_new_terms_is_clean_under_the_sanitizers(tmp_path):
    """the stand-alone program once more with AddressSanitizer and UndefinedBehaviorSanitizer: the loop over both graph shapes and modes, the
    assembly, the IMU window, and a graph of poses alone (no term array is read)"""
    exe = str(tmp_path / "test_nav_graph_step_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-Wno-unknown-pragmas", CPP, "-o", exe])
    for sc in (nr.submap_scene(4, PERT_A, nr.MANIFOLD), nr.global_scene(5, PERT_A)):
        rows = cpp_step(exe, tmp_path, nr.params(max_iterations=3), sc["g"], sc["X0"], [[]] * 4)
        assert rows[-1]["iterations"] == 3
        cpp_assemble(exe, tmp_path, sc["g"], sc["X0"])
    rng = np.random.default_rng(2)
    gb = random_graph(rng, 5, 1, 3)
    g = nr.graph(5, [nr.POSE] * 5, gb["factors"], gb["priors"], gb["betweens"], [(1, 10.0)])
    cpp_assemble(exe, tmp_path, g, np.stack([pose12(random_pose(rng, 0.4, 3.0)) for _ in range(5)]), [random_record(rng) for _ in g["factors"]])
    Xi, vi, Xj, vj, b, t = reference_cases()[3]
    data = np.concatenate([[1.0], Xi[:3].reshape(-1), vi, Xj[:3].reshape(-1), vj, b, [float(t["mode"])], nr.imu_data(t)])
    assert len(run_cpp(exe, tmp_path, "imu", data)) == 9 + 9 * 24


# ---- the C++ mirror ------------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_records_the_nodes_and_terms_and_answers_an_empty_problem(tmp_path):
    """include/glim_amd/graph_align.hpp: NavGraph's nodes and terms, ImuTerm, optimize_nav_graph; compiled, linked, and run on an empty problem
    (no device call)"""
    exe = build_cpp(tmp_path, "nav_graph_mirror")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "test_nav_graph_mirror OK" in out.stdout, out.stdout + out.stderr
