"""CPU-side checks of the plane / edge bundle-adjustment factors: the NumPy restatement against central differences and against its own
literal point-pair sum, the host-only algebra of glim_amd/csrc/plane_ba.hpp + eig3_direct.hpp run from a stand-alone program (plain and
under the address / undefined-behaviour sanitizers), the argument checks of the C ABI that need no device, and the C++ layers compiling."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import plane_ba_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _small_problem(seed=1, sizes=(40, 38, 40)):
    """3 frames / 118 points of a slab, world positions around (5, -3, 2), poses with translations of order 20 m"""
    from glim_amd.se3 import se3_exp

    rng = np.random.default_rng(seed)
    poses = [se3_exp(np.concatenate([rng.normal(size=3) * 0.4, rng.normal(size=3) * 20.0])) for _ in sizes]
    frames = []
    for n, T in zip(sizes, poses):
        w = rng.uniform(-1.0, 1.0, size=(n, 3))
        w[:, 2] = 0.3 * w[:, 0] + 0.02 * w[:, 2]  # a tilted slab
        w[:, 1] *= 0.6
        w += np.array([5.0, -3.0, 2.0])
        frames.append((w - T[:3, 3]) @ T[:3, :3])
    return frames, poses


def _moved(poses, seed):
    from glim_amd.se3 import se3_exp

    rng = np.random.default_rng(seed)
    return [T @ se3_exp(0.05 * rng.normal(size=6) / np.sqrt(6)) for T in poses]


@pytest.mark.parametrize("kind", [0, 1])
def test_restatement_gradient_matches_central_differences(kind):
    frames, poses = _small_problem()
    for ps in (poses, _moved(poses, 2)):
        f = R.factor(frames, ps, kind)
        num = R.numeric_gradient(frames, ps, kind, h=1e-6)
        rel = np.abs(f["g"] - num).max() / np.abs(f["g"]).max()
        print("gradient vs central differences:", rel)
        assert rel < 1e-7  # about 1e-8 expected at h = 1e-6: truncation h^2 and rounding u / h both sit there


def test_restatement_is_the_literal_pair_sum_and_symmetric():
    frames, poses = _small_problem(sizes=(7, 1, 9))
    poses = _moved(poses, 4)
    for e in (0, 1):
        a = R._single(frames, poses, e, R.eigh_pairs)
        b = R.factor_pairs(frames, poses, e)
        assert a[4][0] > 0 and a[4][1] >= np.abs(a[2]).max()
        assert np.abs(a[2] - b["H"]).max() <= 1e-12 * np.abs(b["H"]).max()
        assert np.abs(a[1] - b["g"]).max() <= 1e-13 * np.abs(b["g"]).max()
    H = R.factor(frames, poses, 0)["H"]
    assert np.abs(H - H.T).max() <= 1e-13 * np.abs(H).max()


def test_edge_is_the_sum_of_the_two_single_eigenvalue_forms():
    frames, poses = _small_problem()
    edge = R.factor(frames, poses, 1)
    c0, g0, H0, _, _ = R._single(frames, poses, 0, R.eigh_pairs)
    c1, g1, H1, _, _ = R._single(frames, poses, 1, R.eigh_pairs)
    assert edge["cost"] == c0 + c1 and np.array_equal(edge["g"], g0 + g1) and np.array_equal(edge["H"], H0 + H1)


def test_auto_radius_rule_stops():
    """the rule alone, on a synthetic table: shrink while lambda_0 / lambda_2 > eps, grow otherwise, and the three stops"""
    planar, thick = np.array([1e-4, 1.0, 1.0]), np.array([0.5, 1.0, 1.0])
    r, stop, tr = R.auto_radius(lambda r: (100, thick), 1.0, 0.3, 5.0, 0.01)
    assert stop == "range" and r == 1.0 * 0.8 * 0.8 * 0.8 * 0.8 * 0.8 and tr[-1][1] == -1
    r, stop, tr = R.auto_radius(lambda r: (100 if r > 0.6 else 9, thick), 1.0, 0.1, 5.0, 0.01)
    assert stop == "few_points" and r == 1.0 * 0.8 * 0.8
    r, stop, tr = R.auto_radius(lambda r: (100, planar if r < 1.2 else thick), 1.0, 0.1, 5.0, 0.01)
    assert stop == "plane_eps" and r == 1.0 * 1.1
    r, stop, tr = R.auto_radius(lambda r: (100, planar), 1.0, 0.1, 5.0, 0.01)
    assert stop == "trials" and len(tr) == 11


# ---- the host-only algebra of the new headers, from a stand-alone program ------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("plane_ba_host")
    src = os.path.join(ROOT, "tests", "cpp", "test_plane_ba_host.cpp")
    out = {}
    for name, flags in (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", *flags, src, "-o", exe])
        out[name] = exe
    return out


def _run_host(exe, tmp_path, frames, poses, kind):
    K = len(frames)
    inp, outp = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    with open(inp, "w") as f:
        f.write(f"{kind} {K} {sum(len(p) for p in frames)}\n")
        for s, p in enumerate(frames):
            for x in p:
                f.write(f"{s} {float(x[0])!r} {float(x[1])!r} {float(x[2])!r}\n")
        for T in poses:
            f.write(" ".join(repr(float(v)) for v in np.asarray(T)[:3, :4].reshape(12)) + "\n")
    res = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    v = np.array([float(x) for x in open(outp).read().split()])
    n = 6 * K
    if int(v[0]) == 0xFFFFFFFF:  # refused: fewer than three points
        return {"status": int(v[0])}
    return {"status": int(v[0]), "cost": v[1], "g": v[2 : 2 + n], "H": v[2 + n : 2 + n + n * n].reshape(n, n), "lam": v[2 + n + n * n : 5 + n + n * n],
            "U": v[5 + n + n * n :].reshape(3, 3)}


@pytest.mark.parametrize("build", ["plain", "sanitized"])
@pytest.mark.parametrize("kind", [0, 1])
def test_moment_form_on_the_host_equals_the_point_form(host_programs, tmp_path, build, kind):
    frames, poses = _small_problem(sizes=(40, 1, 77))
    for ps in (poses, _moved(poses, 6)):
        got = _run_host(host_programs[build], tmp_path, frames, ps, kind)
        ref = R.factor(frames, ps, kind)
        dg = np.abs(got["g"] - ref["g"]).max() / np.abs(ref["g"]).max()
        dH = np.abs(got["H"] - ref["H"]).max() / np.abs(ref["H"]).max()
        print(f"{build} kind {kind}: g {dg:.2e} H {dH:.2e} cost {got['cost'] - ref['cost']:.2e}")
        # the issue's CPU figures for the moment form against the point-pair form are 2e-15 (H) and 7e-13 (g); the closed-form solver in
        # place of eigh adds its own last places
        assert dg < 1e-10 and dH < 1e-10 and abs(got["cost"] - ref["cost"]) < 1e-13
        assert got["status"] == 0
        assert np.array_equal(got["H"], got["H"].T)
        # the second matrix through the solver: eigenpairs of the first block of 2 H
        M = 2 * got["H"][:3, :3]
        assert np.abs(M @ got["U"].T - got["U"].T * got["lam"]).max() <= 1e-12 * np.abs(M).max()
        assert np.abs(got["lam"] - np.linalg.eigvalsh(M)).max() <= 1e-12 * np.abs(M).max()


def test_host_algebra_flags_a_gapless_pair_and_refuses_two_points(host_programs, tmp_path):
    line = np.zeros((20, 3))
    line[:, 0] = np.arange(20) / 8.0
    got = _run_host(host_programs["sanitized"], tmp_path, [line], [np.eye(4)], 0)
    assert got["status"] == 1 and np.isfinite(got["H"]).all()  # GLIM_AMD_BA_DEGENERATE: the (0, 1) term is dropped
    two = _run_host(host_programs["sanitized"], tmp_path, [line[:2]], [np.eye(4)], 0)
    assert two["status"] == 0xFFFFFFFF


# ---- the C ABI's argument checks that need no device ---------------------------------------------------------------------------------------
def test_abi_argument_checks_without_a_device():
    from glim_amd import _lib

    L = _lib.lib()
    INVALID = -1
    h = C.c_void_p()
    n = C.c_int64()
    pts = np.zeros((4, 3))
    fi = np.zeros(4, dtype=np.int32)
    T = np.eye(4)[:3].reshape(12).copy()
    c = np.zeros(3)
    dp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)))
    one_null = (C.c_void_p * 1)(None)
    assert L.glim_amd_ba_default_params(None) == INVALID
    prm = _lib.BaParams()
    assert L.glim_amd_ba_default_params(C.byref(prm)) == 0 and (prm.min_radius, prm.max_radius, prm.plane_eps) == (0.1, 5.0, 0.01)
    # null handles
    assert L.glim_amd_ba_ball_select(None, 1, dp(T), dp(c), 1.0, 0, None, C.byref(n)) == INVALID
    assert L.glim_amd_ba_ball_select(one_null, 1, dp(T), dp(c), 1.0, 0, None, C.byref(n)) == INVALID
    st = _lib.BaStats()
    assert L.glim_amd_ba_ball_stats(one_null, 1, dp(T), dp(c), 1.0, C.byref(st)) == INVALID
    rr = _lib.BaRadiusResult()
    assert L.glim_amd_ba_auto_radius(one_null, 1, dp(T), dp(c), 1.0, None, C.byref(rr)) == INVALID
    assert L.glim_amd_ba_factor_create_from_ball(one_null, 1, dp(T), dp(c), 1.0, 0, C.byref(h)) == INVALID
    assert L.glim_amd_ba_factor_create(None, 0, 4, dp(pts), ip(fi), 1, C.byref(h)) == INVALID
    assert L.glim_amd_ba_factor_info(None, None, None, None, None, None) == INVALID
    cost = C.c_double()
    assert L.glim_amd_ba_factor_error(None, dp(T), C.byref(cost), None) == INVALID
    assert L.glim_amd_ba_factor_linearize(None, dp(T), C.byref(cost), dp(np.zeros(6)), dp(np.zeros(36)), None) == INVALID
    assert L.glim_amd_ba_factor_destroy(None) == 0
    # r <= 0, capacity < 0 (refused before any handle is looked at)
    assert L.glim_amd_ba_ball_select(one_null, 1, dp(T), dp(c), 0.0, 0, None, C.byref(n)) == INVALID
    assert L.glim_amd_ba_ball_select(one_null, 1, dp(T), dp(c), -1.0, 0, None, C.byref(n)) == INVALID
    assert L.glim_amd_ba_ball_select(one_null, 1, dp(T), dp(c), float("nan"), 0, None, C.byref(n)) == INVALID
    assert L.glim_amd_ba_ball_select(one_null, 1, dp(T), dp(c), 1.0, -1, None, C.byref(n)) == INVALID
    # K > 128, N < 3, a kind that does not exist: refused before the context is looked at
    ctx_stand_in = C.c_void_p(1)  # never dereferenced: the refusal comes first
    assert L.glim_amd_ba_factor_create(ctx_stand_in, 0, 4, dp(pts), ip(fi), 129, C.byref(h)) == INVALID
    assert L.glim_amd_ba_factor_create(ctx_stand_in, 0, 2, dp(pts), ip(fi), 1, C.byref(h)) == INVALID
    assert L.glim_amd_ba_factor_create(ctx_stand_in, 2, 4, dp(pts), ip(fi), 1, C.byref(h)) == INVALID
    assert L.glim_amd_ba_factor_create(ctx_stand_in, 0, 4, dp(pts), ip(fi), 0, C.byref(h)) == INVALID
    assert not h.value


# ---- the C++ layers ------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_compiles_links_and_throws_on_a_refused_call(tmp_path):
    from glim_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exe = str(tmp_path / "test_plane_ba_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_plane_ba_mirror.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "glim_amd"), "-lglim_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "glim_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "plane_ba mirror: ok" in out.stdout


def test_drop_in_header_compiles_against_the_stand_ins_and_the_lsq_factor_says_it_is_not_built(tmp_path):
    from glim_amd import _lib, api

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exe = R.build_drop_in(tmp_path)
    if api.device_count() > 0:
        return  # tests/test_plane_ba_gpu.py runs it
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "no device" in out.stdout
