"""CPU side of the GNC global registration: the pose step of the solve kernel (glim_amd/csrc/gnc_pose.hpp) run on the CPU by a stand-alone
program -- plain, and under -fsanitize=address,undefined -- against the NumPy restatement (tests/gnc_restatement.py) at the step gates that
module derives; the selection and tuple rules on hand-made lists; the new C-ABI entries on NULL handles; the drop-in header and the C++ mirror
compiled with -Wall -Werror.

Measured worst ratio to the gate over the 400 random weighted lists below (both builds, x86-64): rotation 5.6e-3, translation 1.0e-2 (dof 6);
rotation 5.9e-4, translation 1.9e-3 (dof 4)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gnc_restatement as G
import ransac_restatement as R
from registration_cases import build_drop_in_cpp, build_pose_program
from registration_cases import rot as _rot


@pytest.fixture(scope="module")
def pose_programs(tmp_path_factory):
    return build_pose_program(tmp_path_factory, "gnc_pose")


def _run(programs, cases):
    """cases: list of (dof, W, a, b, M, c_s, c_t) -> per program a list of (ok, T 3x4)"""
    d, exes = programs
    path = d / "cases.txt"
    with open(path, "w") as f:
        for dof, W, a, b, M, cs, ct in cases:
            vals = [W] + list(np.ravel(a)) + list(np.ravel(b)) + list(np.ravel(M)) + list(np.ravel(cs)) + list(np.ravel(ct))
            f.write(" ".join([str(dof)] + [float(v).hex() for v in vals]) + "\n")
    results = []
    for exe in exes:
        out = d / (os.path.basename(exe) + ".out")
        res = subprocess.run([exe, str(path), str(out)], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0 and f"({len(cases)} cases)" in res.stdout, res.stdout + res.stderr
        rows = []
        for line in open(out):
            w = line.split()
            rows.append((int(w[0]), np.array([float.fromhex(x) for x in w[1:]]).reshape(3, 4)))
        assert len(rows) == len(cases)
        results.append(rows)
    return results


def _random_lists(rng, dof, count):
    """lists of 20 .. 400 pairs, 1 .. 30 m across, 0 .. 100 m from the origin, moved rigidly (dof 4: about z), a share of outliers, evaluated
    from a pose a few degrees off at a mu between the scale and the noise: what one iteration of the loop sees"""
    out = []
    for _ in range(count):
        n = int(rng.integers(20, 400))
        scale = 10.0 ** rng.uniform(0, 1.5)
        P = (rng.normal(size=(n, 3)) * scale + rng.normal(size=3) * 10.0 ** rng.uniform(0, 2)).astype(np.float32).astype(np.float64)
        Rm = _rot([0, 0, 1], rng.uniform(-np.pi, np.pi)) if dof == 4 else _rot(rng.normal(size=3), rng.uniform(0, np.pi))
        t = rng.normal(size=3) * 20.0
        Q = P @ Rm.T + t + rng.normal(size=(n, 3)) * 0.01
        bad = rng.random(n) < rng.uniform(0, 0.4)
        Q[bad] = rng.normal(size=(int(bad.sum()), 3)) * scale + t
        Q = Q.astype(np.float32).astype(np.float64)
        T_in = np.eye(4)
        T_in[:3, :3] = Rm @ (_rot([0, 0, 1], rng.normal() * 0.05) if dof == 4 else _rot(rng.normal(size=3), rng.normal() * 0.05))
        T_in[:3, 3] = t + rng.normal(size=3) * 0.1
        out.append((P, Q, T_in, scale * scale * 10.0 ** rng.uniform(-3, 1)))
    return out


@pytest.mark.parametrize("dof", [6, 4])
def test_pose_step_on_the_cpu_matches_the_restatement_within_the_gates(pose_programs, dof):
    lists = _random_lists(np.random.default_rng(60 + dof), dof, 200)
    steps = [G.step(P, Q, T_in, mu, dof) for P, Q, T_in, mu in lists]
    cases = [(dof, s["moments"]["W"], s["moments"]["a"], s["moments"]["b"], s["moments"]["M"], s["moments"]["c_s"], s["moments"]["c_t"]) for s in steps]
    compared = 0
    for rows in _run(pose_programs, cases):
        worst_r = worst_t = 0.0
        for (P, _, _, _), s, (ok, T) in zip(lists, steps, rows):
            assert ok == 1
            if s["S"] / s["gap"] > 100.0:
                continue
            compared += 1
            g_r, g_t, _, _ = G.step_gates(s, len(P))
            worst_r = max(worst_r, R.rotation_angle(s["T"][:3, :3], T[:, :3]) / g_r)
            worst_t = max(worst_t, np.linalg.norm(s["T"][:3, 3] - T[:, 3]) / g_t)
            assert abs(np.linalg.det(T[:, :3]) - 1.0) < 1e-12
            if dof == 4:
                assert T[2, 2] == 1.0 and T[0, 2] == 0.0 and T[2, 0] == 0.0
        print(f"dof {dof}: worst rotation / gate {worst_r:.3e}, worst translation / gate {worst_t:.3e}")
        assert worst_r <= 1.0 and worst_t <= 1.0
    assert compared >= 2 * 150  # the comparison is not vacuous


def test_pose_step_on_exact_and_degenerate_moments(pose_programs):
    # an exact quarter turn about z + an integer shift, unit weights, integer points: both forms return it to the last bits
    P = np.array([[1.0, 2, 0], [4, -1, 2], [-2, 3, 1], [0, 0, 5]])
    Rq = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    Q = P @ Rq.T + np.array([10.0, 20.0, 30.0])
    m = G.step(P, Q, np.eye(4), 1e30, 6)["moments"]  # (mu = 1e30: every weight is 1 to the last bit)
    exact = (m["W"], m["a"], m["b"], m["M"], m["c_s"], m["c_t"])
    line = np.array([[0.0, 0, 0], [1, 1, 1], [2, 2, 2], [5, 5, 5]])
    ml = G.step(line, line + 1.0, np.eye(4), 1e30, 6)["moments"]
    z3, z9 = np.zeros(3), np.zeros((3, 3))
    cases = [(6,) + exact, (4,) + exact,
             (6, ml["W"], ml["a"], ml["b"], ml["M"], ml["c_s"], ml["c_t"]),        # collinear, dof 6: finite, a rotation about the line at most
             (6, 4.0, z3, z3, z9, z3, z3),                                          # H = 0: the identity rotation
             (6, 0.0, z3, z3, z9, z3, z3),                                          # W = 0: refused
             (6, float("nan"), z3, z3, z9, z3, z3), (6, 1.0, z3, z3, np.full((3, 3), np.inf), z3, z3), (6, float("inf"), z3, z3, z9, z3, z3)]
    for rows in _run(pose_programs, cases):
        for ok, T in rows[:2]:
            assert ok == 1 and np.abs(T[:, :3] - Rq).max() < 1e-14 and np.abs(T[:, 3] - [10.0, 20.0, 30.0]).max() < 1e-13
        ok, T = rows[2]
        assert ok == 1 and np.all(np.isfinite(T)) and abs(np.linalg.det(T[:, :3]) - 1.0) < 1e-12
        assert np.abs(line @ T[:, :3].T + T[:, 3] - (line + 1.0)).max() < 1e-12  # the line itself lands where it should
        ok, T = rows[3]
        assert ok == 1 and np.array_equal(T, np.eye(4)[:3])
        assert [r[0] for r in rows[4:]] == [0, 0, 0, 0]


def _cloud(n, seed):
    return np.random.default_rng(seed).uniform(-5, 5, (n, 3)).astype(np.float32)


def test_selection_below_at_and_above_the_source_size():
    n = 50
    src, tgt = _cloud(n, 1), _cloud(70, 2)
    near = np.arange(n, dtype=np.int32)
    near[[3, 10]] = -1
    src[20, 1] = np.nan
    tgt[30, 0] = np.inf     # the partner of source 30
    full = [i for i in range(n) if i not in (3, 10, 20, 30)]
    for m in (n, n + 1, 5000):
        lst = G.select(tgt, src, near, 9, m)
        assert lst[:, 0].tolist() == full and np.array_equal(lst[:, 1], near[lst[:, 0]])
    # below: the SET of the draws, by the scalar generator of the RANSAC restatement
    for m in (1, 7, n - 1):
        want = sorted({R.sample_hash(9, j) % n for j in range(m)} - {3, 10, 20, 30})
        lst = G.select(tgt, src, near, 9, m)
        assert lst[:, 0].tolist() == want and len(want) <= m
    assert len({R.sample_hash(9, j) % n for j in range(n - 1)}) < n - 1  # draws repeat: the set is smaller than the sample count
    assert G.select(tgt, src, np.full(n, -1), 9, 5000).shape == (0, 2)
    assert int(G.hashes(0, [0])[0]) == 0xE220A8397B1DCDAF and int(G.hashes(R.MASK, [5])[0]) == R.sample_hash(R.MASK, 5)


def test_tuple_rule_on_hand_made_lists():
    # an exact copy: every trial of three distinct entries passes; the list is the first max_num_tuples of them, in trial order, duplicates kept
    src = _cloud(12, 3)
    tgt = src.copy()
    lst = np.stack([np.arange(12), np.arange(12)], axis=1).astype(np.int32)
    draws = [[R.sample_hash(6, 3 * j + k) % 12 for k in range(3)] for j in range(1200)]  # seed 5 + 1
    passing = [d for d in draws if len(set(d)) == 3]
    out, kept, passed, _ = G.tuples(lst, tgt, src, 5, 0.9, 10 ** 6)
    assert passed == len(passing) == kept and 0 < passed < 1200 and out[:, 0].tolist() == [i for d in passing for i in d]
    assert len(np.unique(out[:, 0])) < len(out)  # repeated entries stay
    out, kept, passed, _ = G.tuples(lst, tgt, src, 5, 0.9, 7)  # the stop in the middle of the trials
    assert kept == 7 and passed == len(passing) and out[:, 0].tolist() == [i for d in passing[:7] for i in d]
    # entries 0 and 1 share a source point AND a target point: an edge of length 0 on both sides never passes
    src2, tgt2 = src.copy(), tgt.copy()
    src2[1], tgt2[1] = src2[0], tgt2[0]
    out, kept, passed, _ = G.tuples(lst, tgt2, src2, 5, 0.0, 10 ** 6)
    want = [d for d in passing if not {0, 1} <= set(d)]
    assert passed == len(want) < len(passing) and out[:, 0].tolist() == [i for d in want for i in d]
    # a target stretched by 1.2: min / max = 1 / 1.2 = 0.833 on every edge
    big = (src.astype(np.float64) * 1.2).astype(np.float32)
    assert G.tuples(lst, big, src, 5, 0.9, 100)[1] == 0 and G.tuples(lst, big, src, 5, 0.8, 100)[1] == 100
    assert G.tuples(lst[:2], tgt, src, 5, 0.9, 100)[1:3] == (0, 0)


def test_free_running_restatement_recovers_an_exact_motion_and_stops_on_degenerate_input():
    rng = np.random.default_rng(4)
    P = rng.uniform(-5, 5, (300, 3))
    Rm = _rot([1, 2, 3], 0.7)
    Q = P @ Rm.T + [1.0, -2.0, 0.5]
    Q[:60] = rng.uniform(-5, 5, (60, 3))
    out = G.run(P, Q, 6)
    assert out["iterations_run"] == 64 and R.rotation_angle(out["T"][:3, :3], Rm) < 5e-3 and np.linalg.norm(out["T"][:3, 3] - [1.0, -2.0, 0.5]) < 2e-2  # (outlier leakage at the final mu)
    assert out["mu"][0] == G.frame(P, Q)[2] and out["mu"][4] == out["mu"][0] / 1.4 and out["mu"][3] == out["mu"][0]
    assert min(out["mu"]) >= G.mu_min_of(G.frame(P, Q)[2], 0.0)
    same = np.ones((5, 3))
    assert G.run(same, same, 6)["iterations_run"] == 0  # D2 = 0: mu = 0, the weights are 0 / 0
    x = rng.normal(size=(1300, 3))
    assert np.array_equal(G.tree_sum(x[:1]), x[0]) and np.allclose(G.tree_sum(x), x.sum(axis=0), rtol=0, atol=1e-11)


def test_new_entry_points_refuse_null_handles_and_fill_the_defaults():
    from glim_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    prm = _lib.GncParams()
    assert L.glim_amd_gnc_default_params(None) == -1
    assert L.glim_amd_gnc_default_params(C.byref(prm)) == 0
    assert (prm.max_init_samples, prm.tuple_check, prm.tuple_thresh, prm.max_num_tuples, prm.div_factor, prm.max_iterations, prm.max_corr_dist,
            prm.inlier_voxel_resolution, prm.dof, prm.seed) == (5000, 0, 0.9, 1000, 1.4, 64, 0.0, 1.0, 6, 0)
    res, info = _lib.RegistrationResult(), _lib.GncInfo()
    idx = (C.c_int32 * 4)()
    n = C.c_int64()
    buf = (C.c_float * 4)()
    dbl = (C.c_double * 16)()
    assert L.glim_amd_gnc_align(None, None, idx, C.byref(prm), C.byref(res), C.byref(info)) == -1
    assert L.glim_amd_gnc_align_fpfh(None, None, None, None, 0, C.byref(prm), C.byref(res), None) == -1
    assert L.glim_amd_gnc_debug_trace(None, None, idx, C.byref(prm), 2, idx, C.byref(n), dbl, dbl, dbl, C.byref(res), None) == -1
    assert L.glim_amd_gnc_profile(None, None, idx, C.byref(prm), 1, buf, buf, buf, buf, buf) == -1
    assert C.sizeof(_lib.GncParams) == 72 and C.sizeof(_lib.GncInfo) == 48


def build_cpp(tmp_path):
    """tests/cpp/test_gnc.cpp over the drop-in tree and the stand-in GLIM headers"""
    return build_drop_in_cpp(tmp_path, "test_gnc")


def test_drop_in_header_and_mirror_compile_against_the_stand_in_headers(tmp_path):
    exe = build_cpp(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "test_gnc OK" in out.stdout, out.stdout + out.stderr
