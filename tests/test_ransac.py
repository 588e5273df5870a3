"""CPU side of the RANSAC global registration: the pose solver of the hypothesis kernel (glim_amd/csrc/ransac_pose.hpp) run on the CPU by a
stand-alone program -- plain, and under -fsanitize=address,undefined -- against the NumPy restatement (tests/ransac_restatement.py) at the gates
that module derives; hand-made cases of the restatement that can be verified by eye; the new C-ABI entries on NULL handles; the drop-in header
and the C++ mirror compiled with -Wall -Werror.

Pose gate: rotation angle <= 64 * 2^-52 * cond^2, translation <= that * |farthest source point| + 64 * 2^-52 * |farthest target point|, on
triangles with cond <= 100.  Measured worst ratio to the gate over the 1 200 random triangles below (both builds, x86-64): rotation 0.051,
translation 0.033 (dof 6); rotation 0.014, translation 0.0087 (dof 4).  The constant 64 stands."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ransac_restatement as R
from registration_cases import build_drop_in_cpp, build_pose_program
from registration_cases import rot as _rot


@pytest.fixture(scope="module")
def pose_programs(tmp_path_factory):
    return build_pose_program(tmp_path_factory, "ransac_pose")


def _run(programs, cases):
    """cases: list of (dof, thresh, s 3x3, t 3x3) -> per program a list of (status, T 3x4)"""
    d, exes = programs
    path = d / "cases.txt"
    with open(path, "w") as f:
        for dof, thresh, s, t in cases:
            f.write(" ".join([str(dof), float(thresh).hex()] + [float(v).hex() for v in np.asarray(s).ravel()] + [float(v).hex() for v in np.asarray(t).ravel()]) + "\n")
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


def _random_cases(rng, dof, n):
    """triangles of 0.3 .. 30 m edges, 0 .. 300 m from the origin, moved rigidly (dof 4: about z) with 0 .. 1 % noise, FP32-rounded like cloud points"""
    cases = []
    for _ in range(n):
        scale = 10.0 ** rng.uniform(-0.5, 1.5)
        s = rng.normal(size=(3, 3)) * scale + rng.normal(size=3) * 10.0 ** rng.uniform(-1, 2.5)
        Rm = _rot([0, 0, 1], rng.uniform(-np.pi, np.pi)) if dof == 4 else _rot(rng.normal(size=3), rng.uniform(0, np.pi))
        t = s @ Rm.T + rng.normal(size=3) * 20.0 + rng.normal(size=(3, 3)) * scale * rng.choice([0.0, 1e-3, 1e-2])
        cases.append((dof, 0.5, s.astype(np.float32).astype(np.float64), t.astype(np.float32).astype(np.float64)))
    return cases


@pytest.mark.parametrize("dof", [6, 4])
def test_pose_solver_on_the_cpu_matches_the_restatement_within_the_gates(pose_programs, dof):
    cases = _random_cases(np.random.default_rng(40 + dof), dof, 600)
    ref = [R.solve(s, t, th, d) for d, th, s, t in cases]
    compared = 0
    for rows in _run(pose_programs, cases):
        worst_r = worst_t = 0.0
        for (d, th, s, t), r, (status, T) in zip(cases, ref, rows):
            if min(r["edge_margin"], r["col_margin"]) > 1e-9:
                assert status == r["status"]
            if status != 0 or r["status"] != 0 or r["cond"] > 100.0:
                continue
            compared += 1
            g_r, g_t = R.pose_gates(r["cond"], np.linalg.norm(s, axis=1).max(), np.linalg.norm(t, axis=1).max())
            worst_r = max(worst_r, R.rotation_angle(r["T"][:3, :3], T[:, :3]) / g_r)
            worst_t = max(worst_t, np.linalg.norm(r["T"][:3, 3] - T[:, 3]) / g_t)
            assert abs(np.linalg.det(T[:, :3]) - 1.0) < 1e-12
        print(f"dof {dof}: worst rotation / gate {worst_r:.3e}, worst translation / gate {worst_t:.3e}")
        assert worst_r <= 1.0 and worst_t <= 1.0
    assert compared >= 2 * 300  # the comparison is not vacuous: most triangles are ok and well conditioned


def test_pose_solver_rejections(pose_programs):
    tri = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    nan = tri.copy()
    nan[1, 2] = np.nan
    inf = tri.copy()
    inf[2, 0] = np.inf
    cases = [
        (6, 0.5, np.array([[0.0, 0, 0], [1, 1, 1], [2, 2, 2]]), np.array([[0.0, 0, 0], [1, 1, 1], [2, 2, 2]])),  # collinear: 4
        (4, 0.5, np.array([[0.0, 0, 0], [1, 0, 0], [3, 0, 0]]), np.array([[5.0, 0, 0], [5, 1, 0], [5, 3, 0]])),  # collinear, rotated: 4
        (6, 0.5, np.array([[1.0, 2, 3]] * 3), np.array([[4.0, 5, 6]] * 3)),                                        # zero size: 4
        (6, 0.5, np.array([[0.0, 0, 0], [1, 0, 0], [1, 0, 0]]), np.array([[0.0, 0, 0], [1, 0, 0], [1, 0, 0]])),  # a repeated point: 4
        (6, 0.5, tri, nan), (6, 0.5, inf, tri),                                                                   # not finite: 4, before the edge rule
        (6, 0.5, tri, 2.1 * tri), (6, 0.5, 2.1 * tri, tri),                                                        # edges differ by more than 1 / 0.5: 3
        (6, 0.5, tri, 1.9 * tri), (4, 0.5, tri, 1.9 * tri),                                                        # ... by less: ok
        (6, 0.0, tri, tri), (6, 0.0, tri, tri * (1 + 1e-9)),                                                       # thresh 0: equal lengths only
    ]
    want = [4, 4, 4, 4, 4, 4, 3, 3, 0, 0, 0, 3]
    for rows in _run(pose_programs, cases):
        assert [st for st, _ in rows] == want
        for (st, T), w in zip(rows, want):
            if w != 0:
                assert np.array_equal(T, np.eye(4)[:3])
    assert [R.solve(s, t, th, d)["status"] for d, th, s, t in cases] == want


def test_pure_yaw_is_solved_identically_by_dof_4_and_dof_6(pose_programs):
    s = np.array([[1.0, 2, 0.5], [4, -1, 1.5], [-2, 3, -0.25]])
    Rz = _rot([0, 0, 1], 0.7)
    t = (s @ Rz.T + np.array([3.0, -2.0, 1.0])).astype(np.float32).astype(np.float64)
    for rows in _run(pose_programs, [(6, 0.5, s, t), (4, 0.5, s, t)]):
        (s6, T6), (s4, T4) = rows
        assert s6 == 0 and s4 == 0
        r = R.solve(s, t, 0.5, 6)
        g_r, g_t = R.pose_gates(r["cond"], np.linalg.norm(s, axis=1).max(), np.linalg.norm(t, axis=1).max())
        # FP32 rounding of the target leaves a residual of ~1e-7 that the two models absorb differently: compare at that level, and each at the gate
        assert R.rotation_angle(T6[:, :3], T4[:, :3]) < 1e-6 and np.linalg.norm(T6[:, 3] - T4[:, 3]) < 1e-5
        assert R.rotation_angle(T4[:, :3], Rz) < 1e-6 and np.allclose(T4[:, 3], [3.0, -2.0, 1.0], atol=1e-5)
        for dof, T in ((6, T6), (4, T4)):
            ref = R.solve(s, t, 0.5, dof)["T"]
            assert R.rotation_angle(ref[:3, :3], T[:, :3]) <= g_r and np.linalg.norm(ref[:3, 3] - T[:, 3]) <= g_t
        assert T4[2, 2] == 1.0 and T4[0, 2] == 0.0 and T4[2, 0] == 0.0
    # exact data (a quarter turn, integer coordinates): both forms give the same matrix to the last bits of the gate
    s = np.array([[1.0, 2, 0], [4, -1, 2], [-2, 3, 1]])
    Rq = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    t = s @ Rq.T + np.array([10.0, 20.0, 30.0])
    for rows in _run(pose_programs, [(6, 0.5, s, t), (4, 0.5, s, t)]):
        for _, T in rows:
            assert np.abs(T[:, :3] - Rq).max() < 1e-14 and np.abs(T[:, 3] - [10.0, 20.0, 30.0]).max() < 1e-13


def _lattice_cloud():
    """60 points at small integers + 1/4: every rigid motion by quarter turns and integers is exact in FP32 and keeps them a quarter of a
    voxel away from the voxel faces (a pose that is right to 1e-15 must not move a point across one)"""
    rng = np.random.default_rng(2)
    p = rng.integers(-8, 9, size=(200, 3))
    p = np.unique(p, axis=0)
    return (p[rng.permutation(len(p))[:60]] + 0.25).astype(np.float32)


def test_an_exact_rigid_copy_is_found_by_the_first_ok_hypothesis():
    src = _lattice_cloud()
    M = np.eye(4)
    M[:3, :3] = [[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]
    M[:3, 3] = [3.0, -5.0, 2.0]
    tgt = (src.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    h = R.hypotheses(tgt, src, np.arange(60), seed=7, thresh=0.5, res=1.0, dof=6, first=0, count=50)
    ok = np.nonzero(h["status"] == 0)[0]
    assert len(ok) > 0 and set(h["status"]) <= {0, 2, 4}  # (a draw can repeat a point or be collinear on a lattice; no edge can fail)
    best, inliers, run = R.sequential_result(h["status"], h["inliers"], 60, 0.9, 50)
    assert best == ok[0] and run == ok[0] + 1 and inliers == 60  # inlier_rate = 1
    assert np.abs(h["T"][best] - M).max() < 1e-12  # T_target_source: source -> target, the inverse of the motion target -> source
    h4 = R.hypotheses(tgt, src, np.arange(60), seed=7, thresh=0.5, res=1.0, dof=4, first=0, count=50)
    assert np.array_equal(h4["status"], h["status"]) and np.abs(h4["T"][best] - M).max() < 1e-12 and h4["inliers"][best] == 60


def test_the_result_rule_on_hand_made_records():
    status = np.array([1, 0, 0, 3, 0, 0])
    inl = np.array([0, 5, 9, 0, 9, 12])
    assert R.sequential_result(status, inl, 10, 2.0, 6) == (5, 12, 6)      # never stops: the largest count
    assert R.sequential_result(status, inl, 10, 2.0, 5) == (2, 9, 5)       # a tie goes to the smaller index
    assert R.sequential_result(status, inl, 10, 0.9, 6) == (2, 9, 3)       # the first to reach 9 of 10 stops the loop
    assert R.sequential_result(status, inl, 10, 0.9, 1) == (-1, 0, 1)      # no ok hypothesis
    assert R.sequential_result(status, inl * 0, 10, 2.0, 6) == (1, 0, 6)   # all-zero counts: the first ok hypothesis
    assert R.sample_hash(0, 0) == 0xE220A8397B1DCDAF  # splitmix64's first output for seed 0


def test_new_entry_points_refuse_null_handles_and_fill_the_defaults():
    from glim_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    prm = _lib.RansacParams()
    assert L.glim_amd_ransac_default_params(None) == -1
    assert L.glim_amd_ransac_default_params(C.byref(prm)) == 0
    assert (prm.max_iterations, prm.early_stop_inlier_rate, prm.poly_error_thresh, prm.inlier_voxel_resolution, prm.dof, prm.seed) == (5000, 0.9, 0.5, 1.0, 6, 0)
    res = _lib.RegistrationResult()
    idx = (C.c_int32 * 4)()
    buf = (C.c_float * 33)()
    pose = (C.c_double * 12)()
    h = C.c_void_p()
    assert L.glim_amd_ransac_align(None, None, idx, C.byref(prm), C.byref(res)) == -1
    assert L.glim_amd_ransac_align_fpfh(None, None, None, None, 0, C.byref(prm), C.byref(res)) == -1
    assert L.glim_amd_ransac_debug_hypotheses(None, None, idx, C.byref(prm), 0, 1, idx, idx, pose, idx, idx, idx) == -1
    assert L.glim_amd_ransac_profile(None, None, idx, C.byref(prm), 1, buf, buf, buf, idx, idx) == -1
    assert L.glim_amd_fpfh_create(None, 1, buf, C.byref(h)) == -1
    assert L.glim_amd_debug_ransac_max_lds_slots(-1) == -1
    assert L.glim_amd_debug_ransac_max_lds_slots(8192) == 0
    assert C.sizeof(_lib.RansacParams) == 48 and C.sizeof(_lib.RegistrationResult) == 120


def build_cpp(tmp_path):
    """tests/cpp/test_ransac.cpp over the drop-in tree and the stand-in GLIM headers"""
    return build_drop_in_cpp(tmp_path, "test_ransac")


def test_drop_in_header_and_mirror_compile_against_the_stand_in_headers(tmp_path):
    exe = build_cpp(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "test_ransac OK" in out.stdout, out.stdout + out.stderr
