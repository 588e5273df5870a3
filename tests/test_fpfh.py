"""CPU side of the FPFH feature: hand-made cases of the NumPy restatement (tests/fpfh_restatement.py) that can be verified by eye, the new C-ABI
entry points on NULL handles, and the drop-in header + C++ mirror compiled against the stand-in GLIM headers with -Wall -Werror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fpfh_restatement as R
from registration_cases import build_drop_in_cpp
S = np.sqrt(0.5)


def _pair(points, normals, i, j):
    p = np.asarray(points, dtype=np.float32)
    d = p[j].astype(np.float64) - p[i].astype(np.float64)
    d2 = np.array([(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]])
    bins, skipped, margin, swap = R.pair_features(p, np.asarray(normals, dtype=np.float32), np.array([i]), np.array([j]), d2)
    return bins[0], bool(skipped[0])


def test_two_points_with_parallel_normals_fall_into_the_middle_bins():
    # dp = x, both normals z: a1 = a2 = 0 (no swap), f3 = 0, v = dp x n = -y, w = n x v = x, f2 = v.n = 0, f1 = atan2(0, 1) = 0: 5.5 -> bin 5 each
    bins, skipped = _pair([[0, 0, 0], [1, 0, 0]], [[0, 0, 1], [0, 0, 1]], 0, 1)
    assert not skipped and list(bins) == [5, 5, 5]


def test_roles_swap_when_the_other_normal_is_more_aligned_with_the_line():
    # n_i = z, n_j = (x + z) / sqrt 2, dp = x: a1 = 0 < a2 = 0.707 -> n1 = n_j, n2 = n_i, dp = -x, f3 = -0.707 -> 11 * 0.146 = 1.6 -> bin 1
    # v = dp x n1 = +y, w = n1 x v = (-s, 0, s), f2 = v.n2 = 0 -> bin 5, f1 = atan2(s, s) = pi / 4 -> 11 * 0.625 = 6.875 -> bin 6
    pts, nrm = [[0, 0, 0], [1, 0, 0]], [[0, 0, 1], [S, 0, S]]
    bins, skipped = _pair(pts, nrm, 0, 1)
    assert not skipped and list(bins) == [6, 5, 1]
    # seen from the other point nothing swaps (|a1| = 0.707 > |a2| = 0) and the same frame comes out
    bins, skipped = _pair(pts, nrm, 1, 0)
    assert not skipped and list(bins) == [6, 5, 1]
    out = R.spfh(np.array(pts, dtype=np.float32), np.array(nrm, dtype=np.float32), 2.0)
    assert list(out["k"]) == [1, 1]
    for i in range(2):
        assert out["S"][i, 6] == 100.0 and out["S"][i, 11 + 5] == 100.0 and out["S"][i, 22 + 1] == 100.0 and out["S"][i].sum() == 300.0


def test_a_duplicate_point_is_no_neighbour():
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0]], dtype=np.float32)
    nrm = np.array([[0, 0, 1]] * 3, dtype=np.float32)
    out = R.spfh(pts, nrm, 2.0)
    assert list(out["k"]) == [1, 2, 1]  # 0 and 2 see only point 1; point 1 sees both
    assert not any((i, j) in ((0, 2), (2, 0)) for i, j in zip(out["i"], out["j"]))


def test_a_pair_along_the_normal_is_skipped_but_counted():
    # dp = z = n1: v = dp x n1 = 0.  Point 2 gives point 0 one real pair: its SPFH is 1 count * 100 / k with k = 2
    pts = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0]], dtype=np.float32)
    nrm = np.array([[0, 0, 1]] * 3, dtype=np.float32)
    _, skipped = _pair(pts, nrm, 0, 1)
    assert skipped
    out = R.spfh(pts, nrm, 1.2)
    assert out["k"][0] == 2 and out["counts"][0].sum() == 3
    assert out["S"][0, 5] == 50.0 and out["S"][0].sum() == 150.0


def test_an_isolated_point_is_all_zero_and_blocks_of_the_others_sum_to_100():
    rng = np.random.default_rng(3)
    pts = rng.uniform(-1, 1, (200, 3)).astype(np.float32)
    pts[7] = (50, 50, 50)
    nrm = rng.normal(size=(200, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    out = R.fpfh(pts, nrm, 0.5)
    assert out["k"][7] == 0 and not out["F"][7].any() and not out["S"][7].any()
    rest = out["k"] > 0
    assert rest.sum() > 150
    for b in range(3):
        np.testing.assert_allclose(out["F"][rest, 11 * b:11 * b + 11].sum(axis=1), 100.0, rtol=0, atol=1e-10)
    assert (out["F"] >= 0).all()


def test_match_restatement_prefers_the_smaller_index_on_a_tie():
    t = np.array([[1.0, 0], [0, 1.0], [1.0, 0]])
    best, d1, d2 = R.match(t, np.array([[1.0, 0], [0.1, 1.0]]))
    assert list(best) == [0, 1] and d1[0] == 0.0 and d2[0] == 0.0
    rec, _, _ = R.match_reciprocal(t, np.array([[1.0, 0], [1.0, 0]]))
    assert list(rec) == [0, -1]  # target 0's nearest source is source 0 (tie to the smaller index)


def test_new_entry_points_refuse_null_handles():
    from glim_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    h = C.c_void_p()
    n = C.c_int64()
    buf = (C.c_float * 33)()
    idx = (C.c_int32 * 1)()
    assert L.glim_amd_fpfh_estimate(None, 1.0, C.byref(h)) == -1
    assert L.glim_amd_fpfh_size(None, C.byref(n)) == -1
    assert L.glim_amd_fpfh_download(None, buf) == -1
    assert L.glim_amd_fpfh_match(None, None, 0, idx, buf) == -1
    assert L.glim_amd_fpfh_destroy(None) == 0


def build_cpp(tmp_path):
    """tests/cpp/test_fpfh.cpp over the drop-in tree and the stand-in GLIM headers"""
    return build_drop_in_cpp(tmp_path, "test_fpfh")


def test_drop_in_header_and_mirror_compile_against_the_stand_in_headers(tmp_path):
    exe = build_cpp(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "test_fpfh OK" in out.stdout, out.stdout + out.stderr
