"""CPU-side checks of the map editing entry points: the NumPy restatement against independent statements of the same thing (scipy's shortest
hop counts; a literal dictionary of cells), the host-callable predicates of glim_amd/csrc/map_edit.hpp run from a stand-alone program (plain
and under the address / undefined-behaviour sanitizers), the C++ mirror compiling and linking, and the no-device code of every new entry
point."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_edit_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bfs_levels_equal_scipy_shortest_hop_counts():
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import shortest_path

    clouds, poses, normals = R.make_scene()
    for kw in ({}, {"normals": normals, "cos_angle": float(np.cos(np.deg2rad(10.0)))}):
        res = R.region_grow(clouds, poses, R.CENTER, distance_threshold=0.15, dilation_radius=0.0, **kw)
        w, cand = res["world"], res["candidates"]
        nw = None
        if kw:
            nw = np.concatenate([R.rotate(normals[s][cand[cand[:, 0] == s, 1]], poses[s]) for s in range(4)])
        adj = R.adjacency(w, 0.15, nw, kw.get("cos_angle"))
        np.fill_diagonal(adj, False)
        seed = int(np.nonzero((cand == np.array(res["seed"])).all(axis=1))[0][0])
        hops = shortest_path(csr_matrix(adj.astype(np.int8)), method="D", unweighted=True, indices=seed)
        want = np.where(np.isfinite(hops), hops, -1).astype(np.int32)
        np.testing.assert_array_equal(res["all_levels"], want)
        assert res["rounds"] == want.max() and res["rounds"] >= 3  # several levels, and (below) points the growth does not reach
        assert (want < 0).any()
        print("levels:", np.bincount(want[want >= 0]), "unreached:", int((want < 0).sum()))


def _literal_window(clouds, poses, point, resolution, window):
    """update_cells (:166-186) + collect_neighbor_point_ids (:85-112), literally: a dictionary of cells keyed by the integer coordinate"""
    inv_resolution = 1.0 / resolution
    cells = {}
    for s, (p, T) in enumerate(zip(clouds, poses)):
        for i, x in enumerate(p):
            pt = R.transform(x[None], T)[0]
            coord = tuple(int(np.floor(v * inv_resolution)) for v in pt)
            cells.setdefault(coord, []).append((s, i))
    center = [int(np.floor(v / resolution)) for v in point]
    ids = []
    for i in range(-window, window + 1):
        for j in range(-window, window + 1):
            for k in range(-window, window + 1):
                ids += cells.get((center[0] + i, center[1] + j, center[2] + k), [])
    return np.array(sorted(ids), dtype=np.int32).reshape(-1, 2)


def test_window_predicate_equals_a_literal_dictionary_of_cells():
    clouds, poses, _ = R.make_scene()
    # small cells and a window of one or two of them, so that the window cuts through the slab; a centre with negative cell coordinates too
    for point, res, win in ((R.CENTER, 0.5, 1), (R.CENTER + np.array([0.7, -0.4, 0.1]), 0.3, 2), (np.array([-0.1, -0.1, -0.1]), 16.0, 1)):
        got, _ = R.select(clouds, poses, R.WINDOW, point, 0.0, res, win)
        want = _literal_window(clouds, poses, point, res, win)
        np.testing.assert_array_equal(got, want)
        assert 0 < len(got) < sum(len(c) for c in clouds) or res == 16.0


# ---- the host-callable predicates of map_edit.hpp, from a stand-alone program ------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("map_edit_host")
    src = os.path.join(ROOT, "tests", "cpp", "test_map_edit_host.cpp")
    out = {}
    for name, flags in (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", *flags, src, "-o", exe])
        out[name] = exe
    return out


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_predicates_on_the_host_equal_the_restatement(host_programs, tmp_path, build):
    clouds, poses, normals = R.make_scene()
    p, T, nl = clouds[2][:300], poses[2], normals[2][:300].astype(np.float64)
    res, win, radius, thr, cosang = 0.5, 1, 0.8, 0.15, float(np.cos(np.deg2rad(10.0)))
    for M, center in ((T[:3, :4], R.CENTER), ((np.linalg.inv(R.MODEL) @ T)[:3, :4], R.CENTER)):
        inp, outp = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
        with open(inp, "w") as f:
            f.write(f"{res!r} {win} {radius!r} " + " ".join(repr(float(v)) for v in center) + "\n")
            f.write(" ".join(repr(float(v)) for v in M.reshape(12)) + "\n")
            f.write(f"{thr!r} {cosang!r} {len(p)}\n")
            for x, n in zip(p, nl):
                f.write(" ".join(repr(float(v)) for v in (*x, *n)) + "\n")
        out = subprocess.run([host_programs[build], inp, outp], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        rows = [np.array(line.split(), dtype=np.int64).astype(bool) for line in open(outp).read().splitlines()]
        v = R.transform(p, M)
        counts = []
        for mode in (R.BOX, R.SPHERE, R.WINDOW, R.WINDOW_BALL):
            want = R.predicate(mode, v, center, radius, res, win)
            np.testing.assert_array_equal(rows[mode], want)
            counts.append(int(want.sum()))
        np.testing.assert_array_equal(np.array(rows[4:]), R.adjacency(v, thr, R.rotate(nl, M), cosang))
        print(build, "selected per mode:", counts)


# ---- the C++ mirror, and the C ABI without a device ------------------------------------------------------------------------------------------------
def test_cpp_mirror_compiles_links_and_throws_on_a_refused_call(tmp_path):
    from glim_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exe = str(tmp_path / "test_map_edit_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_map_edit_mirror.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "glim_amd"), "-lglim_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "glim_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "map_edit mirror: ok" in out.stdout


def test_symbols_are_declared_and_the_python_api_names_exist():
    from glim_amd import _lib, api

    for name in ("glim_amd_edit_select", "glim_amd_edit_select_outliers", "glim_amd_edit_region_grow", "glim_amd_edit_remove_points"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    for name in ("edit_select", "edit_select_outliers", "edit_region_grow", "edit_remove_points", "edit_remove_selected", "RegionGrowingParams"):
        assert hasattr(api, name)
    header = open(os.path.join(ROOT, "include", "glim_amd.h")).read()
    assert f"#define GLIM_AMD_EDIT_ROUNDS_PER_LOOK {api.EDIT_ROUNDS_PER_LOOK} " in header
    for k, name in enumerate(("BOX", "SPHERE", "WINDOW", "WINDOW_BALL")):
        assert f"#define GLIM_AMD_EDIT_{name} {k}\n" in header and getattr(api, "EDIT_" + name) == k


def test_every_entry_point_returns_the_no_device_code_without_a_device():
    from glim_amd import _lib, api

    if api.device_count() > 0:
        return  # tests/test_map_edit_gpu.py runs them
    L = _lib.lib()
    NO_DEVICE = -3
    n, st, h = C.c_int64(), C.c_int32(), C.c_void_p()
    T = np.eye(4)[:3].reshape(12).copy()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    win = _lib.EditWindow((C.c_double * 3)(0, 0, 0), 2.0, 5, 0)
    one_null = (C.c_void_p * 1)(None)
    out = _lib.EditRegionResult()
    assert L.glim_amd_edit_select(one_null, 1, dp(T), api.EDIT_WINDOW, C.byref(win), 0.0, 0, None, C.byref(n)) == NO_DEVICE
    assert L.glim_amd_edit_select(None, 0, None, api.EDIT_BOX, None, 0.0, 0, None, C.byref(n)) == NO_DEVICE
    assert L.glim_amd_edit_select_outliers(one_null, 1, dp(T), C.byref(win), 2.0, None, 0, None, C.byref(n), C.byref(st)) == NO_DEVICE
    assert L.glim_amd_edit_region_grow(one_null, 1, dp(T), C.byref(win), None, 0, None, None, C.byref(out)) == NO_DEVICE
    assert L.glim_amd_edit_remove_points(None, 0, None, C.byref(h)) == NO_DEVICE
    assert not h.value
