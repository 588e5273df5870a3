"""CPU-side checks of the map editor's min-cut segmentation: the NumPy restatement of the round-based solver against scipy's maximum flow (flow
and minimal source side) on the scene and on the tiny graphs of the GPU test, the host-callable weight / capacity functions of
glim_amd/csrc/map_edit.hpp run from a stand-alone program (plain and under the address / undefined-behaviour sanitizers), the C++ mirror
compiling and linking, the declared symbols, and the no-device code of every new entry point."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import min_cut_restatement as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE_SEED = 2  # tests/test_min_cut_gpu.py uses the same scene


def test_the_restated_solver_equals_scipy_on_the_tiny_graphs():
    differ = 0
    for name, (n, edges, cap, src, snk) in M.tiny_graphs().items():
        got = M.solve(n, edges, cap, src, snk)
        flow, flags = M.judge(n, edges, cap, src, snk)
        _, largest = M.judge(n, edges, cap, src, snk, maximal=True)
        print(name, "flow", flow, "minimal side", int(flags.sum()), "maximal side", int(largest.sum()), "rounds", got["rounds"], "looks", got["looks"])
        assert got["status"] == M.OK and got["flow"] == flow, name
        np.testing.assert_array_equal(got["flags"], flags, err_msg=name)
        assert (largest >= flags).all(), name
        differ += name.startswith("8 x 8 grid") and int(largest.sum()) > int(flags.sum())
    assert differ >= 2  # graphs on which returning the maximal source side would be noticed
    # the chain in which everything is saturated: nothing on the minimal side, both nodes on the maximal one
    n, edges, cap, src, snk = M.tiny_graphs()["chain s-5-a-5-b-5-t, all saturated"]
    assert M.judge(n, edges, cap, src, snk)[1].sum() == 0 and M.judge(n, edges, cap, src, snk, maximal=True)[1].sum() == 2
    # the long chain needs more than one chunk, and one round is not enough for it
    n, edges, cap, src, snk = M.long_chain()
    assert M.solve(n, edges, cap, src, snk)["looks"] > 1
    cut = M.solve(n, edges, cap, src, snk, max_rounds=1)
    assert cut["status"] == M.ROUND_LIMIT and cut["rounds"] == 1 and not cut["flags"].any()


def test_the_restated_solver_equals_scipy_on_the_scene():
    clouds, poses, normals = M.make_scene(SCENE_SEED)
    want = M.min_cut(clouds, poses, M.CENTER)
    g = want["graph"]
    flow, flags = M.judge(g["num_candidates"], g["edges"], g["cap"], g["src"], g["snk"])
    print("candidates", g["num_candidates"], "edges", g["num_edges"], "foreground", g["num_foreground"], "background", g["num_background"], "flow", flow,
          "segment", int(flags.sum()), "rounds", want["rounds"], "looks", want["looks"], "margins", g["margins"])
    assert M.graph_margins_hold(g["margins"])
    assert want["status"] == M.OK and want["flow"] == flow > 0
    np.testing.assert_array_equal(want["pairs"], g["candidates"][flags == 1])
    assert g["num_foreground"] < want["count"] < g["num_candidates"]
    # with normals the post and the ground hardly share an edge that carries anything
    c32, p32, n32 = M.make_scene(SCENE_SEED, fp32=True)
    prm = dict(M.PARAMS, use_normals=True)
    wn = M.min_cut(c32, p32, M.CENTER, prm, n32)
    gn = wn["graph"]
    assert M.graph_margins_hold(gn["margins"])
    flow, flags = M.judge(gn["num_candidates"], gn["edges"], gn["cap"], gn["src"], gn["snk"])
    assert wn["flow"] == flow and wn["count"] == flags.sum()
    np.testing.assert_array_equal(gn["edges"], M.graph(c32, p32, M.CENTER)["edges"])
    assert (gn["cap"] <= M.graph(c32, p32, M.CENTER)["cap"]).all() and (gn["cap"] < M.graph(c32, p32, M.CENTER)["cap"]).any()


# ---- the host-callable weight functions of map_edit.hpp, from a stand-alone program ------------------------------------------------------------
@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("min_cut_host")
    src = os.path.join(ROOT, "tests", "cpp", "test_min_cut_host.cpp")
    out = {}
    for name, flags in (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", *flags, src, "-o", exe])
        out[name] = exe
    return out


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_capacities_on_the_host_equal_the_restatement(host_programs, tmp_path, build):
    clouds, poses, normals = M.make_scene(SCENE_SEED, fp32=True)
    prm = dict(M.PARAMS, use_normals=True)
    g = M.graph(clouds, poses, M.CENTER, prm, normals)
    assert M.graph_margins_hold(g["margins"]) and M.graph_margins_hold(M.graph(clouds, poses, M.CENTER)["margins"])
    cand, w, edges = g["candidates"], g["world"], g["edges"][:3000]
    nw = np.concatenate([M.R.rotate(np.asarray(normals[s])[cand[cand[:, 0] == s, 1]], poses[s]) for s in range(3)])
    weights = [10.0, 1e-9, 0.5 / 65536.0, 0.25 / 65536.0, 32767.99999, 32768.0, 1e300, -1.0]
    inp, outp = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    with open(inp, "w") as f:
        f.write(f"{prm['distance_sigma']!r} {prm['angle_sigma']!r} {len(edges)}\n")
        for i, j in edges:
            f.write(" ".join(repr(float(v)) for v in (*w[i], *w[j], *nw[i], *nw[j])) + "\n")
        f.write(f"{len(weights)}\n" + "\n".join(repr(float(v)) for v in weights) + "\n")
    out = subprocess.run([host_programs[build], inp, outp], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = np.array([line.split() for line in open(outp).read().splitlines()], dtype=np.int64)
    plain = M.quantize(M.edge_weight(w[edges[:, 0]], w[edges[:, 1]], prm["distance_sigma"]))
    np.testing.assert_array_equal(rows[: len(edges), 0], plain)
    np.testing.assert_array_equal(rows[: len(edges), 1], g["cap"][: len(edges)])
    assert plain.max() > 30000 and plain.min() < 30000 and (g["cap"][: len(edges)] < plain).any()
    np.testing.assert_array_equal(rows[len(edges):], [[1, 655360], [1, 0], [1, 1], [1, 0], [1, 2**31 - 1], [0, -1], [0, -1], [0, -1]])
    print(build, "capacities", int(plain.min()), "...", int(plain.max()))


# ---- the C++ mirror, the symbols, and the C ABI without a device ---------------------------------------------------------------------------------
def test_cpp_mirror_compiles_links_and_throws_on_a_refused_call(tmp_path):
    from glim_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exe = str(tmp_path / "test_min_cut_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_min_cut_mirror.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "glim_amd"), "-lglim_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "glim_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "min_cut mirror: ok" in out.stdout


def test_symbols_are_declared_and_the_python_api_names_exist():
    from glim_amd import _lib, api

    for name in ("glim_amd_edit_min_cut", "glim_amd_diag_edit_min_cut_graph", "glim_amd_diag_max_flow"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    for name in ("edit_min_cut", "MinCutParams", "diag_edit_min_cut_graph", "diag_max_flow", "EDIT_NO_SEED", "EDIT_ROUND_LIMIT"):
        assert hasattr(api, name)
    assert (api.EDIT_NO_SEED, api.EDIT_ROUND_LIMIT) == (3, 4)
    header = open(os.path.join(ROOT, "include", "glim_amd.h")).read()
    assert "GLIM_AMD_EDIT_NO_SEED = 3" in header and "GLIM_AMD_EDIT_ROUND_LIMIT = 4" in header
    assert f"#define GLIM_AMD_EDIT_CAP_SCALE {api.EDIT_CAP_SCALE} " in header and api.EDIT_CAP_SCALE == M.CAP_SCALE
    assert f"#define GLIM_AMD_EDIT_MIN_CUT_MAX_ROUNDS {api.EDIT_MIN_CUT_MAX_ROUNDS} " in header and api.EDIT_MIN_CUT_MAX_ROUNDS == M.MAX_ROUNDS
    assert api.EDIT_ROUNDS_PER_LOOK == M.ROUNDS_PER_LOOK
    assert "Min-cut segmentation (:774-797) is not built" not in header
    assert C.sizeof(_lib.EditMinCutParams) == 64 and C.sizeof(_lib.EditMinCutResult) == 64
    # the defaults of the Python mirror are the header's
    p = api.MinCutParams()
    assert (p.distance_sigma, p.foreground_mask_radius, p.background_mask_radius, p.foreground_weight, p.background_weight, p.k_neighbors, p.use_normals,
            p.max_rounds) == (0.25, 0.5, 5.0, 10.0, 0.0, 20, False, 0) and p.angle_sigma == np.deg2rad(10.0) == M.DEFAULTS["angle_sigma"]


def test_every_entry_point_returns_the_no_device_code_without_a_device():
    from glim_amd import _lib, api

    if api.device_count() > 0:
        return  # tests/test_min_cut_gpu.py runs them
    L = _lib.lib()
    NO_DEVICE = -3
    T = np.eye(4)[:3].reshape(12).copy()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    win = _lib.EditWindow((C.c_double * 3)(0, 0, 0), 2.0, 5, 0)
    one_null = (C.c_void_p * 1)(None)
    out = _lib.EditMinCutResult()
    assert L.glim_amd_edit_min_cut(one_null, 1, dp(T), C.byref(win), None, 0, None, C.byref(out)) == NO_DEVICE
    assert L.glim_amd_edit_min_cut(None, 0, None, C.byref(win), None, 0, None, C.byref(out)) == NO_DEVICE
    assert L.glim_amd_diag_edit_min_cut_graph(one_null, 1, dp(T), C.byref(win), None, 0, None, None, None, 0, None, None, C.byref(out)) == NO_DEVICE
    flow, r, lk, st = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
    assert L.glim_amd_diag_max_flow(None, 0, 0, None, None, None, None, 0, None, C.byref(flow), C.byref(r), C.byref(lk), C.byref(st)) == NO_DEVICE
