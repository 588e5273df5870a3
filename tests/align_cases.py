"""What the tests of the fine-registration family share (tests/test_{gicp,ct,vgicp,bundle}_align.py on the CPU, their _gpu twins on the device):
the perturbations and margins of the cases, the device scans and maps built once per module, the comparisons of records and results, the
teacher-forced check of a trace, and the scaffolding of the CPU modules -- the declared-once check, the host drivers of the step headers, the
comparison against a restatement, the C++ mirror programs.  A plain module: it holds no tests."""
import os
import re
import subprocess

import numpy as np
import pytest

import lm_restatement as lmr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD_TOL = 2e-4  # of a device record against the FP64 oracle (tests/test_gicp.py, tests/test_gpu_parity.py)
MOVES = 5e-3       # a trial whose error moves by less than this of itself must not decide a test: 25 x RECORD_TOL
SMALL, BIG = (16, 128), (32, 384)
PERT_A = [0.01, -0.01, 0.01, 0.08, -0.05, 0.03]
PERT_B = [0.02, 0.01, -0.015, 0.15, -0.1, 0.05]
PERT_C = [0.03, -0.02, 0.02, 0.2, 0.15, -0.05]
PERT_D = [0.015, 0.001, 0.026, -0.217, 0.171, -0.217]


# ---- on the device ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    """one context per test module that imports this fixture"""
    from glim_amd import api

    return api.Context(0, 1)


_PAIRS, _MAPS = {}, {}


def pair(orc, ctx, size):
    """the two scans of tests/test_gicp.py::clouds at a size (rings, az), built once per context, that is once per module"""
    from glim_amd import api
    from test_gicp import clouds

    if (id(ctx), size) not in _PAIRS:
        _PAIRS[(id(ctx), size)] = clouds(orc, api, ctx, rings=size[0], az=size[1])
    return _PAIRS[(id(ctx), size)]


def vmap(orc, ctx, size, res):
    """the device voxel map of the target scan of a size at a resolution, built once per context"""
    from glim_amd import api

    if (id(ctx), size, res) not in _MAPS:
        ((tp, tc, tg), _), _ = pair(orc, ctx, size)
        _MAPS[(id(ctx), size, res)] = api.GaussianVoxelMapGPU(res, ctx=ctx).insert(tg)
    return _MAPS[(id(ctx), size, res)]


def api_params(kw, factory="LMParams"):
    from glim_amd import api

    return getattr(api, factory)(**kw)


def same_record(compact, T, L):
    from glim_amd import api

    ex = api.expand_compact(compact, T, 0)
    return ex["num_inliers"] == L["num_inliers"] and ex["error"] == L["error"] and np.array_equal(ex["H_ss"], L["H_ss"]) and np.array_equal(ex["b_s"], L["b_s"])


ALIGN_FIELDS = ("T_target_source", "error", "num_inliers", "iterations", "trials", "status", "lam", "compact")
BUNDLE_FIELDS = ("poses", "cost", "factor_cost", "prior_cost", "between_cost", "lam", "num_inliers", "iterations", "trials", "status", "compact")


def same_result(a, b):
    """two results of glim_amd_*_align_batch, or two of glim_amd_bundle_align, hold the same bits"""
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in (BUNDLE_FIELDS if hasattr(a, "poses") else ALIGN_FIELDS))


def moves(trace, cost=False):
    """|e_new - e_cur| / e_cur of every trial of a restatement trace.  cost: of a loop with terms, where "the error" is the total cost"""
    at = (lambda e: e["cost"]) if cost else (lambda e: e["record"]["error"])
    kept = (lambda e: e["state"]["sys"]["cost"]) if cost else (lambda e: e["state"]["rec"]["error"])
    out, e_cur = [], at(trace[0])
    for e in trace[1:]:
        out.append(abs(at(e) - e_cur) / e_cur)
        e_cur = kept(e)
    return out


def teacher_forced(linearize_all, results, traces, T0s, p):
    """Test 1 for one batch: every trace record is the caller's own record at the trace's poses, bit for bit; the restatement, fed that record
    from the device's own previous state, takes the same decision and proposes the same next pose.  linearize_all(poses) -> the B records of
    round k: ONE evaluation of the whole batch; a problem that has finished keeps its last pose there (its record is not looked at)."""
    B = len(results)
    states = [lmr.new_state(T0, p) for T0 in T0s]
    for i in range(B):
        assert len(traces[i]) == results[i].trials + 1
    for k in range(max(len(t) for t in traces)):
        records = linearize_all([traces[i][min(k, len(traces[i]) - 1)]["T"] for i in range(B)])
        for i in range(B):
            if k >= len(traces[i]):
                continue
            e, s, L = traces[i][k], states[i], records[i]
            assert same_record(e["compact"], e["T"], L), (i, k)
            assert e["lam"] == s["lam"], (i, k)
            if k == 0:
                assert np.array_equal(e["T"], T0s[i])
            else:
                assert np.abs(e["T"] - s["cand"]).max() <= lmr.pose_gate(s), (i, k, np.abs(e["T"] - s["cand"]).max(), lmr.pose_gate(s))
            s["cand"] = e["T"]  # teacher forcing: the device's pose is the one the record belongs to
            s = states[i] = lmr.step(p, s, L)
            assert (e["accepted"], e["status"]) == (s["accepted"], s["status"]), (i, k)
    for i, (s, r) in enumerate(zip(states, results)):
        assert s["status"] != lmr.RUNNING and (r.status, r.iterations, r.trials) == (s["status"], s["iterations"], s["trials"]), i
        assert np.array_equal(r.T_target_source, s["T"]) and r.lam == s["lam"], i
        assert same_record(r.compact, r.T_target_source, s["rec"]) and r.error == s["rec"]["error"] and r.num_inliers == s["rec"]["num_inliers"], i
    return states


def packed(p, c):
    """points and covariances as the C++ mirror programs upload them: n x 4 and n x 16 (column-major 4 x 4)"""
    p4 = np.ones((len(p), 4))
    p4[:, :3] = p
    m = np.zeros((len(p), 4, 4))
    m[:, :3, :3] = c
    return p4, np.ascontiguousarray(np.transpose(m, (0, 2, 1))).reshape(len(p), 16)


# ---- on the CPU ------------------------------------------------------------------------------------------------------------------------------
def check_symbols(stable, diag, mirror_header):
    """the new entry points are declared once, in the header they belong to, listed in _lib.SYMBOLS and resolved; the C++ mirror knows nothing
    of the diagnostic header.  -> the mirror's text"""
    from glim_amd import _lib

    decl = {h: re.findall(r"\b(glim_amd_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", h)).read()) for h in ("glim_amd.h", "glim_amd_diag.h")}
    for n in stable:
        assert decl["glim_amd.h"].count(n) == 1 and n not in decl["glim_amd_diag.h"] and n in _lib.SYMBOLS, n
    for n in diag:
        assert decl["glim_amd_diag.h"].count(n) == 1 and n not in decl["glim_amd.h"] and n in _lib.SYMBOLS, n
    mirror = open(os.path.join(ROOT, "include", "glim_amd", mirror_header)).read()
    assert "glim_amd_diag.h" not in mirror and "glim_amd_debug_" not in mirror
    L = _lib.lib()
    for n in stable + diag:
        assert hasattr(L, n)
    return mirror


def build_driver(tmp_path_factory, name, *flags):
    """tests/cpp/test_<name>.cpp, the host driver of a step header, under a plain C++ compiler with contraction off -> the program"""
    exe = str(tmp_path_factory.mktemp(name) / ("test_" + name))
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", *flags, os.path.join(ROOT, "tests", "cpp", "test_" + name + ".cpp"), "-o", exe])
    return exe


def params_head(p):
    """the nine doubles every `step` input of a host driver begins with: glim_amd_lm_params in its order, max_trials resolved"""
    head = [p[k] for k in ("lambda_initial", "lambda_factor", "lambda_upper_bound", "lambda_lower_bound", "relative_error_tol", "absolute_error_tol")]
    return head + [float(p["max_iterations"]), float(p["max_trials"]), p["error_scale"]]


def check_against_restatement(rows, states, cand=("cand",), kept=("T",), cost_floor=0.0, gate_scale=1.0):
    """The rounds of a host driver against the restatement's states after the same rounds.  Decisions, counts, statuses and lambda are equal
    (lambda moves by one division or multiplication per round: the same double on both sides); where the loop has terms the kept cost agrees to
    1e-12 of itself (cost_floor: what a cost that goes to zero is known to, absolutely).  While the loop runs, the step is within the
    self-scaled gate of lm_restatement.solve -- 100 cond(H + lambda I) eps max(|delta|, 1e-12), from the reference's own matrix, times
    gate_scale -- and the poses `cand` and `kept` within what that step error does to the retractions (lm_restatement.pose_gate)."""
    assert len(rows) == len(states)
    for k, (got, s) in enumerate(zip(rows, states)):
        assert (got["accepted"], got["status"], got["iterations"], got["trials"]) == (s["accepted"], s["status"], s["iterations"], s["trials"]), k
        assert got["lam"] == s["lam"], k
        if "cost" in got and s["sys"] is not None:
            assert abs(got["cost"] - s["sys"]["cost"]) <= 1e-12 * abs(s["sys"]["cost"]) + cost_floor, k
        if s["status"] != lmr.RUNNING:
            continue
        assert got["solve_ok"] == s["solve_ok"], k
        s = dict(s, gate=s["gate"] * gate_scale)
        assert np.abs(got["delta"] - s["delta"]).max() <= s["gate"], (k, np.abs(got["delta"] - s["delta"]).max(), s["gate"])
        gate = lmr.pose_gate(s, cand)
        for name in cand + kept:
            assert np.abs(got[name] - s[name]).max() <= gate, (k, name, np.abs(got[name] - s[name]).max(), gate)


def build_cpp(tmp_path, name):
    """tests/cpp/test_<name>.cpp, a program over a C++ mirror of include/glim_amd/, compiled and linked against the built library"""
    from glim_amd import _lib

    assert os.path.exists(_lib.LIB_PATH)
    exe = str(tmp_path / ("test_" + name))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_" + name + ".cpp"),
                           "-o", exe, "-L" + os.path.join(ROOT, "glim_amd"), "-lglim_amd", "-Wl,-rpath," + os.path.join(ROOT, "glim_amd"), "-Wl,-rpath,/opt/rocm/lib",
                           "-L/opt/rocm/lib", "-lamdhip64"])
    return exe
