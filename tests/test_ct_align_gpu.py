"""CT-GICP frame alignment on the device (include/glim_amd.h "CT-GICP frame alignment", glim_amd/csrc/ct_align.hip): the device pose table is
the host's, every trial record is the factor's at the trial's pair, the decisions are those of tests/ct_lm_restatement.py, and the call leaves
the factor's kept state alone.  Cases and scenes: tests/ct_align_cases.py."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import ct_lm_restatement as ctl
from align_cases import build_cpp, ctx, packed  # noqa: F401 (ctx: a fixture)
from ct_align_cases import CASES, case_inputs, pose_table_cases
from ct_restatement import POSE_TOL, _check_record, expmap, moving_source, np_ct_linearize, static_map, sweep_poses

pytestmark = pytest.mark.gpu

_SCENE = {}


def device_cloud(ctx, pts):
    from glim_amd import api

    g = api.PointCloudGPU.clone(pts, ctx=ctx)
    g.find_neighbors(10, download=False)
    g.estimate_covariances(10)
    xyz, c, _ = g.download(covs=True, normals=False)
    return xyz.astype(np.float64), c.astype(np.float64), g


def scene(ctx, points):
    """-> ((tp, tc, target cloud), (sp, sc, source cloud, times)) of the cases' scenes with the device's covariances; built once per module"""
    if "target" not in _SCENE:
        _SCENE["target"] = device_cloud(ctx, static_map(16, 512))
        _SCENE["raw"] = moving_source(16, 256)
    if points not in _SCENE:
        p, t = _SCENE["raw"]
        _SCENE[points] = device_cloud(ctx, p[:points]) + (t[:points].copy(),)
    return _SCENE["target"], _SCENE[points]


def ivox_map(ctx):
    """the target as a device iVox searched in neighbour mode 1 (config_odometry_ct.json's)"""
    from glim_amd import api

    if "ivox" not in _SCENE:
        m = api.IncrementalVoxelMap(1.0, ctx=ctx)
        m.voxel_insertion_setting(min_dist=0.05, max_points=20)
        m.set_neighbor_voxel_mode(1)
        m.insert(_SCENE["target"][2])
        _SCENE["ivox"] = m
    return _SCENE["ivox"]


def make_factor(ctx, name, target="index"):
    from glim_amd import api

    (tp, tc, tg), (sp, sc, sg, times) = scene(ctx, CASES[name]["points"])
    X0, Y0, tm, max_d = case_inputs(name)
    tgt = tg if target == "index" else ivox_map(ctx)
    f = api.IntegratedCT_GICPFactor(0, 1, tgt, sg, max_correspondence_distance=max_d, times=times)
    return f, X0, Y0, tm, max_d


def api_terms(tm):
    return dict(location_prior=tm["location"], between=tm["between"])


def api_params(**kw):
    from glim_amd import api

    return api.ct_align_params(**kw)


def miss(A, B):
    return float(np.linalg.norm((np.linalg.inv(B) @ A)[:3, 3]))


@pytest.mark.parametrize("name", list(pose_table_cases()))
def test_device_pose_table_is_the_hosts(ctx, name):
    from glim_amd import api

    table, X, Y = pose_table_cases()[name]
    _, (sp, sc, sg, times) = scene(ctx, 4001)
    (_, _, tg), _ = scene(ctx, 4001)
    f = api.IntegratedCT_GICPFactor(0, 1, tg, sg, times=np.zeros(len(sp)) if table is not None else times)
    values = {0: X, 1: Y}
    tab, T, D0, D1, _ = f.debug_poses(values)
    assert len(tab) == 1 if table is not None else 80 <= len(tab) <= 90
    Td, D0d, D1d = f.debug_align_poses(values)
    dev = max(np.abs(Td - T).max(), np.abs(D0d - D0).max(), np.abs(D1d - D1).max())
    print("pose table", name, "buckets", len(tab), "max |device - host|", dev)
    assert dev < 1e-12
    # the kernel wrote the factor's table: the next linearize uploads the host's again and is what it was
    a = f.linearize(values)
    f.debug_align_poses({0: Y, 1: X})
    b = f.linearize(values)
    assert a["error"] == b["error"] and np.array_equal(a["H_01"], b["H_01"])
    f.close()


@pytest.mark.parametrize("target", ["index", "ivox"])
@pytest.mark.parametrize("name", ["C", "A"])
def test_teacher_forced_trace(ctx, name, target):
    from glim_amd import api

    f, X0, Y0, tm, _ = make_factor(ctx, name, target)
    values = {0: X0, 1: Y0}
    p = ctl.params()
    result, trace = api.ct_align_debug_trace(f, values, params=api_params(), **api_terms(tm))
    assert len(trace) == result.trials + 1 >= 3
    assert np.array_equal(trace[0]["X"], X0) and np.array_equal(trace[0]["Y"], Y0) and trace[0]["lam"] == p["lambda_initial"]
    s = ctl.new_state(X0, Y0, p)
    kept = None
    for k, e in enumerate(trace):
        # the record is the factor's at the entry's pair (the device's pose table against the host's: 1e-12 on the poses)
        got = ctl.record_of_row(e["record"])
        ref = f.linearize({0: e["X"], 1: e["Y"]})
        assert got["num_inliers"] == ref["num_inliers"]
        _check_record(got, ref)
        # the restatement, fed the device's record, decides the same and goes to the same next pair
        assert e["lam"] == s["lam"], k
        gate = ctl.pose_gate(s) if k else 0.0
        assert np.abs(e["X"] - s["candX"]).max() <= gate and np.abs(e["Y"] - s["candY"]).max() <= gate, (k, gate)
        s = ctl.step(p, tm, dict(s, candX=e["X"], candY=e["Y"]), got)
        assert (e["accepted"], e["status"]) == (s["accepted"], s["status"]), k
        assert abs(e["cost"] - ctl.assemble(tm, e["X"], e["Y"], got)["cost"]) <= 1e-12 * e["cost"], k
        if e["accepted"]:
            kept = e
        # teacher-forced: the kept pair is the device's own bits from here on
        s = dict(s, X=kept["X"], Y=kept["Y"])
    assert (result.status, result.iterations, result.trials) == (s["status"], s["iterations"], s["trials"]) and result.lam == s["lam"]
    assert result.status != 0 and trace[-1]["status"] == result.status and all(e["status"] == 0 for e in trace[:-1])
    # the result is the last kept state, bit for bit: its pair, its record, its cost
    assert np.array_equal(result.X, kept["X"]) and np.array_equal(result.Y, kept["Y"]) and result.cost == kept["cost"]
    assert np.array_equal(ctl.row_of_record(result.linearized), kept["record"])
    S = ctl.assemble(tm, result.X, result.Y, result.linearized)
    np.testing.assert_allclose([result.location_cost, result.between_cost], [S["cost_p"], S["cost_b"]], rtol=1e-9, atol=1e-12 * result.cost)
    assert result.cost == (result.error + result.location_cost) + result.between_cost
    # the call without the trace returns the same bytes
    plain = f.align(values, params=api_params(), **api_terms(tm))
    assert plain.raw == result.raw
    if name == "C" and target == "index":
        assert [e["accepted"] for e in trace[1:4]] == [True, True, True]
    f.close()


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_free_running_two_iterations(orc, ctx, name):
    """max_iterations = 2: both trials move the cost by >= 1.4e-2 of itself, 70 x the record tolerance, so a free-running loop takes the decisions
    of any correct implementation.  Measured on an MI355X (max |device - restatement| over X and Y, 3 x 4 entries): see DESIGN.md 4.7d."""
    f, X0, Y0, tm, max_d = make_factor(ctx, name)
    (tp, tc, _), (sp, sc, _, times) = scene(ctx, CASES[name]["points"])
    p = ctl.params(max_iterations=2)
    got = f.align({0: X0, 1: Y0}, params=api_params(max_iterations=2), **api_terms(tm))
    assert (got.status, got.iterations, got.trials) == (ctl.MAX_ITERATIONS, 2, 2)
    own, _ = ctl.run(lambda X, Y: f.linearize({0: X, 1: Y}), X0, Y0, tm, p)
    assert (own["status"], own["iterations"], own["trials"]) == (ctl.MAX_ITERATIONS, 2, 2)
    d_own = max(np.abs(got.X - own["X"]).max(), np.abs(got.Y - own["Y"]).max())
    ref, ref_trace = ctl.run(lambda X, Y: np_ct_linearize(orc, tp, tc, sp, sc, times, X, Y, max_d), X0, Y0, tm, p)
    assert (ref["status"], ref["iterations"], ref["trials"]) == (ctl.MAX_ITERATIONS, 2, 2) and all(e["accepted"] for e in ref_trace)
    d_ref = max(np.abs(got.X - ref["X"]).max(), np.abs(got.Y - ref["Y"]).max())
    print("free-running", name, "vs restatement on factor.linearize", d_own, "vs restatement on the oracle", d_ref)
    assert d_own < POSE_TOL
    assert d_ref < 2 * POSE_TOL
    f.close()


@pytest.mark.parametrize("name", ["A", "B"])
def test_full_run_recovers_the_sweep_and_leaves_the_kept_state(ctx, name):
    f, X0, Y0, tm, _ = make_factor(ctx, name)
    T0, T1 = sweep_poses()
    start = miss(Y0, T1)
    assert 0.25 < start < 0.7
    # error() at other values, after a linearize elsewhere, before and after an align
    lin_at = {0: X0 @ expmap([0.001, 0.0, -0.001, 0.01, 0.0, 0.01]), 1: Y0}
    other = {0: X0, 1: Y0 @ expmap([0.0, 0.002, 0.0, -0.01, 0.02, 0.0])}
    f.linearize(lin_at)
    before = f.error(other, with_inliers=True)
    r = f.align({0: X0, 1: Y0}, params=api_params(), **api_terms(tm))
    after = f.error(other, with_inliers=True)
    assert before == after
    mx, my = miss(r.X, T0), miss(r.Y, T1)
    print("full run", name, r.status_name, "iterations", r.iterations, "trials", r.trials, "miss X", mx, "miss Y", my, "start", start)
    assert r.iterations >= 2 and r.status in (ctl.CONVERGED, ctl.MAX_ITERATIONS, ctl.MAX_TRIALS, ctl.LAMBDA_BOUND)
    assert mx < start / 4 and my < start / 4
    f.close()


def test_edge_cases(ctx):
    from glim_amd import _lib, api

    (tp, tc, tg), (sp, sc, sg, times) = scene(ctx, 4001)
    X0, Y0, tm, _ = case_inputs("A")
    values = {0: X0, 1: Y0}
    # one bucket (all times equal): Y's block of the factor is zero, the between term alone moves Y
    f1 = api.IntegratedCT_GICPFactor(0, 1, tg, sg, times=np.zeros(len(sp)))
    r, trace = api.ct_align_debug_trace(f1, values, params=api_params(max_iterations=2), **api_terms(tm))
    L = r.linearized
    assert not np.any(L["H_11"]) and not np.any(L["H_01"]) and not np.any(L["b_1"]) and r.iterations >= 1
    assert not np.array_equal(r.Y, Y0) and r.between_cost > 0
    nob = f1.align(values, location_prior=tm["location"], params=api_params(max_iterations=2))
    assert nob.iterations >= 1 and not np.array_equal(nob.X, X0) and np.array_equal(nob.Y, Y0)  # without it Y's step is zero
    f1.close()
    f = api.IntegratedCT_GICPFactor(0, 1, tg, sg, times=times)
    # max_iterations = 0: the initial pair with the record at it
    r0 = f.align(values, params=api_params(max_iterations=0), **api_terms(tm))
    assert (r0.status, r0.iterations, r0.trials) == (ctl.MAX_ITERATIONS, 0, 0) and np.array_equal(r0.X, X0) and np.array_equal(r0.Y, Y0)
    _check_record(r0.linearized, f.linearize(values))
    # both precisions 0 and no terms: the same bytes
    a = f.align(values, params=api_params(max_iterations=2))
    b = f.align(values, location_prior=(X0, 0.0), between=(np.eye(4), 0.0), params=api_params(max_iterations=2))
    assert a.raw == b.raw and a.location_cost == 0.0 and a.between_cost == 0.0 and a.cost == a.error
    # a second call, and a second context: the same bytes
    full = f.align(values, params=api_params(), **api_terms(tm))
    assert f.align(values, params=api_params(), **api_terms(tm)).raw == full.raw
    ctx2 = api.Context(0, 1)
    tg2, sg2 = device_cloud(ctx2, static_map(16, 512))[2], device_cloud(ctx2, _SCENE["raw"][0][:4001])[2]
    f2 = api.IntegratedCT_GICPFactor(0, 1, tg2, sg2, times=times)
    assert f2.align(values, params=api_params(), **api_terms(tm)).raw == full.raw
    f2.close()
    for g in (tg2, sg2):
        g.close()
    ctx2.close()
    # no target point in range: NO_CORRESPONDENCES with the initial pair
    far = np.eye(4)
    far[:3, 3] = [500.0, 500.0, 50.0]
    rn = f.align({0: far, 1: far}, params=api_params(), **api_terms(tm))
    assert rn.status == ctl.NO_CORRESPONDENCES and rn.num_inliers == 0 and np.array_equal(rn.X, far) and np.array_equal(rn.Y, far) and rn.trials == 0
    # argument errors with real handles
    L = _lib.lib()
    out = _lib.CtAlignResult()
    X12, Y12 = api.pose12(X0).copy(), api.pose12(Y0).copy()
    px, py = X12.ctypes.data_as(C.POINTER(C.c_double)), Y12.ctypes.data_as(C.POINTER(C.c_double))
    assert L.glim_amd_ct_align(f._h, px, py, None, None, C.byref(out)) == 0
    assert L.glim_amd_ct_align(f._h, None, py, None, None, C.byref(out)) == -1
    assert L.glim_amd_ct_align(f._h, px, None, None, None, C.byref(out)) == -1
    assert L.glim_amd_ct_align(f._h, px, py, None, None, None) == -1
    assert L.glim_amd_debug_ct_align_trace(f._h, px, py, None, None, C.byref(out), None) == -1
    for kp, kb, bad in ((np.nan, 0.0, False), (-1.0, 0.0, False), (0.0, -1.0, False), (0.0, 1.0, True)):
        t = _lib.CtAlignTerms()
        t.T_location[:] = list(X12)
        t.T_between[:] = list(X12)
        if bad:
            t.T_between[0] = np.nan
        t.location_precision, t.between_precision = kp, kb
        assert L.glim_amd_ct_align(f._h, px, py, C.byref(t), None, C.byref(out)) == -1
    t = _lib.CtAlignTerms()
    t.T_between[0] = np.nan  # a term that is off is not read
    assert L.glim_amd_ct_align(f._h, px, py, C.byref(t), None, C.byref(out)) == 0
    bad = api_params()._c()
    bad.lambda_factor = 1.0
    assert L.glim_amd_ct_align(f._h, px, py, None, C.byref(bad), C.byref(out)) == -1
    f.close()
    # an empty source, an empty target: INVALID
    empty = api.PointCloudGPU.clone(np.zeros((0, 3)), covs=np.zeros((0, 3, 3)), ctx=ctx)
    for tgt, src, tt in ((tg, empty, np.zeros(0)), (empty, sg, times)):
        fe = api.IntegratedCT_GICPFactor(0, 1, tgt, src, times=tt)
        with pytest.raises(api.GlimAmdError) as ei:
            fe.align(values)
        assert ei.value.code == -1
        fe.close()


def test_cpp_mirror_returns_the_python_result(ctx, tmp_path):
    """tests/cpp/test_ct_align.cpp calls glim_amd::align_ct and the compat class's align on clouds it uploads itself from the dumped arrays"""
    from glim_amd import api

    (tp, tc, _), (sp, sc, _, times) = scene(ctx, 4001)
    X0, Y0, tm, max_d = case_inputs("A")

    (tp4, tc16), (sp4, sc16) = packed(tp, tc), packed(sp, sc)
    tg, sg = api.PointCloudGPU.clone_packed(tp4, tc16, ctx=ctx), api.PointCloudGPU.clone_packed(sp4, sc16, ctx=ctx)
    f = api.IntegratedCT_GICPFactor(0, 1, tg, sg, max_correspondence_distance=max_d, times=times)
    res = f.align({0: X0, 1: Y0}, **api_terms(tm))
    assert res.iterations >= 2
    f.close()
    path = tmp_path / "case.bin"
    (P, kp), (D, kb) = tm["location"], tm["between"]
    with open(path, "wb") as fh:
        fh.write(struct.pack("<ii", len(tp), len(sp)))
        for a in (tp4, tc16, sp4, sc16, times, [max_d], api.pose12(X0), api.pose12(Y0), api.pose12(P), [kp], api.pose12(D), [kb]):
            fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        fh.write(res.raw)
    exe = build_cpp(tmp_path, "ct_align")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "test_ct_align OK" in out.stdout, out.stdout + out.stderr
