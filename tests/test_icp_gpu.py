"""The ICP factors on the device (include/glim_amd.h "ICP factors", glim_amd/csrc/icp_factor.hpp, icp_kernel of gicp.hip) against the FP64
restatement (tests/icp_restatement.py): correspondences to the bit, records at the project's record tolerance, and the edges of the call."""
import subprocess

import numpy as np
import pytest

import icp_restatement as icpr
import lm_restatement as lmr
from align_cases import BIG, RECORD_TOL, SMALL, ctx, pair  # noqa: F401 (ctx: a fixture)
from ct_restatement import gn_step
from test_gicp import POSE_TOL, rigid_edge_sizes, rigid_edge_subset
from test_icp import build_drop_in

pytestmark = pytest.mark.gpu
PERT = [0.004, -0.003, 0.002, 0.03, 0.02, -0.01]  # of test_hip_gicp_matches_oracle
_BARE = {}


def bare(orc, ctx, size):
    """the pair of a size WITHOUT covariances -- the case GLIM reaches -- (target, target with normals only, source), the target's normals as the
    device holds them, and what every case of a size shares: the pose, q = T p and the exact nearest neighbours, computed once"""
    from glim_amd import api

    if (id(ctx), size) not in _BARE:
        ((tp, tc, tg), (sp, sc, sg)), delta = pair(orc, ctx, size)
        normals = tg.download(covs=False, normals=True)[2].astype(np.float64)
        T = delta @ orc.se3_exp(PERT)
        q = icpr.transform(sp, T)
        _BARE[(id(ctx), size)] = dict(target=api.PointCloudGPU.clone(tp, ctx=ctx), target_n=api.PointCloudGPU.clone(tp, normals=normals, ctx=ctx),
                                      source=api.PointCloudGPU.clone(sp, ctx=ctx), normals=normals, T=T, q=q, nn=icpr.nearest(tp, q))
    return _BARE[(id(ctx), size)]


def check_record(got, ref, T, binary, step=True):
    """the form of test_hip_gicp_matches_oracle at the project's record tolerance"""
    from glim_amd import api

    assert got["num_inliers"] == ref["num_inliers"]
    scale = np.abs(ref["H_ss"]).max()
    worst = max(abs(got["error"] - ref["error"]) / ref["error"], np.abs(got["H_ss"] - ref["H_ss"]).max() / scale)
    print(f"inliers {got['num_inliers']}, error {got['error']:.9g} / {ref['error']:.9g}, worst relative record difference {worst:.3e}")
    np.testing.assert_allclose(got["error"], ref["error"], rtol=RECORD_TOL)
    np.testing.assert_allclose(got["H_ss"], ref["H_ss"], rtol=0, atol=RECORD_TOL * scale)
    np.testing.assert_allclose(got["b_s"], ref["b_s"], rtol=0, atol=RECORD_TOL * np.abs(ref["b_s"]).max() + 1e-6 * scale)
    if binary:
        ex = api.expand_compact(lmr.compact_of_record(ref), T, api.FACTOR_BINARY)
        for k in ("H_tt", "H_ts"):
            np.testing.assert_allclose(got[k], ex[k], rtol=0, atol=RECORD_TOL * np.abs(ex[k]).max())
        np.testing.assert_allclose(got["b_t"], ex["b_t"], rtol=0, atol=RECORD_TOL * np.abs(ex["b_t"]).max() + 1e-6 * scale)
    else:
        assert not np.any(got["H_tt"]) and not np.any(got["H_ts"]) and not np.any(got["b_t"])
    if step:
        lam = 1e-6 * np.trace(ref["H_ss"]) / 6
        assert np.abs(gn_step(got, lam) - gn_step(ref, lam)).max() < POSE_TOL


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
@pytest.mark.parametrize("max_d", [1.0, 0.5, 0.05])
@pytest.mark.parametrize("size", [SMALL, BIG], ids=["16x128", "32x384"])
def test_factor_matches_the_restatement(orc, ctx, size, max_d, plane):
    from glim_amd import api

    ((tp, tc, tg), (sp, sc, sg)), delta = pair(orc, ctx, size)
    b = bare(orc, ctx, size)
    T = b["T"]
    corr = icpr.correspondences(b["nn"], max_d)
    ref = icpr.icp_linearize(tp, sp, T, max_d, normals=b["normals"] if plane else None, corr=corr, q=b["q"])
    assert ref["num_inliers"] > 50
    gicp = api.IntegratedGICPFactor(np.eye(4), 1, tg, sg, max_correspondence_distance=max_d)
    values = {0: np.eye(4), 1: T}
    np.testing.assert_array_equal(gicp.correspondences(values), corr)
    for binary in (False, True):
        f = api.IntegratedICPFactor(0 if binary else np.eye(4), 1, b["target_n"] if plane else b["target"], b["source"], max_correspondence_distance=max_d,
                                    use_point_to_plane=plane)
        np.testing.assert_array_equal(f.correspondences(values), corr)
        got = f.linearize(values)
        check_record(got, ref, T, binary)
        assert f.inlier_fraction() == ref["num_inliers"] / len(sp)
        e = f.error(values)
        assert abs(e - ref["error"]) <= RECORD_TOL * ref["error"] and f.inlier_fraction() == ref["num_inliers"] / len(sp)
        f.close()
    gicp.close()


def test_point_to_plane_sibling_and_shared_index(orc, ctx):
    """IntegratedPointToPlaneICPFactor is the flag; one index serves a GICP factor and both ICP factors at once, each with its own distance"""
    from glim_amd import api

    ((tp, tc, tg), (sp, sc, sg)), delta = pair(orc, ctx, SMALL)
    owner = api.IntegratedGICPFactor(np.eye(4), 1, tg, sg, max_correspondence_distance=1.0)  # tg has covariances and normals
    point = api.IntegratedICPFactor(np.eye(4), 1, tg, sg, target_tree=owner.target_tree, max_correspondence_distance=0.25)
    plane = api.IntegratedPointToPlaneICPFactor(np.eye(4), 1, tg, sg, target_tree=owner.target_tree, max_correspondence_distance=0.25)
    flag = api.IntegratedICPFactor(np.eye(4), 1, tg, sg, target_tree=owner.target_tree, max_correspondence_distance=0.25, use_point_to_plane=True)
    v = {1: delta}
    before = owner.linearize(v)
    a, b, c = point.linearize(v), plane.linearize(v), flag.linearize(v)
    assert 0 < a["num_inliers"] == b["num_inliers"] <= before["num_inliers"]
    assert b["error"] == c["error"] and np.array_equal(b["H_ss"], c["H_ss"]) and np.array_equal(b["b_s"], c["b_s"])
    assert 0 < b["error"] < a["error"]  # |n o r|^2 <= |r|^2 for unit normals
    np.testing.assert_array_equal(point.correspondences(v), api.IntegratedGICPFactor(np.eye(4), 1, tg, sg, target_tree=owner.target_tree,
                                                                                       max_correspondence_distance=0.25).correspondences(v))
    after = owner.linearize(v)
    assert after["error"] == before["error"] and np.array_equal(after["H_ss"], before["H_ss"])  # the index is shared, never changed
    for f in (point, plane, flag, owner):
        f.close()


def test_edges(orc, ctx):
    from glim_amd import api

    ((tp, tc, tg), (sp, sc, sg)), delta = pair(orc, ctx, SMALL)
    b = bare(orc, ctx, SMALL)
    far = delta.copy()
    far[0, 3] += 1e3
    for plane in (False, True):
        f = api.IntegratedICPFactor(np.eye(4), 1, b["target_n"], b["source"], use_point_to_plane=plane)
        L = f.linearize({1: far})  # no correspondences: zero information, never NaN
        assert L["num_inliers"] == 0 and L["error"] == 0.0 and not np.any(L["H_ss"]) and not np.any(L["b_s"])
        assert f.error({1: far}) == 0.0 and f.inlier_fraction() == 0.0 and np.all(f.correspondences({1: far}) == -1)
        # a radius far beyond what the index was sized for is refused, not searched incompletely
        f.set_max_correspondence_distance(100.0)
        with pytest.raises(api.GlimAmdError) as e:
            f.linearize({1: delta})
        assert e.value.code == -6
        with pytest.raises(api.GlimAmdError) as e:
            f.error({1: delta})
        assert e.value.code == -6
        f.set_max_correspondence_distance(5.0)  # 5 x the hint: fine, and still exact
        np.testing.assert_array_equal(f.correspondences({1: delta}), icpr.correspondences(icpr.nearest(tp, icpr.transform(sp, delta)), 5.0))
        f.close()
    empty = api.PointCloudGPU.clone(np.zeros((0, 3)), ctx=ctx)
    for plane in (False, True):
        for t, s in ((b["target_n"], empty), (empty, b["source"])):
            if plane and t is empty:
                continue  # (an empty cloud has no normals: the state error below)
            f = api.IntegratedICPFactor(np.eye(4), 1, t, s, use_point_to_plane=plane)
            L = f.linearize({1: delta})
            assert L["num_inliers"] == 0 and L["error"] == 0.0 and not np.any(L["H_ss"]) and f.error({1: delta}) == 0.0
            f.close()
    # point-to-plane without target normals is a state error, not a crash; point-to-point over the same clouds is fine
    f = api.IntegratedPointToPlaneICPFactor(np.eye(4), 1, b["target"], b["source"])
    for call in (f.linearize, f.error):
        with pytest.raises(api.GlimAmdError) as e:
            call({1: delta})
        assert e.value.code == -5
    f.close()
    empty.close()


def test_source_sizes_at_the_edges_of_the_block_epilogue_and_the_ordered_sum(orc, ctx):
    """1 point, a block less one, a block, a block and one, and one block more than a full finaliser trip, both metrics, against the restatement;
    the GN step from a block less one on (one point gives a rank-deficient system)"""
    from glim_amd import api

    ((tp, tc, tg), (sp, sc, sg)), delta = pair(orc, ctx, SMALL)
    b = bare(orc, ctx, SMALL)
    T = b["T"]
    sizes = rigid_edge_sizes(ctx.device_info()["num_cus"])
    assert sizes[:4] == [1, 255, 256, 257]
    reps = -(-sizes[-1] // len(sp))  # the largest size from shifted copies of the scan (a millimetre apart: the same surfaces)
    big = np.concatenate([(sp + 1e-3 * k).astype(np.float32).astype(np.float64) for k in range(reps)])[: sizes[-1]]
    owner = api.IntegratedICPFactor(np.eye(4), 1, b["target_n"], b["source"], max_correspondence_distance=1.0)
    for n in sizes:
        pts = big if n == sizes[-1] else sp[rigid_edge_subset(sp, n)]
        g = api.PointCloudGPU.clone(pts, ctx=ctx)
        q = icpr.transform(pts, T)
        corr = icpr.correspondences(icpr.nearest(tp, q), 1.0)
        for plane in (False, True):
            f = api.IntegratedICPFactor(np.eye(4), 1, b["target_n"], g, target_tree=owner.target_tree, max_correspondence_distance=1.0, use_point_to_plane=plane)
            ref = icpr.icp_linearize(tp, pts, T, 1.0, normals=b["normals"] if plane else None, corr=corr, q=q)
            assert ref["num_inliers"] > 0
            np.testing.assert_array_equal(f.correspondences({1: T}), corr)
            check_record(f.linearize({1: T}), ref, T, False, step=n > 1)
            assert abs(f.error({1: T}) - ref["error"]) <= RECORD_TOL * ref["error"]
            f.close()
        g.close()
    owner.close()


def test_drop_in_header_on_the_device(tmp_path):
    """tests/cpp/test_icp_drop_in.cpp: gtsam_points::IntegratedICPFactor / IntegratedPointToPlaneICPFactor of the drop-in tree, driven as GLIM drives them"""
    out = subprocess.run([build_drop_in(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "test_icp_drop_in OK (3000 points" in out.stdout, out.stdout + out.stderr
