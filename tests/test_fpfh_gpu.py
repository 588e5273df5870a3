"""Device FPFH (glim_amd_fpfh_estimate) and descriptor matching (glim_amd_fpfh_match) against the NumPy restatement (tests/fpfh_restatement.py).

Parity gate of the descriptors: the device's FP64 pair features differ from NumPy's by ~1e-15, so as long as no feature of the input lies within
1e-9 of a bin edge (asserted on the input) every bin decision, hence every count, is the same; what is left is the FP64 summation order and ONE
rounding to FP32 of values <= 100: |device - reference| <= 100 * 2^-23 (one FP32 rounding of a value <= 100, doubled).

Matching gate: FP32 error bound of a 36-term product e = 36 * 2^-24 * (|a|^2 + |b|^2).  A query counts when the reference's gap between best and
second best exceeds 50 e (50 = slack over the worst-case bound); on counted queries the index must be equal, on ALL queries the returned distance is
within 50 e of the reference distance to the returned index.  At most 5 % of the queries may be left out; the crops and the seed were chosen on the
CPU so that the reference alone meets that, and the test asserts it."""
import os
import struct
import subprocess

import numpy as np
import pytest

import fpfh_restatement as R
from registration_cases import room_scan as _room_scan

pytestmark = pytest.mark.gpu

GATE = 100.0 * 2.0 ** -23
SLACK = 50.0


@pytest.fixture(scope="module")
def ctx():
    """Not closed by hand: a context refuses to go while a child is alive, and the clouds that the `pytest.raises` blocks below caught an error
    on stay in the reference cycle of their traceback until the collector runs.  As in the other GPU test modules, Context.__del__ sees to it."""
    from glim_amd import api

    return api.Context(0, 1)


def _device_cloud(ctx, pts32, normals32=None):
    """normals32 None: kNN(10) + covariance estimation on the device"""
    from glim_amd import api

    c = api.PointCloudGPU.clone(pts32, normals=normals32, ctx=ctx)
    if normals32 is None:
        c.find_neighbors(10, download=False)
        c.estimate_covariances(10)
    return c


def _check_descriptors(got, ref):
    err = np.abs(got.astype(np.float64) - ref["F"])
    print(f"n = {len(got)}: median k {np.median(ref['k'])}, max k {ref['k'].max()}, max |device - reference| = {err.max():.3e} (gate {GATE:.3e})")
    assert err.max() <= GATE


@pytest.fixture(scope="module")
def parity_cloud(ctx):
    """3 001 points of one LiDAR scan of the room (floor, ceiling, four walls, boxes): the 700 nearest to the foot of the sensor -- the dense
    rings on the floor -- and 2 301 of the others; r = 1 m gives a median of ~95 neighbours and a maximum above 400"""
    pts = _room_scan(0.01)
    rng = np.random.default_rng(7)
    d = np.linalg.norm(pts - pts[np.argmin(np.linalg.norm(pts[:, :2], axis=1))], axis=1)
    near = np.argsort(d, kind="stable")[:700]
    rest = np.setdiff1d(np.arange(len(pts)), near)
    p = pts[np.sort(np.concatenate([near, rng.choice(rest, 2301, replace=False)]))].astype(np.float32)
    cloud = _device_cloud(ctx, p)
    normals = cloud.download(covs=False)[2]
    ref = R.fpfh(p, normals, 1.0)
    return {"points": p, "cloud": cloud, "normals": normals, "ref": ref, "radius": 1.0}


def test_fpfh_parity_on_a_room_scan(parity_cloud):
    ref = parity_cloud["ref"]
    k = ref["k"]
    print(f"bin margin {ref['bin_margin'].min():.3e}, swap margin {ref['swap_margin'].min():.3e}, skipped pairs {ref['skipped'].sum()}")
    assert len(k) == 3001 and 80 <= np.median(k) <= 120 and k.max() >= 400
    assert ref["bin_margin"].min() >= 1e-9 and ref["swap_margin"].min() >= 1e-9  # the condition under which the counts must agree
    f = parity_cloud["cloud"].estimate_fpfh(parity_cloud["radius"])
    assert f.size() == 3001
    got = f.download()
    _check_descriptors(got, ref)
    again = parity_cloud["cloud"].estimate_fpfh(parity_cloud["radius"]).download()
    assert got.tobytes() == again.tobytes()


def _random_cloud(rng, n, extent):
    p = rng.uniform(-extent, extent, (n, 3)).astype(np.float32)
    nr = rng.normal(size=(n, 3))
    return p, (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_fpfh_small_clouds(ctx, n):
    p, nr = _random_cloud(np.random.default_rng(100 + n), n, 1.0)
    ref = R.fpfh(p, nr, 0.9)
    assert n == 1 or (ref["bin_margin"].min() >= 1e-9 and ref["swap_margin"].min() >= 1e-9)
    f = _device_cloud(ctx, p, nr).estimate_fpfh(0.9)
    assert f.size() == n
    _check_descriptors(f.download(), ref)


def test_fpfh_every_point_sees_every_other(ctx):
    p, nr = _random_cloud(np.random.default_rng(5), 300, 1.0)
    ref = R.fpfh(p, nr, 10.0)
    assert (ref["k"] == 299).all() and ref["bin_margin"].min() >= 1e-9 and ref["swap_margin"].min() >= 1e-9
    _check_descriptors(_device_cloud(ctx, p, nr).estimate_fpfh(10.0).download(), ref)


def test_fpfh_duplicates_and_isolated_points(ctx):
    rng = np.random.default_rng(6)
    p, nr = _random_cloud(rng, 400, 1.0)
    p[350:] = p[:50]  # 50 exact duplicates (their normals differ)
    far = rng.uniform(-1, 1, (20, 3)) + 100.0 * (1 + np.arange(20))[:, None]  # 20 points 100 m from everything and from each other
    p = np.concatenate([p, far.astype(np.float32)])
    nr = np.concatenate([nr, nr[:20]])
    ref = R.fpfh(p, nr, 0.8)
    assert (ref["k"][400:] == 0).all() and ref["bin_margin"].min() >= 1e-9 and ref["swap_margin"].min() >= 1e-9
    got = _device_cloud(ctx, p, nr).estimate_fpfh(0.8).download()
    assert not got[400:].any()
    _check_descriptors(got, ref)


def test_fpfh_error_codes(ctx):
    from glim_amd import api

    p, nr = _random_cloud(np.random.default_rng(8), 100, 1.0)
    with pytest.raises(api.GlimAmdError) as e:
        api.PointCloudGPU.clone(p, ctx=ctx).estimate_fpfh(1.0)
    assert e.value.code == -5  # GLIM_AMD_ERR_STATE: no normals
    c = _device_cloud(ctx, p, nr)
    for r in (0.0, -1.0, float("nan")):
        with pytest.raises(api.GlimAmdError) as e:
            c.estimate_fpfh(r)
        assert e.value.code == -1


# ---- matching ----
@pytest.fixture(scope="module")
def crops(ctx):
    """Two overlapping crops along x of 2 000 points of a noisy (sigma = 8 cm) scan of the room: 1 537 target and 1 000 source points, 537 in
    both.  The normals are the CPU oracle's, uploaded, so that everything the gap condition depends on is decided on the CPU; r = 0.6 m.  The
    descriptors compared are the device's own (downloaded)."""
    from oracle import oracle as orc

    pts = _room_scan(0.08)
    q = pts[np.sort(np.random.default_rng(11).choice(len(pts), 2000, replace=False))].astype(np.float32)
    nq = orc.covariances(q.astype(np.float64), orc.knn(q.astype(np.float64), 10))[0][:, :3].astype(np.float32)
    order = np.argsort(q[:, 0], kind="stable")
    out = {}
    for name, idx in (("target", np.sort(order[:1537])), ("source", np.sort(order[-1000:]))):
        f = _device_cloud(ctx, q[idx], nq[idx]).estimate_fpfh(0.6)
        out[name] = (f, f.download())
    return out


def _check_match(got_idx, got_d, target, source, max_left_out):
    """the forward rule of the module docstring; returns the counted mask"""
    best, d1, d2 = R.match(target, source)
    e = R.fp32_bound(source, target[best])
    counted = (d2 - d1) > SLACK * e
    print(f"{len(source)} x {len(target)}: counted {counted.mean():.4f}, index mismatches on counted {np.sum(got_idx[counted] != best[counted])}")
    assert 1.0 - counted.mean() <= max_left_out
    assert (got_idx >= 0).all() and (got_idx < len(target)).all()
    assert np.array_equal(got_idx[counted], best[counted])
    D = R.sqdist_matrix(source, target)
    d_ret = D[np.arange(len(source)), got_idx]
    err = np.abs(got_d.astype(np.float64) - d_ret)
    bound = SLACK * R.fp32_bound(source, target[got_idx])
    print(f"max |sqdist - reference| / (50 e) = {(err / bound).max():.3e}")
    assert (err <= bound).all()
    return counted


def test_match_parity_on_two_overlapping_crops(crops):
    from glim_amd import api

    (ft, t), (fs, s) = crops["target"], crops["source"]
    assert t.shape == (1537, 33) and s.shape == (1000, 33)
    idx, d = api.match_fpfh(ft, fs)
    _check_match(idx, d, t, s, 0.05)


def test_match_reciprocal_on_two_overlapping_crops(crops):
    from glim_amd import api

    (ft, t), (fs, s) = crops["target"], crops["source"]
    idx, d = api.match_fpfh(ft, fs, reciprocal=True)
    rec, (fb, fd1, fd2), (bb, be1, be2) = R.match_reciprocal(t, s)
    okf = (fd2 - fd1) > SLACK * R.fp32_bound(s, t[fb])
    okb = (be2 - be1) > SLACK * R.fp32_bound(t, s[bb])
    counted = okf & okb[fb]  # the forward decision and the backward decision of the chosen target both pass the gap condition
    print(f"reciprocal: kept by the reference {np.mean(rec >= 0):.3f}, counted {counted.mean():.3f}, mismatches on counted {np.sum(idx[counted] != rec[counted])}")
    assert counted.mean() >= 0.5  # (the check is not vacuous; the 5 % cap is the forward test's)
    assert np.array_equal(idx[counted], rec[counted])
    fwd_idx, fwd_d = api.match_fpfh(ft, fs)
    assert np.array_equal(d, fwd_d) and ((idx == fwd_idx) | (idx == -1)).all()


def test_match_a_set_against_itself(crops):
    """A row whose nearest OTHER row is farther than 50 e must match itself, at a distance within 50 e of 0, and be reciprocal; rows with a twin
    closer than that follow the general rule (the twin with the smaller index may win)."""
    from glim_amd import api

    fs, s = crops["source"]
    idx, d = api.match_fpfh(fs, fs)
    counted = _check_match(idx, d, s, s, 0.05)
    assert np.array_equal(idx[counted], np.arange(len(s))[counted])
    assert (d[counted].astype(np.float64) <= SLACK * R.fp32_bound(s, s)[counted]).all()
    ridx, _ = api.match_fpfh(fs, fs, reciprocal=True)
    assert np.array_equal(ridx[counted], np.arange(len(s))[counted])


def test_match_odd_sizes(ctx, crops):
    from glim_amd import api

    rng = np.random.default_rng(9)
    p1, n1 = _random_cloud(rng, 1, 1.0)
    p65, n65 = _random_cloud(rng, 65, 1.0)
    f65 = _device_cloud(ctx, p65, n65).estimate_fpfh(0.9)
    f1 = _device_cloud(ctx, p1, n1).estimate_fpfh(0.9)  # one isolated point: an all-zero descriptor
    idx, d = api.match_fpfh(f1, f65)
    s = f65.download()
    assert (idx == 0).all()
    np.testing.assert_allclose(d, np.sum(s.astype(np.float64) ** 2, axis=1), rtol=0, atol=SLACK * 36.0 * 2.0 ** -24 * 3e4)
    empty = api.PointCloudGPU.clone(np.zeros((0, 3), dtype=np.float32), normals=np.zeros((0, 3), dtype=np.float32), ctx=ctx).estimate_fpfh(1.0)
    assert empty.size() == 0 and empty.download().shape == (0, 33)
    for recip in (False, True):
        idx, d = api.match_fpfh(empty, f65, reciprocal=recip)
        assert (idx == -1).all() and np.isinf(d).all()
    idx, d = api.match_fpfh(f65, empty)
    assert len(idx) == 0 and len(d) == 0
    other = api.Context(0, 1)
    g = _device_cloud(other, p65, n65).estimate_fpfh(0.9)  # (the cloud itself goes with this statement)
    try:
        with pytest.raises(api.GlimAmdError) as e:
            api.match_fpfh(g, f65)
        assert e.value.code == -1  # handles of two contexts
    finally:
        g.close()
        other.close()


def test_cpp_drop_in_and_mirror_return_the_python_values(ctx, tmp_path):
    """tests/cpp/test_fpfh.cpp calls gtsam_points::estimate_fpfh (the drop-in) and glim_amd::estimate_fpfh / match_fpfh (the mirror) on a
    500-point cloud and compares with what this process got for the same cloud."""
    from glim_amd import api
    from test_fpfh import build_cpp

    from oracle import oracle as orc

    pts = _room_scan(0.08)
    q = pts[np.sort(np.random.default_rng(13).choice(len(pts), 500, replace=False))].astype(np.float32)
    nq = orc.covariances(q.astype(np.float64), orc.knn(q.astype(np.float64), 10))[0][:, :3].astype(np.float32)
    p4 = np.ones((500, 4))
    p4[:, :3] = q
    n4 = np.zeros((500, 4))
    n4[:, :3] = nq
    f = api.PointCloudGPU.clone(p4, normals=n4, ctx=ctx).estimate_fpfh(1.2)
    desc = f.download()
    assert np.abs(desc.astype(np.float64) - R.fpfh(q, nq, 1.2)["F"]).max() <= GATE
    nearest, _ = api.match_fpfh(f, f)
    recip, _ = api.match_fpfh(f, f, reciprocal=True)
    path = tmp_path / "cloud.bin"
    with open(path, "wb") as fh:
        fh.write(struct.pack("<id", 500, 1.2))
        for a in (p4, n4, desc, nearest.astype(np.int32), recip.astype(np.int32)):
            fh.write(np.ascontiguousarray(a).tobytes())
    out = subprocess.run([build_cpp(tmp_path), str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "test_fpfh OK (500 points" in out.stdout, out.stdout + out.stderr
