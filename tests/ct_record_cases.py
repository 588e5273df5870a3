"""The cases of the continuous-time record tests (tests/test_record_slots_ct.py on the CPU, tests/test_gpu_ct_record_slots.py on the device): which
points, which times, which begin and end poses.  A plain module: it holds no tests.

The target is ct_restatement.static_map(16, 512); the source is the first n points of ct_restatement.moving_source(16, 256) (4096 points) with
times handed to the factor, piecewise constant and stepping by 2e-3 where the case sets the bucket sizes."""
import numpy as np

import ct_restatement as ctg

STEP = 2e-3
TAILS = [1, 63, 64, 65, 255, 256, 257, 513, 1]  # one lane, a wavefront's edge, a block's edge, two and three blocks, a last block of one point
NBK = [1, 7, 8, 9, 63, 64, 65, 73]              # ordered_column_sum: each group's first row, a full trip of 64, the first row of a second trip
FAR_BUCKET = 4                                   # the bucket of TAILS (255 points) that the "empty bucket" case moves 1e3 m away
FAR = np.array([1e3, 0.0, 0.0])


def stepped(sizes):
    return np.repeat(np.arange(len(sizes)) * STEP, sizes)


def poses():
    """(X, Y): the begin and end poses of test_ct_factor_edge_cases, a few millimetres and milliradians off the sweep's own"""
    T0, T1 = ctg.sweep_poses()
    return T0 @ ctg.expmap([0.001, 0.0, 0.002, 0.02, 0.01, 0.0]), T1 @ ctg.expmap([0.0, -0.001, 0.0, 0.0, 0.02, -0.01])


def moved(X, Y):
    """the evaluation poses of test_ct_factor_matches_the_restatement_on_a_moving_scan"""
    return X @ ctg.expmap([0.001, 0.0, -0.001, 0.01, 0.0, 0.01]), Y @ ctg.expmap([0.0, 0.002, 0.0, -0.01, 0.02, 0.0])


def cases():
    """name -> dict(n, times, X, Y, far, pre): far is the index range of the points moved by FAR, or None; pre is a pose the source is moved by
    before it is uploaded (points and covariances), or None"""
    X, Y = poses()
    _, t = ctg.moving_source(16, 256)
    slow = X @ ctg.expmap(0.1 * ctg.logmap(np.linalg.inv(X) @ Y))
    assert np.linalg.norm(ctg.logmap(np.linalg.inv(X) @ Y)[:3]) > ctg.SERIES > np.linalg.norm(ctg.logmap(np.linalg.inv(X) @ slow)[:3]) > 0
    tails = stepped(TAILS)
    out = {"tails": dict(n=len(tails), times=tails, X=X, Y=Y, far=None)}
    for k in NBK:
        out[f"nbk{k}"] = dict(n=3 * k, times=stepped([3] * k), X=X, Y=Y, far=None)
    out["sweep"] = dict(n=len(t), times=np.asarray(t, dtype=np.float64), X=X, Y=Y, far=None)  # |omega| above SERIES: the closed forms
    out["slow"] = dict(n=len(tails), times=tails, X=X, Y=slow, far=None)                      # below it: the series
    out["equal"] = dict(n=len(tails), times=tails, X=X, Y=X.copy(), far=None)
    a = int(np.sum(TAILS[:FAR_BUCKET]))
    out["empty-bucket"] = dict(n=len(tails), times=tails, X=X, Y=Y, far=(a, a + TAILS[FAR_BUCKET]))
    rng = np.random.default_rng(3)
    out["non-ascending"] = dict(n=1000, times=np.asarray(t[:1000], dtype=np.float64)[rng.permutation(1000)], X=X, Y=Y, far=None)
    for c in out.values():
        c["pre"] = None
    # a scan that barely rotates: the source already in the world frame (moved by X), begin and end poses a milliradian and a few millimetres
    # from the identity.  R_k is then so near I that a kept metric left in the source frame changes the frozen error by 1e-4 of itself
    Xr = ctg.expmap(1e-3 * np.array([0.3, -0.5, 0.8, 2.0, -1.0, 1.5]))
    out["registered"] = dict(n=len(tails), times=tails, X=Xr, Y=Xr @ ctg.expmap(1e-3 * np.array([-0.4, 0.2, 1.0, 3.0, 2.0, -1.0])), far=None, pre=X)
    return out


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def source_points(case, p):
    """the case's source points from the scan's (FP32 values in and out)"""
    sp = _f32(p)[: case["n"]].copy()
    if case["far"] is not None:
        sp[case["far"][0] : case["far"][1]] += FAR
    if case["pre"] is not None:
        sp = sp @ case["pre"][:3, :3].T + case["pre"][:3, 3]
    return _f32(sp)


def source_covs(case, covs):
    sc = _f32(covs)[: case["n"]]
    if case["pre"] is not None:
        sc = case["pre"][:3, :3] @ sc @ case["pre"][:3, :3].T
    return _f32(sc)


def scene(case, tp, tc, p, covs):
    """the record_slots scene of a case.  tp, tc: the target's points and covariances; p, covs: the 4096 points of the scan and their
    covariances (a covariance does not change when its point is moved by FAR); every array holding FP32 values"""
    return dict(tp=_f32(tp), tc=_f32(tc), sp=source_points(case, p), sc=source_covs(case, covs))
