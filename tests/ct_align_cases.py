"""The scenes and cases of the CT-GICP frame alignment tests (tests/test_ct_align.py on the CPU, tests/test_ct_align_gpu.py on the device): the
scenes of tests/ct_restatement.py -- target static_map(16, 512), 16 384 points; source moving_source(16, 256) -- and four starts found with the
FP64 oracle driven through tests/ct_lm_restatement.py with GLIM's CT parameters.  The source cut to its first 4001 points gives some 85 buckets, a last
block that is not full and many blocks per launch; the GLIM-form cases use all 4096.  A plain module: it holds no tests."""
import numpy as np

from ct_lm_restatement import terms
from ct_restatement import expmap, logmap, moving_source, static_map, sweep_poses

#        f: the fraction of the true sweep motion the constant-velocity prediction carries; between: the measurement ('pred' = that prediction,
#        'identity' = GLIM's form) and its precision.  The location prior is (X_pred, 1e-3) in every case.
CASES = {
    "A": dict(points=4001, f=0.7, max_dist=1.0, between=("pred", 1e3)),   # trials: 0.94, 0.023 of the cost, then every trial rejected up to MAX_TRIALS
    "B": dict(points=4001, f=0.4, max_dist=2.0, between=("pred", 1e3)),   # 0.97, 0.066
    "C": dict(points=4096, f=0.7, max_dist=1.0, between=("identity", 1e3)),   # accept x 3 (0.875, 0.0147, 2.6e-4), 13 rejections at -1.1e-6: MAX_TRIALS
    "D": dict(points=4096, f=0.7, max_dist=1.0, between=("identity", 1e-3)),  # 5 accepted trials: CONVERGED
}
LOCATION_PRECISION = 1e-3


def case_inputs(name):
    """-> (X start, Y start, terms, max_correspondence_distance)"""
    c = CASES[name]
    T0, T1 = sweep_poses()
    X_pred = T0 @ expmap([0.0, 0.0, 0.004, 0.03, -0.02, 0.0])
    delta_pred = expmap(c["f"] * logmap(np.linalg.inv(T0) @ T1))
    kind, kb = c["between"]
    D = delta_pred if kind == "pred" else np.eye(4)
    return X_pred.copy(), X_pred @ delta_pred, terms((X_pred, LOCATION_PRECISION), (D, kb)), c["max_dist"]


def pose_table_cases():
    """the four inputs of the pose table checks (also tests/test_ct_align_gpu.py): name -> (table or None = the scene's own, X, Y)"""
    T0, T1 = sweep_poses()
    small = T0 @ expmap([0.004, -0.003, 0.006, 0.3, -0.1, 0.02])  # a relative rotation of 0.0078 rad: the series branch
    return {"sweep": (None, T0, T1), "equal": (None, T0, T0.copy()), "series": (None, T0, small), "one entry": (np.array([0.0]), T0, T1)}


_cpu = {}


def cpu_scene(orc, points):
    """(tp, tc, sp, sc, times) with the oracle's covariances (of the cut cloud, as a device cloud of the cut points has them); computed once"""
    if "target" not in _cpu:
        tp = static_map(16, 512)
        _cpu["target"] = (tp, orc.covariances(tp, orc.knn(tp, 10))[1])
        _cpu["source"] = moving_source(16, 256)
    if points not in _cpu:
        p, t = _cpu["source"]
        sp = p[:points]
        _cpu[points] = (sp, orc.covariances(sp, orc.knn(sp, 10))[1], t[:points])
    return _cpu["target"] + _cpu[points]
