"""NumPy restatement of the scan-to-keyframes VGICP registration (glim_amd/csrc/keyframe_lm_step.hpp, include/glim_amd.h "Scan-to-keyframes
VGICP registration"): one pose X over M unary factors with fixed target poses P_f, an optional prior on X.  Factor f is evaluated at
T_f = P_f^-1 X; the 29 entries of the factors' compact records are summed one factor at a time from +0.0, the prior's contribution is added
last, and the rule is lm_restatement's, unchanged, on the summed record.  A plain module: it holds no tests.

A factor is (linearize, P): linearize(T) -> a record (num_inliers, error, H_ss, b_s) as the oracle returns it.  A prior is (P, information)."""
import numpy as np

import bundle_lm_restatement as blr
import lm_restatement as lmr

PRIOR = 28
TRIU = np.triu_indices(6)


def sum_compact(compacts):
    """((+0.0 + c_0) + c_1) + ...: each of the 29 entries on its own, ascending"""
    s = np.zeros(29)
    for c in compacts:
        s = s + np.asarray(c, dtype=np.float64)
    return s


def prior_contribution(X, prior):
    """the 21 upper entries of J^T L J, the 6 of J^T L r, then r^T L r (bundle_lm_restatement.prior_term)"""
    H, b, c = blr.prior_term(np.asarray(X, dtype=np.float64), np.asarray(prior[0], dtype=np.float64), prior[1])
    return np.concatenate([H[TRIU], b, [c]])


def add_prior(compact, c):
    """to H, b and the error; never to the inlier count"""
    out = np.array(compact, dtype=np.float64)
    out[1] = out[1] + c[27]
    out[2:29] = out[2:29] + c[:27]
    return out


def factor_poses(Ps, X):
    return [np.linalg.inv(P) @ X for P in Ps]


def evaluate(factors, X, prior=None):
    """-> (the summed record as a dict, its compact form, the factors' compact records, the T_f, the prior's contribution)"""
    Tf = factor_poses([P for _, P in factors], X)
    compacts = [lmr.compact_of_record(lin(T)) for (lin, _), T in zip(factors, Tf)]
    pc = prior_contribution(X, prior) if prior is not None else np.zeros(PRIOR)
    total = sum_compact(compacts)
    if prior is not None:
        total = add_prior(total, pc)
    rec = lmr.record_of_compact(total) if np.all(np.isfinite(total)) else {"num_inliers": 0, "error": float("nan"), "H_ss": np.full((6, 6), np.nan), "b_s": np.full(6, np.nan)}
    return rec, total, compacts, Tf, pc


RESOLUTIONS = (0.5, 1.0)
REJECT_PERT = [0.114, 0.029, -0.095, 0.624, 0.125, -0.339]
_SCANS = {}


def scans(size, n=3):
    """the scans of synth.arc_trajectory(n, step=0.6, yaw_step_deg=3.0) at a size (rings, az) -> (world poses, points per scan), built once"""
    from glim_amd import synth

    if (size, n) not in _SCANS:
        world, dirs = synth.Scene.default(), synth.lidar_directions(*size)
        poses = synth.arc_trajectory(n, step=0.6, yaw_step_deg=3.0)
        _SCANS[(size, n)] = (poses, [synth.scan(world, T, dirs, frame_id=i).astype(np.float64) for i, T in enumerate(poses)])
    return _SCANS[(size, n)]


def oracle_factors(orc, clouds, keyframes, source, poses, resolutions=RESOLUTIONS):
    """the scene of the tests: the keyframes' scans at their world poses, a map per resolution each (keyframe-major), the source scan.
    clouds: (points, covariances) per scan -> the factors of run()"""
    sp, sc = clouds[source]
    factors = []
    for k in keyframes:
        for res in resolutions:
            ref_map = orc.VoxelMap(res).insert(*clouds[k])
            factors.append((lambda T, m=ref_map: orc.vgicp_linearize(m, sp, sc, T), poses[k]))
    return factors


def run(factors, X_init, p=None, prior=None):
    """lm_restatement.run on the summed record -> (final state, trace); a trace entry also holds `compact` (the summed record's 29 doubles),
    `factor_compact` (M x 29), `Tf` (M poses) and `prior` (28)"""
    seen = []

    def linearize(X):
        rec, total, compacts, Tf, pc = evaluate(factors, X, prior)
        seen.append({"compact": total, "factor_compact": np.stack(compacts), "Tf": Tf, "prior": pc})
        return rec

    s, trace = lmr.run(linearize, X_init, p)
    for e, extra in zip(trace, seen):
        e.update(extra)
    return s, trace
