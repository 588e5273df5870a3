"""Times of the sub-map bundle optimisation (glim_amd_bundle_align) on one device, the host-driven Levenberg-Marquardt iteration beside it.

Workload: the bundle of bench.py --workload submap20 (BASELINE.json configs[2]): 20 keyframes x 65 536 directions on the arc, all 190 pairs x 2
voxel levels (0.25 / 0.5 m) = 380 binary VGICP factors, a prior of precision 1e6 on keyframe 0 (sub_mapping.cpp:186), the other keyframes
started a few centimetres and milliradians off.  The variants alternate in one process:
  device_loop    one glim_amd_bundle_align call: 1 + max_trials rounds enqueued, ONE host synchronisation.  A round is the 380 factors' row kernels
                 and finalising blocks plus the bundle decide kernel (expansion, 120 x 120 assembly, Cholesky in LDS, retraction, relative poses)
  host_iteration what a host-driven optimiser pays per trial over the same NonlinearFactorSetGPU: one synchronous linearize and one synchronous
                 error of the 380 factors (NonlinearFactorSetGPU.profile_lm: what bench.py reports as lm_iteration_ms) -- without the host's own
                 assembly and solve, which come on top
  factor_round   the 380 factors' evaluation alone, enqueued back to back with the records left on the device (linearize_device_async, what
                 bench.py reports as bundle_linearize_ms): the part of a device round that is not the decide kernel
Recorded: wall time of the device call (p50 and min over `--iters` repeats after a warm-up), the rounds that ran (1 + trials), the wall time per
round that ran, and the split of a round into factor_round and the rest (the decide kernel and the launch gaps, BY DIFFERENCE: the two parts are
not timed inside one run).  Rounds after the problem has finished cost a status load per block; they are inside the wall time.  No ratio is
promised: the tool reports what it measures.  Prints one JSON object; `--out` writes it too.

    python tools/bundle_align_time.py [--iters 5] [--out profiles/bundle_align/bundle_align_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--keyframes", type=int, default=20)
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--azimuths", type=int, default=1024)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    import lm_restatement as lmr
    from glim_amd import api, synth

    ctx = api.Context(0, 1)
    K, levels = args.keyframes, (0.25, 0.5)
    scene = synth.Scene.default()
    dirs = synth.lidar_directions(args.rings, args.azimuths)
    poses = synth.arc_trajectory(K, step=0.5, yaw_step_deg=1.5)
    clouds = []
    for i, T in enumerate(poses):
        g = api.PointCloudGPU.clone(synth.scan(scene, T, dirs, frame_id=i), ctx=ctx)
        g.find_neighbors(10, download=False)
        g.estimate_covariances(10)
        clouds.append(g)
    vmaps = [[api.GaussianVoxelMapGPU(r, ctx=ctx).insert(c) for r in levels] for c in clouds]
    factors = [(vmaps[i][lv], clouds[j], i, j) for i in range(K) for j in range(i + 1, K) for lv in range(len(levels))]
    fset = api.NonlinearFactorSetGPU(ctx)
    for vm, c, i, j in factors:
        fset.add(api.IntegratedVGICPFactorGPU(i, j, vm, c))
    rng = np.random.default_rng(20)
    X0 = [poses[0]] + [T @ lmr.expmap(rng.uniform(-1, 1, 6) * [0.005, 0.005, 0.005, 0.04, 0.04, 0.02]) for T in poses[1:]]
    priors = [(0, poses[0], 1e6 * np.eye(6))]
    Tf0 = np.stack([api.pose12(np.linalg.inv(X0[i]) @ X0[j]) for _, _, i, j in factors])
    nf = len(factors)
    records = torch.zeros(nf, api._lib.COMPACT_DOUBLES, dtype=torch.float64, device="cuda")
    prm = api.bundle_align_params()
    out = {"what": __doc__.split("\n")[0], "iters": args.iters, "repeated": "one box, not repeated", "device": ctx.device_info(), "keyframes": K, "factors": nf,
           "points_per_cloud": int(np.mean([c.size() for c in clouds])), "rounds_enqueued": 1 + prm.resolved_max_trials()}
    wall, host_lin, host_err, factor_round = [], [], [], []
    res = None
    for it in range(args.iters + 1):  # the first round is the warm-up
        ctx.synchronize()
        t0 = time.perf_counter()
        res = api.bundle_align(factors, priors, [], X0, 0, prm, ctx=ctx)
        t1 = time.perf_counter()
        lin_ms, err_ms = fset.profile_lm(Tf0, iters=20)
        ctx.synchronize()
        t2 = time.perf_counter()
        for _ in range(20):
            fset.linearize_device_async(Tf0, records.data_ptr(), 0)
        ctx.synchronize()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if it:
            wall.append(t1 - t0)
            host_lin.append(lin_ms)
            host_err.append(err_ms)
            factor_round.append((t3 - t2) / 20)
    ran = 1 + res.trials
    # the same problem with exactly the rounds it needs enqueued (max_trials = the trials it took): what the 1 + max_trials - ran rounds that find
    # the problem finished cost is the difference to the call above
    exact, prm_exact = [], api.bundle_align_params(max_trials=max(1, res.trials))
    for it in range(args.iters + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        res_exact = api.bundle_align(factors, priors, [], X0, 0, prm_exact, ctx=ctx)
        if it:
            exact.append(time.perf_counter() - t0)
    assert np.array_equal(res_exact.poses, res.poses)
    we = float(np.median(exact))
    out["device_loop_exact_budget"] = {"rounds_enqueued": 1 + prm_exact.resolved_max_trials(), "wall_ms_p50": we * 1e3, "wall_ms_min": float(min(exact)) * 1e3,
                                       "wall_us_per_round": we * 1e6 / (1 + prm_exact.resolved_max_trials()),
                                       "note": "includes the call's fixed part: the arguments, the transient plan of the 380 pairs, the uploads"}
    # and with round 0 alone (max_iterations = 0): the fixed part plus one evaluation and one decide step that solves nothing
    zero, prm_zero = [], api.bundle_align_params(max_iterations=0)
    for it in range(args.iters + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        api.bundle_align(factors, priors, [], X0, 0, prm_zero, ctx=ctx)
        if it:
            zero.append(time.perf_counter() - t0)
    wz = float(np.median(zero))
    out["device_loop_round_0_only"] = {"rounds_enqueued": 1, "wall_ms_p50": wz * 1e3, "wall_ms_min": float(min(zero)) * 1e3}
    if res.trials:
        out["device_loop_exact_budget"]["wall_us_per_trial_round_beyond_round_0"] = (we - wz) * 1e6 / res.trials
    w = float(np.median(wall))
    per_round = w / ran
    fr = float(np.median(factor_round))
    out["device_loop"] = {"wall_ms_p50": w * 1e3, "wall_ms_min": float(min(wall)) * 1e3, "rounds_that_ran": ran, "iterations": res.iterations, "trials": res.trials,
                          "status": res.status_name, "cost": res.cost, "num_inliers": res.num_inliers, "wall_us_per_round_that_ran": per_round * 1e6,
                          "max_distance_to_the_true_poses": float(np.abs(res.poses - np.stack(poses)).max()),
                          "start_distance_to_the_true_poses": float(np.abs(np.stack(X0) - np.stack(poses)).max())}
    out["host_iteration"] = {"sync_linearize_ms_p50": float(np.median(host_lin)), "sync_error_ms_p50": float(np.median(host_err)),
                             "lm_iteration_ms_p50": float(np.median(np.array(host_lin) + np.array(host_err))),
                             "for_the_same_rounds_ms": float(np.median(np.array(host_lin) + np.array(host_err))) * ran}
    clean = out["device_loop_exact_budget"].get("wall_us_per_trial_round_beyond_round_0", per_round * 1e6)
    out["round_split"] = {"trial_round_us": clean, "factor_round_us_p50": fr * 1e6, "rest_of_a_round_us_by_difference": clean - fr * 1e6,
                          "note": "trial_round = (exact budget - round 0 only) / trials: no fixed part, no finished rounds; rest = the decide kernel and "
                                  "the launch gaps; the two parts are not timed inside one run"}
    fset.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
