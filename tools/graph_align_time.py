"""Times of the global-graph optimisation (glim_amd_graph_align) on one device, the host-driven Levenberg-Marquardt iteration beside it.

Workload: the clouds of bench.py's m2_global256 (BASELINE.json configs[3]): merged sub-maps of 4 keyframes on a grid, 1.0 m voxel maps, all
pairs i < j as binary VGICP factors -- at N = 64 (2 016 pairs) and N = 256 (32 640 pairs), the first N sub-maps of the same 256.  A prior of
precision 1e6 sits on sub-map 0, the others start a few centimetres and milliradians off.  The variants alternate in one process:
  device_loop    one glim_amd_graph_align call with max_iterations = 3: the rounds enqueued C at a time (the default chunk), the status read
                 between two chunks.  A round is the factors' row kernels and finalising blocks, then the graph's launches: items, assembly,
                 decision, load, the blocked solve (3 launches per tile column), retraction, relative poses
  host_iteration what a host-driven optimiser pays per trial over the same NonlinearFactorSetGPU: one synchronous linearize and one synchronous
                 error of the factors (NonlinearFactorSetGPU.profile_lm) -- without the host's own assembly and solve, which come on top
  factor_round   the factors' evaluation alone, enqueued back to back with the records left on the device (linearize_device_async): the part of
                 a device round that is not the graph's own launches
Recorded: wall time of the device call (p50 and min over `--iters` repeats after a warm-up), the rounds that ran (1 + trials), the wall time of
a trial round ((the call - the call with round 0 alone) / trials: no fixed part) and its split into factor_round and the rest (assembly + solve
and the launch gaps, BY DIFFERENCE: the two parts are not timed inside one run), and the call's wall time at chunk lengths 1, 2, 4, 8 and 64 with
the fastest of them; the default chunk length is measured twice, and the spread of the two is the run's noise floor.  No ratio is promised:
the tool reports what it measures.  Prints one JSON object; `--out` writes it too.

    python tools/graph_align_time.py [--iters 3] [--out profiles/graph_align/graph_align_time.json]
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
CHUNKS = (1, 2, 4, 8, 64)


def timed(fn, iters):
    """wall seconds of fn() over `iters` repeats after one warm-up, and fn's last return"""
    out, res = [], None
    for it in range(iters + 1):
        t0 = time.perf_counter()
        res = fn()
        if it:
            out.append(time.perf_counter() - t0)
    return out, res


def measure(api, torch, lmr, ctx, submaps, vmaps, N, iters):
    poses = [T for T, _ in submaps[:N]]
    clouds = [g for _, g in submaps[:N]]
    factors = [(vmaps[i], clouds[j], i, j) for j in range(N) for i in range(j)]  # source-major, as bench.py lists them
    fset = api.NonlinearFactorSetGPU(ctx)
    for vm, c, i, j in factors:
        fset.add(api.IntegratedVGICPFactorGPU(i, j, vm, c))
    rng = np.random.default_rng(N)
    X0 = [poses[0]] + [T @ lmr.expmap(rng.uniform(-1, 1, 6) * [0.005, 0.005, 0.005, 0.04, 0.04, 0.02]) for T in poses[1:]]
    priors = [(0, poses[0], 1e6 * np.eye(6))]
    Tf0 = np.stack([api.pose12(np.linalg.inv(X0[i]) @ X0[j]) for _, _, i, j in factors])
    nf = len(factors)
    records = torch.zeros(nf, api._lib.COMPACT_DOUBLES, dtype=torch.float64, device="cuda")
    prm, prm_zero = api.graph_align_params(max_iterations=3), api.graph_align_params(max_iterations=0)
    out = {"poses": N, "factors": nf, "rows": 6 * N, "points_per_cloud": int(np.mean([c.size() for c in clouds])), "rounds_budget": 1 + prm.resolved_max_trials()}

    def call(p, chunk=0):
        ctx.synchronize()
        return api.graph_align_debug_trace(factors, priors, [], X0, 0, p, ctx=ctx, trace=False, rounds_per_chunk=chunk)[0]

    wall, res = timed(lambda: call(prm), iters)
    zero, _ = timed(lambda: call(prm_zero), iters)
    host_lin, host_err, factor_round = [], [], []
    for _ in range(iters):
        lin_ms, err_ms = fset.profile_lm(Tf0, iters=5)
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            fset.linearize_device_async(Tf0, records.data_ptr(), 0)
        ctx.synchronize()
        torch.cuda.synchronize()
        factor_round.append((time.perf_counter() - t0) / 5)
        host_lin.append(lin_ms)
        host_err.append(err_ms)
    ran = 1 + res.trials
    w, wz, fr = float(np.median(wall)), float(np.median(zero)), float(np.median(factor_round))
    out["device_loop"] = {"wall_ms_p50": w * 1e3, "wall_ms_min": float(min(wall)) * 1e3, "rounds_that_ran": ran, "iterations": res.iterations, "trials": res.trials,
                          "status": res.status_name, "cost": res.cost, "num_inliers": res.num_inliers,
                          "max_distance_to_the_true_poses": float(np.abs(res.poses - np.stack(poses)).max()),
                          "start_distance_to_the_true_poses": float(np.abs(np.stack(X0) - np.stack(poses)).max())}
    out["device_loop_round_0_only"] = {"wall_ms_p50": wz * 1e3, "wall_ms_min": float(min(zero)) * 1e3,
                                       "note": "the call's fixed part (arguments, lists, the transient plan of the pairs, uploads) plus one evaluation and one decision"}
    lm_ms = float(np.median(np.array(host_lin) + np.array(host_err)))
    out["host_iteration"] = {"sync_linearize_ms_p50": float(np.median(host_lin)), "sync_error_ms_p50": float(np.median(host_err)), "lm_iteration_ms_p50": lm_ms}
    if res.trials:
        trial = (w - wz) / res.trials
        out["round_split"] = {"trial_round_ms": trial * 1e3, "factor_round_ms_p50": fr * 1e3, "assembly_and_solve_ms_by_difference": (trial - fr) * 1e3,
                              "host_lm_iteration_ms": lm_ms,
                              "note": "trial_round = (the call - round 0 only) / trials; the rest is the graph's own launches and the gaps between launches, with "
                                      "the chunk's status read; the parts are not timed inside one run"}
    chunks = {}
    for c in CHUNKS:
        t, r = timed(lambda: call(prm, c), iters)
        assert np.array_equal(r.poses, res.poses) and (r.status, r.trials) == (res.status, res.trials)  # the chunk length moves no bit
        chunks[str(c)] = {"wall_ms_p50": float(np.median(t)) * 1e3, "wall_ms_min": float(min(t)) * 1e3}
    out["chunk_length"] = chunks
    out["fastest_chunk_length"] = int(min(chunks, key=lambda k: chunks[k]["wall_ms_p50"]))
    # the default chunk length is in the table too: the same call measured twice in one process, seconds apart -- the run's own noise floor
    twice = [w * 1e3, chunks["4"]["wall_ms_p50"]]
    out["same_call_measured_twice"] = {"wall_ms_p50": twice, "spread": abs(twice[0] - twice[1]) / min(twice),
                                       "note": "device_loop and chunk_length['4'] are the same configuration; differences below this spread, the chunk "
                                               "lengths' among them, are not findings of this run"}
    if res.trials:
        out["round_split"]["trial_round_ms_from_the_second_measurement"] = (twice[1] - wz * 1e3) / res.trials
    fset.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    import bench
    import lm_restatement as lmr
    from glim_amd import api

    ctx = api.Context(0, 1)
    t0 = time.time()
    submaps = bench.make_merged_submaps(api, ctx, max(args.sizes), 4, 40, 560)  # bench.py's defaults for global256
    vmaps = [api.GaussianVoxelMapGPU(1.0, ctx=ctx).insert(g) for _, g in submaps]
    out = {"what": __doc__.split("\n")[0], "iters": args.iters, "repeated": "one box, not repeated", "device": ctx.device_info(),
           "default_chunk_length": "GRAPH_ROUNDS_PER_CHUNK of glim_amd/csrc/bundle_align.hip (rounds_per_chunk = 0)", "scene_seconds": time.time() - t0, "sizes": {}}
    for N in args.sizes:
        out["sizes"][str(N)] = measure(api, torch, lmr, ctx, submaps, vmaps, N, args.iters)
        print(f"N = {N} done", file=sys.stderr, flush=True)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
