"""Wall time of the on-device CT-GICP frame alignment (glim_amd_ct_align) against the host-driven loop it replaces.

GLIM's LiDAR-only CT odometry (odometry_estimation_ct.cpp:158-195) optimises the sweep's begin and end pose once per frame, up to 8
Levenberg-Marquardt iterations.  Workload: tools/ct_gicp_time.py's -- a 0.1 s sweep of a moving sensor (~1 m, 5 deg) through the shipped
preprocessing (~10 000 points, "pre10k") against a static 131 072-point map, as a search index and as a device iVox in neighbour mode 1 -- from
the constant-velocity prediction of a frame that moved 30 % slower.  Two variants on the same factor and clouds, alternating in one process:

    host_loop    the 8-iteration loop of tools/ct_gicp_time.py (`lm_frame_8_iterations`): one synchronous linearize and one error per iteration,
                 the 12 x 12 solve in NumPy
    device       IntegratedCT_GICPFactor.align with GLIM's parameters and its two terms (location 1e-3, between identity 1e3): every round
                 enqueued up front, one synchronisation.  `rounds` = the evaluations it ran (1 + trials)

Prints one JSON object; `--out` writes it too.

    python tools/ct_align_time.py [--iters 100] [--out profiles/ct_align/ct_align_time.json]
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


def stats(t):
    t = np.array(t)
    return {"p50_us": round(float(np.median(t)), 1), "p10_us": round(float(np.percentile(t, 10)), 1), "p90_us": round(float(np.percentile(t, 90)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from glim_amd import api
    import ct_restatement as W  # the workload builders of the parity tests (static map, moving sweep)

    ctx = api.Context(0, 1)
    tg = api.PointCloudGPU.clone(W.static_map(64, 1024), ctx=ctx)
    tg.find_neighbors(10, download=False)
    tg.estimate_covariances(10)
    ivox = api.IncrementalVoxelMap(1.0, ctx=ctx)
    ivox.voxel_insertion_setting(min_dist=0.05, max_points=20)
    ivox.set_neighbor_voxel_mode(1)
    ivox.insert(tg)
    _, _, _, pass_times, sg = W._source(api, ctx, "pre10k")
    T0, T1 = W.sweep_poses()
    X0 = T0 @ W.expmap([0.0, 0.0, 0.004, 0.03, -0.02, 0.0])
    Y0 = X0 @ W.expmap(0.7 * W.logmap(np.linalg.inv(T0) @ T1))
    values = {0: X0, 1: Y0}
    terms = dict(location_prior=(X0, 1e-3), between=(np.eye(4), 1e3))
    res = {"target_points": int(tg.size()), "source_points": int(sg.size()), "iters": args.iters, "targets": {}}
    for name, target in (("index", tg), ("ivox_mode1", ivox)):
        f = api.IntegratedCT_GICPFactor(0, 1, target, sg, max_correspondence_distance=1.0, times=pass_times)

        def host_loop():
            Xi, Yi = X0.copy(), Y0.copy()
            for _ in range(8):
                L = f.linearize({0: Xi, 1: Yi})
                H, b = W.full_system(L)
                dx = np.linalg.solve(H + 1e-6 * np.trace(H) / 12 * np.eye(12), -b)
                Xi, Yi = Xi @ W.expmap(dx[:6]), Yi @ W.expmap(dx[6:])
                f.error({0: Xi, 1: Yi})

        def device():
            return f.align(values, **terms)

        for _ in range(3):
            host_loop()
            device()
        t_host, t_dev = [], []
        for _ in range(args.iters):  # alternating: both variants see the same clocks and the same neighbours on the box
            t0 = time.perf_counter()
            host_loop()
            t1 = time.perf_counter()
            r = device()
            t2 = time.perf_counter()
            t_host.append((t1 - t0) * 1e6)
            t_dev.append((t2 - t1) * 1e6)
        row = {"buckets": len(f.debug_poses(values)[0]), "host_loop": stats(t_host), "device": stats(t_dev), "rounds": r.trials + 1, "iterations": r.iterations,
               "status": r.status_name}
        row["device_per_round_us"] = round(row["device"]["p50_us"] / row["rounds"], 1)
        row["host_over_device"] = round(row["host_loop"]["p50_us"] / row["device"]["p50_us"], 2)
        res["targets"][name] = row
        f.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
