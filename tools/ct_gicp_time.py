"""Wall time of the continuous-time GICP factor on the device (glim_amd_ct_gicp_*), next to the rigid GICP factor on the same clouds.

GLIM's LiDAR-only CT odometry (odometry_estimation_ct.cpp:158-183) linearises one IntegratedCT_GICPFactor up to 8 times per frame.  Workload:
a 0.1 s sweep of a moving sensor (~1 m, 5 deg; ~100 time buckets) against a static 131 072-point map; sources of ~10 000 points (the shipped
preprocessing) and of 131 072 points.  Per source: CT linearize, CT error (kept correspondences), glim_amd_gicp_linearize at the scan-begin
pose, and one 8-iteration Gauss-Newton frame of the CT factor (linearize + error per iteration).  Prints one JSON object; `--out` writes it too.

    python tools/ct_gicp_time.py [--iters 200] [--out profiles/ct_gicp/ct_gicp_time.json]
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


def timed(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    t = np.array(t)
    return {"p50_us": round(float(np.median(t)), 1), "p10_us": round(float(np.percentile(t, 10)), 1), "p90_us": round(float(np.percentile(t, 90)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from glim_amd import api
    import ct_restatement as W  # the workload builders of the parity tests (static map, moving sweep)

    ctx = api.Context(0, 1)
    tp = W.static_map(64, 1024)
    tg = api.PointCloudGPU.clone(tp, ctx=ctx)
    tg.find_neighbors(10, download=False)
    tg.estimate_covariances(10)
    T0, T1 = W.sweep_poses()
    X = T0 @ W.expmap([0.002, -0.001, 0.003, 0.03, -0.02, 0.01])
    Y = T1 @ W.expmap([-0.001, 0.002, -0.002, 0.02, 0.03, -0.01])
    values = {0: X, 1: Y}
    res = {"target_points": int(tg.size()), "iters": args.iters, "sources": {}}
    for kind in ("pre10k", "raw131k"):
        _, _, times, pass_times, sg = W._source(api, ctx, kind)
        f = api.IntegratedCT_GICPFactor(0, 1, tg, sg, max_correspondence_distance=1.0, times=pass_times)
        g = api.IntegratedGICPFactor(np.eye(4), 1, tg, sg, target_tree=f.target_tree, max_correspondence_distance=1.0)
        nb = len(f.debug_poses(values)[0])
        f.linearize(values)
        r = {"source_points": int(sg.size()), "buckets": nb}
        r["ct_linearize"] = timed(lambda: f.linearize(values), args.iters)
        r["ct_error"] = timed(lambda: f.error(values), args.iters)
        r["gicp_linearize"] = timed(lambda: g.linearize({1: X}), args.iters)

        def frame():
            Xi, Yi = X.copy(), Y.copy()
            for _ in range(8):
                L = f.linearize({0: Xi, 1: Yi})
                H, b = W.full_system(L)
                dx = np.linalg.solve(H + 1e-6 * np.trace(H) / 12 * np.eye(12), -b)
                Xi, Yi = Xi @ W.expmap(dx[:6]), Yi @ W.expmap(dx[6:])
                f.error({0: Xi, 1: Yi})

        r["lm_frame_8_iterations"] = timed(frame, max(10, args.iters // 10), warmup=2)
        r["ct_over_gicp_linearize"] = round(r["ct_linearize"]["p50_us"] / r["gicp_linearize"]["p50_us"], 3)
        res["sources"][kind] = r
        g.close()
        f.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
