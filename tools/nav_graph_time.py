"""Times of the graph optimiser over pose, velocity and bias nodes (glim_amd_graph_align_nav) on one device.

Workloads (tests/nav_graph_restatement.py's scenes, the default parameters):
  submap20        the sub-mapping-shaped graph over 20 frames (sub_mapping.cpp:183-243 with enable_imu): 60 nodes X, V, B per frame, 360 rows; a
                  pose prior, the between chain, 40 vector priors, 19 bias betweens, 18 IMU terms and one velocity between.  Terms only, and
                  with the 37 VGICP factors (i, j), 0 < j - i <= 2, over sub-maps of bench.py's m2_global256 clouds at the frames' poses.
  global36        the global-mapping-shaped graph over 36 sub-maps (global_mapping.cpp:162-216 with enable_imu): 252 nodes X, two E, two V, two
                  B per sub-map, 1512 rows; terms only.
Recorded per variant: wall time of the call (p50 and min over `--iters` repeats after a warm-up), the rounds that ran, the status, the cost and
its parts, the distance of the result from the scene's truth.  No ratio is promised: the tool reports what it measures.

  --against ROOT   tools/graph_terms_time.py's timing condition for this change: the round time of graph_align WITHOUT new terms at N = 64 in
                   this tree and in the tree at ROOT (a built checkout of the parent commit), alternating, two processes each.

    python tools/nav_graph_time.py [--iters 5] [--against ../parent] [--out profiles/nav_graph/nav_graph_time.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
PERT = [0.01, -0.01, 0.01, 0.08, -0.05, 0.03]  # tests/align_cases.py's PERT_A


def timed(fn, iters):
    times, res = [], fn()  # (a warm-up)
    for _ in range(iters):
        t0 = time.perf_counter()
        res = fn()
        times.append(time.perf_counter() - t0)
    return times, res


def run(api, nr, ctx, sc, factors, iters):
    g = sc["g"]
    vp, vb, im = nr.api_terms(g)
    nodes = nr.api_nodes(sc["kinds"], sc["X0"])

    def call():
        ctx.synchronize()
        return api.graph_align_nav(factors, g["priors"], g["betweens"], nodes, sc["kinds"], vp, vb, im, g["dampings"], ctx=ctx)

    times, res = timed(call, iters)
    return {"nodes": g["N"], "rows": 6 * g["N"], "factors": len(factors), "pose_priors": len(g["priors"]), "pose_betweens": len(g["betweens"]),
            "vector_priors": len(vp), "vector_betweens": len(vb), "imu_terms": len(im), "dampings": len(g["dampings"]),
            "wall_ms_p50": float(np.median(times)) * 1e3, "wall_ms_min": float(min(times)) * 1e3, "rounds_that_ran": 1 + res.trials,
            "round_ms": float(np.median(times)) * 1e3 / (1 + res.trials), "iterations": res.iterations, "status": res.status_name, "cost": res.cost,
            "cost_parts": {"factor": res.factor_cost, "prior": res.prior_cost, "between": res.between_cost, "vector_prior": res.vector_prior_cost,
                           "vector_between": res.vector_between_cost, "imu": res.imu_cost},
            "max_distance_to_the_truth": nr.node_error(sc["kinds"], res.values12, sc["truth"]),
            "max_distance_of_the_initial_values": nr.node_error(sc["kinds"], sc["X0"], sc["truth"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--against", default="", help="a built checkout of the parent commit")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out = {"what": __doc__.split("\n")[0], "iters": args.iters, "repeated": "one box, one run"}
    if args.against:  # first, in processes of their own: this process has not opened the device yet
        from graph_terms_time import round_time_against

        out["graph_align_round_time_n64"] = round_time_against(args.against, args.iters)
    import nav_graph_restatement as nr
    from glim_amd import api

    import bench

    ctx = api.Context(0, 1)
    out["device"] = ctx.device_info()
    K = 20
    submaps = bench.make_merged_submaps(api, ctx, K, 4, 40, 560)  # bench.py's defaults for global256
    vmaps = [api.GaussianVoxelMapGPU(1.0, ctx=ctx).insert(c) for _, c in submaps]
    pairs = [(i, j) for i in range(K) for j in range(i + 1, min(i + 3, K))]
    sc = nr.submap_scene(K, PERT, poses=np.stack([T for T, _ in submaps]), pairs=pairs)
    terms_only = dict(sc, g=dict(sc["g"], factors=[]))
    out["submap20"] = {"terms_only": run(api, nr, ctx, terms_only, [], args.iters),
                       "with_two_hop_factors": run(api, nr, ctx, sc, [(vmaps[i], submaps[j][1], 3 * i, 3 * j) for i, j in pairs], args.iters)}
    out["global36"] = {"terms_only": run(api, nr, ctx, nr.global_scene(36, PERT), [], args.iters)}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
