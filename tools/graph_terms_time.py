"""Times of the two pose optimisers with damping terms and Huber between terms (glim_amd_graph_align_terms) on one device.

Workloads:
  pose_graph   tests/graph_terms_restatement.py's ring scene -- N poses on a ring, a Gaussian odometry chain, five loop betweens of which one
               (two at N = 64) is falsified, a damping of 1e6 on pose 0 and no prior, the initial poses dead reckoning -- at N = 64 and
               N = 256, terms only (no factor), once with the width 1.0 on the loops (glim_amd_graph_align_terms) and once with every width 0
               (the damping still goes through the same entry point).  The default parameters.
  factors      the N = 64 graph of tools/graph_align_time.py (the clouds of bench.py's m2_global256, all pairs), max_iterations = 3, once
               with its prior of precision 1e6 on sub-map 0 (glim_amd_graph_align) and once with a damping of 1e6 there instead
               (glim_amd_graph_align_terms).
Recorded per variant: wall time of the call (p50 and min over `--iters` repeats after a warm-up, the variants of a workload alternating in one
process), the rounds that ran, the status and the cost.  No ratio is promised: the tool reports what it measures.

  --against ROOT   the timing condition of the change that added the terms: the round time of graph_align WITHOUT new terms at N = 64
                   (tools/graph_align_time.py's round_split.trial_round_ms) in this tree and in the tree at ROOT (a built checkout of the
                   parent commit), the two alternating on the same box, each measured twice in a process of its own.  The margin is the
                   spread of the parent's own two measurements in this run.  Both pairs of figures are recorded.

    python tools/graph_terms_time.py [--iters 5] [--against ../parent] [--out profiles/graph_terms/graph_terms_time.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def alternating(variants, iters):
    """{name: fn} -> {name: (wall seconds of each repeat, fn's last return)}: one warm-up of each, then the variants in turn, `iters` times"""
    out = {k: ([], None) for k in variants}
    for it in range(iters + 1):
        for k, fn in variants.items():
            t0 = time.perf_counter()
            res = fn()
            if it:
                out[k][0].append(time.perf_counter() - t0)
            out[k] = (out[k][0], res)
    return out


def report(times, res):
    return {"wall_ms_p50": float(np.median(times)) * 1e3, "wall_ms_min": float(min(times)) * 1e3, "rounds_that_ran": 1 + res.trials, "iterations": res.iterations,
            "status": res.status_name, "cost": res.cost, "between_cost": res.between_cost,
            "down_weighted_betweens": None if res.between_weights is None else int(np.count_nonzero(res.between_weights != 1.0))}


def pose_graph(api, gtr, ctx, N, iters):
    g, betweens, dampings, X0, _ = gtr.ring_scene(N)
    gauss = [b[:4] for b in betweens]

    def call(bs):
        ctx.synchronize()
        return api.graph_align([], [], bs, list(X0), dampings=dampings, ctx=ctx)

    got = alternating({"huber_loops": lambda: call(betweens), "gaussian_loops": lambda: call(gauss)}, iters)
    out = {"poses": N, "betweens": len(betweens), "rows": 6 * N}
    for k, (t, res) in got.items():
        out[k] = report(t, res)
        out[k]["round_ms"] = out[k]["wall_ms_p50"] / (1 + res.trials)
    return out


def with_factors(api, lmr, ctx, N, iters):
    import bench

    submaps = bench.make_merged_submaps(api, ctx, N, 4, 40, 560)  # bench.py's defaults for global256
    vmaps = [api.GaussianVoxelMapGPU(1.0, ctx=ctx).insert(g) for _, g in submaps]
    poses = [T for T, _ in submaps]
    factors = [(vmaps[i], submaps[j][1], i, j) for j in range(N) for i in range(j)]
    rng = np.random.default_rng(N)
    X0 = [poses[0]] + [T @ lmr.expmap(rng.uniform(-1, 1, 6) * [0.005, 0.005, 0.005, 0.04, 0.04, 0.02]) for T in poses[1:]]
    prm = api.graph_align_params(max_iterations=3)

    def call(priors, dampings):
        ctx.synchronize()
        return api.graph_align(factors, priors, [], X0, 0, prm, ctx=ctx, dampings=dampings)

    got = alternating({"prior_1e6": lambda: call([(0, poses[0], 1e6 * np.eye(6))], []), "damping_1e6": lambda: call([], [(0, 1e6)])}, iters)
    out = {"poses": N, "factors": len(factors), "rows": 6 * N}
    for k, (t, res) in got.items():
        out[k] = report(t, res)
        out[k]["max_distance_to_the_true_poses"] = float(np.abs(res.poses - np.stack(poses)).max())
    return out


def round_time_against(parent, iters):
    """tools/graph_align_time.py --sizes 64 in the tree at `parent` and in this one, alternating, twice each -> the trial round times"""
    out = {"parent": [], "this": [], "what": "round_split.trial_round_ms of tools/graph_align_time.py --sizes 64: graph_align without new terms"}
    for _ in range(2):
        for name, root in (("parent", os.path.abspath(parent)), ("this", ROOT)):
            env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH", "GLIM_AMD_LIB")}
            res = subprocess.run([sys.executable, os.path.join(root, "tools", "graph_align_time.py"), "--sizes", "64", "--iters", str(iters)], cwd=root, env=env,
                                 capture_output=True, text=True, check=True, timeout=900)
            out[name].append(json.loads(res.stdout)["sizes"]["64"]["round_split"]["trial_round_ms"])
            print(f"{name}: {out[name][-1]:.3f} ms", file=sys.stderr, flush=True)
    out["margin_the_parents_own_spread"] = abs(out["parent"][0] - out["parent"][1]) / min(out["parent"])
    out["this_over_parent_of_the_means"] = float(np.mean(out["this"]) / np.mean(out["parent"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--factors", type=int, default=64, help="poses of the graph with factors; 0: leave it out")
    ap.add_argument("--against", default="", help="a built checkout of the parent commit")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out = {"what": __doc__.split("\n")[0], "iters": args.iters, "repeated": "one box, not repeated"}
    if args.against:  # first, in processes of their own: this process has not opened the device yet
        out["graph_align_round_time_n64"] = round_time_against(args.against, args.iters)
    import graph_terms_restatement as gtr
    import lm_restatement as lmr
    from glim_amd import api

    ctx = api.Context(0, 1)
    out["device"] = ctx.device_info()
    out["pose_graph"] = {str(N): pose_graph(api, gtr, ctx, N, args.iters) for N in args.sizes}
    if args.factors:
        out["factors"] = with_factors(api, lmr, ctx, args.factors, args.iters)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
