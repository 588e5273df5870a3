"""Kernel times of the RANSAC global registration (glim_amd_ransac_align) on one device.

Workload: a source cut from the merged scans of the synthetic scene, the target its rigid copy plus clutter, `nearest` the identity with 30 %
of the entries redirected.  Recorded per shape, by HIP events inside the library (glim_amd_ransac_profile: one round of 1 024 hypotheses, mean
of `--iters` rounds after a warm-up), the variants alternating in one process:
  kernels    microseconds of the hypothesis, scoring and fold kernels, with the occupancy table in LDS and -- the same input, the debug cut
             set to 0 -- in global memory, at the GPU-test shape (3 001 points) and at 10 000 / 50 000 points
  align      wall time of the synchronous glim_amd_ransac_align with 5 000 iterations and the early stop out of reach
  overlap    the same 1 024 poses scored through glim_amd_overlap_batch on a Gaussian voxel map of the same resolution, the only route before
             (wall time of the synchronous call), alternating with `align` of 1 024 iterations
Prints one JSON object; `--out` writes it too.

    python tools/ransac_time.py [--iters 10] [--out profiles/ransac/ransac_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def p50_ms(t):
    return round(float(np.median(np.array(t)) * 1e3), 3)


def make_case(n):
    from fpfh_time import submap

    src = submap(n)
    rng = np.random.default_rng(3)
    c, s = np.cos(0.6), np.sin(0.6)
    Rm = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    copy = (src.astype(np.float64) @ Rm.T + [1.5, -2.0, 0.4]).astype(np.float32)
    lo, hi = copy.min(axis=0), copy.max(axis=0)
    target = np.concatenate([copy, rng.uniform(lo, hi, (n // 2, 3)).astype(np.float32)])
    nearest = np.arange(n, dtype=np.int32)
    pick = rng.permutation(n)[:int(0.3 * n)]
    nearest[pick] = rng.integers(0, len(target), len(pick))
    return src, target, nearest


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[3001, 10000, 50000])
    ap.add_argument("--resolution", type=float, default=1.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from glim_amd import _lib, api

    ctx = api.Context(0, 1)
    out = {"what": __doc__.split("\n")[0], "iters": args.iters, "repeated": "one box, not repeated", "resolution": args.resolution, "shapes": []}
    for n in args.sizes:
        src, tgt, nearest = make_case(n)
        tc, sc = api.PointCloudGPU.clone(tgt, ctx=ctx), api.PointCloudGPU.clone(src, ctx=ctx)
        prm = api.RansacParams(seed=1, inlier_voxel_resolution=args.resolution, early_stop_inlier_rate=2.0)
        row = {"source": n, "target": len(tgt)}
        for name, cut in (("lds", 8192), ("global", 0)):
            _lib.lib().glim_amd_debug_ransac_max_lds_slots(cut)
            row["kernels_" + name] = api.ransac_profile(tc, sc, nearest, prm, args.iters)
        _lib.lib().glim_amd_debug_ransac_max_lds_slots(8192)
        # the poses of the first round, for the route through the overlap entry
        prm.max_iterations = 1024
        rec = api.ransac_debug_hypotheses(tc, sc, nearest, prm, 0, 1024)
        vm = api.GaussianVoxelMapGPU(args.resolution, ctx=ctx)
        tc.find_neighbors(10, download=False)
        tc.estimate_covariances(10)
        vm.insert(tc)
        poses = []
        for p in rec["poses"]:
            T = np.eye(4)
            T[:3] = p.reshape(3, 4)
            poses.append(T)
        queries = [([vm], sc, [T]) for T in poses]
        t_align, t_overlap, t_full = [], [], []
        for it in range(args.iters + 1):  # the first round is the warm-up
            t0 = time.perf_counter()
            api.ransac_align(tc, sc, nearest, prm)
            t1 = time.perf_counter()
            api.overlap_gpu_batch(queries, ctx=ctx)
            t2 = time.perf_counter()
            if it:
                t_align.append(t1 - t0)
                t_overlap.append(t2 - t1)
        prm.max_iterations = 5000
        for it in range(args.iters + 1):
            t0 = time.perf_counter()
            r = api.ransac_align(tc, sc, nearest, prm)
            if it:
                t_full.append(time.perf_counter() - t0)
        row["align_1024_ms"] = p50_ms(t_align)
        row["overlap_batch_1024_poses_ms"] = p50_ms(t_overlap)
        row["overlap_over_align"] = round(row["overlap_batch_1024_poses_ms"] / row["align_1024_ms"], 2)
        row["align_5000_ms"] = p50_ms(t_full)
        row["inlier_rate"] = r.inlier_rate
        out["shapes"].append(row)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
