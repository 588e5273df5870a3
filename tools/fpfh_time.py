"""Time of glim_amd_fpfh_estimate and glim_amd_fpfh_match on one device.

Workload: scans of the synthetic scene from the stations of a walk, merged and cut to the requested size (the shape of a merged submap: 66 797
points is BASELINE's submap size), normals from kNN(10) + covariance estimation on the device.  Recorded, the variants alternating in one process
after a warm-up of every variant:
  estimate   n in {10 000, 66 797} x r in {2.5, 5.0} m: wall time of the synchronous call (grid build, both passes, the final synchronise), with
             the mean and maximum neighbour count of the cloud at that radius (from the restatement's pair count on a 2 000-point sample)
  match      n x n for n in {10 000, 66 797}, with and without the reciprocal pass: wall time of the synchronous call and the FP32 rate of the
             all-pairs product (2 * 33 flop per pair, twice that with the reciprocal pass) against the 157 TFLOP/s vector peak
Both calls are synchronous and return results to the host, so the wall time is what a caller sees; it includes the download of the n indices and
distances.  Prints one JSON object; `--out` writes it too.

    python tools/fpfh_time.py [--iters 10] [--out profiles/fpfh/fpfh_time.json]
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

FP32_PEAK_TFLOPS = 157.0


def stats(t):
    t = np.array(t) * 1e3
    return {"p50_ms": round(float(np.median(t)), 3), "p10_ms": round(float(np.percentile(t, 10)), 3), "p90_ms": round(float(np.percentile(t, 90)), 3)}


def submap(n):
    from glim_amd import synth

    scene = synth.Scene.default()
    dirs = synth.lidar_directions(64, 512)
    pts = np.concatenate([synth.scan(scene, T, dirs, 300 + i)[:, :3] for i, T in enumerate(synth.grid_trajectory(3, 3, spacing=3.0))])
    pick = np.sort(np.random.default_rng(1).choice(len(pts), n, replace=False))
    return pts[pick].astype(np.float32)


def neighbour_counts(p, r):
    """mean / max neighbour count of a 2 000-point sample of the cloud (all-pairs in NumPy)"""
    q = p[np.random.default_rng(2).choice(len(p), min(2000, len(p)), replace=False)].astype(np.float64)
    k = np.array([np.count_nonzero(np.sum((p.astype(np.float64) - x) ** 2, axis=1) <= r * r) - 1 for x in q])
    return {"mean_k": round(float(k.mean()), 1), "max_k": int(k.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 66797])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from glim_amd import api

    ctx = api.Context(0, 1)
    out = {"what": __doc__.split("\n")[0], "iters": args.iters, "repeated": "one box, not repeated", "estimate": [], "match": []}
    clouds = {}
    for n in args.sizes:
        c = api.PointCloudGPU.clone(submap(n), ctx=ctx)
        c.find_neighbors(10, download=False)
        c.estimate_covariances(10)
        clouds[n] = c
    variants = [(n, r) for n in args.sizes for r in (2.5, 5.0)]
    times = {v: [] for v in variants}
    for it in range(args.iters + 1):  # the first round is the warm-up
        for v in variants:
            t0 = time.perf_counter()
            f = clouds[v[0]].estimate_fpfh(v[1])
            dt = time.perf_counter() - t0
            f.close()
            if it:
                times[v].append(dt)
    for n, r in variants:
        row = {"n": n, "radius": r}
        row.update(neighbour_counts(clouds[n].download(covs=False, normals=False)[0], r))
        row.update(stats(times[(n, r)]))
        out["estimate"].append(row)
    feats = {n: clouds[n].estimate_fpfh(2.5) for n in args.sizes}
    variants = [(n, rec) for n in args.sizes for rec in (False, True)]
    times = {v: [] for v in variants}
    for it in range(args.iters + 1):
        for v in variants:
            t0 = time.perf_counter()
            api.match_fpfh(feats[v[0]], feats[v[0]], reciprocal=v[1])
            dt = time.perf_counter() - t0
            if it:
                times[v].append(dt)
    for n, rec in variants:
        row = {"source": n, "target": n, "reciprocal": rec}
        row.update(stats(times[(n, rec)]))
        flop = 2.0 * 33.0 * n * n * (2 if rec else 1)
        row["fp32_tflops"] = round(flop / (row["p50_ms"] * 1e-3) / 1e12, 2)
        row["fraction_of_fp32_vector_peak"] = round(row["fp32_tflops"] / FP32_PEAK_TFLOPS, 3)
        out["match"].append(row)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
