"""Times of the GNC global registration (glim_amd_gnc_align) on one device, RANSAC on the same inputs beside it.

Workload: tools/ransac_time.py's -- a source cut from the merged scans of the synthetic scene, the target its rigid copy plus clutter, `nearest`
the identity with 30 % of the entries redirected.  Recorded per source size, with and without the tuple test, the variants alternating in one
process:
  stages     microseconds of the selection, the tuple test, the gather + solve kernel, the occupancy table and the scoring of the final pose, by
             HIP events inside the library (glim_amd_gnc_profile: mean of `--iters` calls after a warm-up)
  align      wall time of the synchronous glim_amd_gnc_align (p50), its inlier_rate and list length
  ransac     wall time of glim_amd_ransac_align with its default parameters on the same inputs (p50), its inlier_rate
Prints one JSON object; `--out` writes it too.

    python tools/gnc_time.py [--iters 10] [--out profiles/gnc/gnc_time.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[3000, 10000, 66797])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from glim_amd import api
    from ransac_time import make_case, p50_ms

    ctx = api.Context(0, 1)
    out = {"what": __doc__.split("\n")[0], "iters": args.iters, "repeated": "one box, not repeated", "shapes": []}
    for n in args.sizes:
        src, tgt, nearest = make_case(n)
        tc, sc = api.PointCloudGPU.clone(tgt, ctx=ctx), api.PointCloudGPU.clone(src, ctx=ctx)
        variants = {"plain": api.GncParams(seed=1, max_init_samples=n), "tuple_test": api.GncParams(seed=1, max_init_samples=n, tuple_check=True)}
        rprm = api.RansacParams(seed=1)
        row = {"source": n, "target": len(tgt)}
        times = {k: [] for k in list(variants) + ["ransac"]}
        last = {}
        for it in range(args.iters + 1):  # the first round is the warm-up
            for name, prm in variants.items():
                t0 = time.perf_counter()
                last[name] = api.gnc_align(tc, sc, nearest, prm)
                if it:
                    times[name].append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            last["ransac"] = api.ransac_align(tc, sc, nearest, rprm)
            if it:
                times["ransac"].append(time.perf_counter() - t0)
        for name, prm in variants.items():
            r = last[name]
            row[name] = {"align_ms": p50_ms(times[name]), "inlier_rate": r.inlier_rate, "list_length": r.info["list_length"],
                         "num_tuples": r.info["num_tuples"], "stages_us": api.gnc_profile(tc, sc, nearest, prm, args.iters)}
        row["ransac"] = {"align_ms": p50_ms(times["ransac"]), "inlier_rate": last["ransac"].inlier_rate, "iterations_run": last["ransac"].iterations_run}
        out["shapes"].append(row)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
