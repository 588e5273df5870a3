#!/usr/bin/env python3
"""Per-block device timelines of the benchmark's single-factor resident session: who is late, and where it runs.

  [GLIM_AMD_LIB=build/ab/<name>/libglim_amd.so] python tools/resident_tail_probe.py <tag> <runs> [out.json]

Builds the headline factor of bench.py (one 128 x 1024 scan against a 0.5 m voxel map, a priority-1 context), times 3 x 2 000 synchronous calls
without stamps (`us_per_call_unstamped`), then takes `runs` stamped timelines, each the last request of 200 calls
(api.resident_timeline(per_block=True): the summary fields and, per block, the four worker stamps and the compute unit).  One JSON object;
tools/late_workers.py sets the workers that share a compute unit with a finalising block against the others."""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from glim_amd import api, synth  # noqa: E402


def main():
    tag, runs = sys.argv[1], int(sys.argv[2])
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(os.getcwd(), f"tail_probe_{tag}.json")
    ctx = api.Context(0, 1)
    yaw0 = math.radians(10.0)
    radius = 0.5 / math.radians(2.0)
    poses = synth.arc_trajectory(2, start=(-2.0 + radius * math.sin(yaw0), -0.5 - radius * math.cos(yaw0), 1.8), yaw0_deg=math.degrees(yaw0))
    t0 = time.time()
    clouds = bench.make_frames(api, ctx, poses[:2], 128, 1024, frame_id0=0)
    vmap = api.GaussianVoxelMapGPU(0.5, ctx=ctx).insert(clouds[0])
    print(f"scans of {clouds[0].size()} points in {time.time() - t0:.1f} s", flush=True)
    T1 = api.pose12(synth.relative_pose(poses[0], poses[1]))[None]
    odo = api.Context(0, 4, priority=1)
    single = api.NonlinearFactorSetGPU(odo)
    single.add(api.IntegratedVGICPFactorGPU(0, 1, vmap, clouds[1]))
    single.profile_sync(T1, iters=50)
    us_call = [single.profile_sync(T1, iters=2000) * 1e3 for _ in range(3)]
    print("us per call (no stamps):", us_call, flush=True)
    api.resident_timeline(0, enable=True, read=False)
    out = {"tag": tag, "lib": os.path.relpath(os.environ.get("GLIM_AMD_LIB") or os.path.join(ROOT, "glim_amd", "libglim_amd.so"), ROOT), "us_per_call_unstamped": us_call, "runs": []}
    for r in range(runs):
        single.profile_sync(T1, iters=200)
        t = api.resident_timeline(0, enable=True, read=True, per_block=True)
        if not t:
            continue
        b = t.pop("blocks")
        t["blocks"] = {k: np.asarray(v).tolist() for k, v in b.items()}
        out["runs"].append(t)
        print(f"run {r}: host {t['host_round_trip']:.2f} loop left {t['worker_loop_left_median']:.2f} / {t['worker_loop_left_max']:.2f} row computed "
              f"{t['worker_row_computed_median']:.2f} / {t['worker_row_computed_max']:.2f} published {t['worker_row_published_median']:.2f} / "
              f"{t['worker_row_published_max']:.2f} rows held {t['finaliser_rows_summed']:.2f} record stored {t['finaliser_record_stored']:.2f}", flush=True)
    api.resident_timeline(0, enable=False, read=False)
    single.close()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(out, open(out_path, "w"))
    print("wrote", out_path)


if __name__ == "__main__":
    main()
