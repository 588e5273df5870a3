"""Times of the GICP fine registration (glim_amd_gicp_align_batch) on one device, the host-driven loop over IntegratedGICPFactor.linearize beside it.

Workload: the two scans of tests/test_gicp.py::clouds (the synthetic scene, 0.6 m / 3 deg apart) at a 10 000-point and a 65 536-point source, B
problems per call, each from its own perturbation of the planted motion (candidates of the pose-graph module: one target, B initial poses).
Per size and B in {1, 8, 32}, the two variants alternating in one process:
  device_batch   one glim_amd_gicp_align_batch call over the B problems (one host synchronisation)
  host_loop      the same step rule (tests/lm_restatement.py) driven from the host, one synchronous IntegratedGICPFactor.linearize per round and
                 problem, the B problems one after the other -- what a caller of the existing entry points does, the baseline
Recorded per variant: wall time of the whole batch (p50 and min over `--iters` repeats after a warm-up) and the time between two HIP events on the
context's stream around it (the context runs on a torch stream, so torch's events bracket its work), the rounds run, the statuses.
No ratio is promised: the tool reports what it measures.  Prints one JSON object; `--out` writes it too.

    python tools/gicp_align_time.py [--iters 5] [--out profiles/gicp_align/gicp_align_time.json]
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


def p50_ms(v):
    return float(np.median(v) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--max-distance", type=float, default=0.5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    import lm_restatement as lmr
    from glim_amd import api, synth

    stream = torch.cuda.Stream()
    ctx = api.Context(0, 1, external_stream=stream.cuda_stream)
    scene = synth.Scene.default()
    poses = synth.arc_trajectory(2, step=0.6, yaw_step_deg=3.0)
    delta = np.linalg.inv(poses[0]) @ poses[1]
    out = {"what": __doc__.split("\n")[0], "iters": args.iters, "max_correspondence_distance": args.max_distance, "repeated": "one box, not repeated",
           "device": ctx.device_info(), "shapes": []}
    rng = np.random.default_rng(11)
    for label, rings, az, keep in (("10000", 64, 256, 10000), ("65536", 64, 1024, 65536)):
        dirs = synth.lidar_directions(rings, az)
        clouds = []
        for i, T in enumerate(poses):
            g = api.PointCloudGPU.clone(synth.scan(scene, T, dirs, frame_id=i).astype(np.float64), ctx=ctx)
            g.find_neighbors(10, download=False)
            g.estimate_covariances(10)
            clouds.append(g)
        tg = clouds[0]
        p, c, _ = clouds[1].download(covs=True, normals=False)
        sel = np.arange(keep) * (len(p) // keep)
        sg = api.PointCloudGPU.clone(p[sel].astype(np.float64), covs=c[sel].astype(np.float64), ctx=ctx)
        f = api.IntegratedGICPFactor(np.eye(4), 1, tg, sg, max_correspondence_distance=args.max_distance)
        for B in args.batches:
            T0 = [delta @ lmr.expmap(rng.uniform(-1, 1, 6) * [0.01, 0.01, 0.01, 0.08, 0.08, 0.03]) for _ in range(B)]
            prm, p_host = api.LMParams(), lmr.params()

            def device_batch():
                return api.gicp_align_batch([f.target_tree] * B, [sg] * B, T0, args.max_distance, prm)

            def host_loop():
                return [lmr.run(lambda T: f.linearize({1: T}), T, p_host)[0] for T in T0]

            variants = {"device_batch": device_batch, "host_loop": host_loop}
            wall = {k: [] for k in variants}
            events = {k: [] for k in variants}
            last = {}
            for it in range(args.iters + 1):  # the first round is the warm-up
                for name, fn in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    e0.record(stream)
                    last[name] = fn()
                    e1.record(stream)
                    e1.synchronize()
                    if it:
                        wall[name].append(time.perf_counter() - t0)
                        events[name].append(e0.elapsed_time(e1))
            dev, host = last["device_batch"], last["host_loop"]
            row = {"source": label, "source_points": int(keep), "target_points": int(tg.size()), "B": B}
            for name in variants:
                row[name] = {"wall_ms_p50": p50_ms(wall[name]), "wall_ms_min": float(min(wall[name]) * 1e3), "hip_events_ms_p50": float(np.median(events[name]))}
            row["device_batch"].update(rounds_enqueued=1 + prm.resolved_max_trials(), trials=[r.trials for r in dev], status=[r.status_name for r in dev])
            row["host_loop"].update(linearize_calls=int(sum(1 + s["trials"] for s in host)), trials=[s["trials"] for s in host],
                                    status=[api.ALIGN_STATUS[s["status"]] for s in host])
            row["max_pose_difference"] = float(max(np.abs(r.T_target_source - s["T"]).max() for r, s in zip(dev, host)))
            out["shapes"].append(row)
        f.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
