"""Times of the ICP fine registration (glim_amd_icp_align_batch) on one device, the host-driven loop over IntegratedICPFactor.linearize beside it.

Workload: the two scans of tests/test_gicp.py::clouds (the synthetic scene, 0.6 m / 3 deg apart), a 2 048-point source against a 65 536-point
target (the pair manual loop closing refines: a scan against a sub-map), uploaded WITHOUT covariances (the target keeps its normals for the
point-to-plane metric), B problems per call, each from its own perturbation of the planted motion.  Per metric (point-to-point, point-to-plane)
and B in {1, 8, 32}, the variants alternating in one process:
  device_chunk41   glim_amd_icp_align_batch as it ships: at most 41 rounds enqueued between two looks at the statuses
  device_all       the same loop with every one of the 1 + max_trials (401) rounds enqueued up front and one synchronisation (through the trace
                   entry point, which also fills a trace): what the idle rounds cost
  host_loop        the same step rule (tests/lm_restatement.py) driven from the host, one synchronous IntegratedICPFactor.linearize per round and
                   problem, the B problems one after the other -- what a caller of the factor's entry points does, the baseline
Recorded per variant: wall time of the whole batch (p50 and min over `--iters` repeats after a warm-up) and the time between two HIP events on the
context's stream around it, the rounds run, the statuses.  device_chunk41 and device_all must return the same bits (asserted).
No ratio is promised: the tool reports what it measures.  Prints one JSON object; `--out` writes it too.

    python tools/icp_align_time.py [--iters 5] [--out profiles/icp_align/icp_align_time.json]
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
    ap.add_argument("--source-points", type=int, default=2048)
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
    dirs = synth.lidar_directions(64, 1024)
    scans = [synth.scan(scene, T, dirs, frame_id=i).astype(np.float64) for i, T in enumerate(poses)]
    full = api.PointCloudGPU.clone(scans[0], ctx=ctx)  # the normals come from the device's own estimator, then travel without the covariances
    full.find_neighbors(10, download=False)
    full.estimate_covariances(10)
    normals = full.download(covs=False, normals=True)[2].astype(np.float64)
    full.close()
    tg = api.PointCloudGPU.clone(scans[0], normals=normals, ctx=ctx)
    keep = min(args.source_points, len(scans[1]))
    sg = api.PointCloudGPU.clone(scans[1][np.arange(keep) * (len(scans[1]) // keep)], ctx=ctx)
    out = {"what": __doc__.split("\n")[0], "iters": args.iters, "max_correspondence_distance": args.max_distance, "repeated": "one box, not repeated",
           "device": ctx.device_info(), "source_points": int(keep), "target_points": int(tg.size()), "shapes": []}
    rng = np.random.default_rng(11)
    for metric, plane in (("point_to_point", False), ("point_to_plane", True)):
        f = api.IntegratedICPFactor(np.eye(4), 1, tg, sg, max_correspondence_distance=args.max_distance, use_point_to_plane=plane)
        flags = api.ICP_POINT_TO_PLANE if plane else 0
        for B in args.batches:
            T0 = [delta @ lmr.expmap(rng.uniform(-1, 1, 6) * [0.01, 0.01, 0.01, 0.08, 0.08, 0.03]) for _ in range(B)]
            prm, p_host = api.icp_align_params(), lmr.params(dict(lmr.DEFAULTS, max_iterations=200))

            def device_chunk41():
                return api.icp_align_batch([f.target_tree] * B, [sg] * B, T0, args.max_distance, flags, prm)

            def device_all():
                return api.icp_align_debug_trace([f.target_tree] * B, [sg] * B, T0, args.max_distance, flags, prm, rounds_per_chunk="all")[0]

            def host_loop():
                return [lmr.run(lambda T: f.linearize({1: T}), T, p_host)[0] for T in T0]

            variants = {"device_chunk41": device_chunk41, "device_all": device_all, "host_loop": host_loop}
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
            dev, everything, host = last["device_chunk41"], last["device_all"], last["host_loop"]
            for a, b in zip(dev, everything):
                assert np.array_equal(a.T_target_source, b.T_target_source) and np.array_equal(a.compact, b.compact) and (a.status, a.trials) == (b.status, b.trials)
            row = {"metric": metric, "B": B}
            for name in variants:
                row[name] = {"wall_ms_p50": p50_ms(wall[name]), "wall_ms_min": float(min(wall[name]) * 1e3), "hip_events_ms_p50": float(np.median(events[name]))}
            most = max(r.trials for r in dev) + 1
            row["device_chunk41"].update(rounds_enqueued=int(min(1 + prm.resolved_max_trials(), 41 * -(-most // 41))), trials=[r.trials for r in dev],
                                         status=[r.status_name for r in dev])
            row["device_all"].update(rounds_enqueued=1 + prm.resolved_max_trials())
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
