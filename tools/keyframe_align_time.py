"""Times of the scan-to-keyframes VGICP registration (glim_amd_keyframe_align_batch) on one device, the host-driven loop over NonlinearFactorSetGPU.linearize_poses beside it.

Workload: GLIM's frame-to-keyframes shape (odometry_estimation_gpu.cpp:150-165, 183-203).  17 scans of 131 072 directions along
synth.arc_trajectory(18, 0.6, 3.0) are the targets, each with voxel maps at 0.5 and 1.0: 17 x 2 = 34 factors with fixed target poses, all on ONE
pose.  12 000 points of the 18th scan are the source.  B frames per call, each from its own perturbation of the true pose (the B problems share
the 34 maps and the source).  Per B in {1, 8}, the two variants alternating in one process:
  device_batch   one glim_amd_keyframe_align_batch call over the B problems (one host synchronisation; 1 + max_trials rounds enqueued, a finished
                 problem's blocks return at once)
  host_loop      the same rule (tests/keyframe_restatement.py over tests/lm_restatement.py) driven from the host over a NonlinearFactorSetGPU of
                 the same 34 B pairs: one synchronous linearize_poses of the whole set per round at P_f^-1 X, the ordered sum and one
                 lm_restatement.step per running problem, until every problem has finished -- the only route before this entry point
Recorded per variant: wall time of the whole batch (p50 and min over `--iters` repeats after a warm-up), the time between two HIP events on the
context's stream around it, and PER-EVALUATION figures: the time per round and per factor evaluation actually used (M x (1 + trials) per
problem).  The two loops need not run the same number of evaluations (the device enqueues every round up front; the host loop stops with the
last problem), so the totals and the per-round figures are both given.  No ratio is promised: the tool reports what it measures.  Prints one
JSON object; `--out` writes it too.

    python tools/keyframe_align_time.py [--iters 5] [--out profiles/keyframe_align/keyframe_align_time.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--keyframes", type=int, default=17)
    ap.add_argument("--resolutions", type=float, nargs="+", default=[0.5, 1.0])
    ap.add_argument("--source-points", type=int, default=12000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    import keyframe_restatement as kr
    import lm_restatement as lmr
    from glim_amd import api, synth

    stream = torch.cuda.Stream()
    ctx = api.Context(0, 1, external_stream=stream.cuda_stream)
    scene = synth.Scene.default()
    K = args.keyframes
    poses = synth.arc_trajectory(K + 1, step=0.6, yaw_step_deg=3.0)
    out = {"what": __doc__.split("\n")[0], "iters": args.iters, "keyframes": K, "resolutions": args.resolutions, "repeated": "one box, not repeated",
           "device": ctx.device_info(), "shapes": []}
    rng = np.random.default_rng(11)

    def cloud(i, rings, az):
        g = api.PointCloudGPU.clone(synth.scan(scene, poses[i], synth.lidar_directions(rings, az), frame_id=i).astype(np.float64), ctx=ctx)
        g.find_neighbors(10, download=False)
        g.estimate_covariances(10)
        return g

    targets, target_points, scans = [], 0, []
    for k in range(K):
        tg = cloud(k, 64, 2048)
        scans.append(tg)
        target_points = int(tg.size())
        targets += [(api.GaussianVoxelMapGPU(res, ctx=ctx).insert(tg), poses[k]) for res in args.resolutions]
        print(f"keyframe {k + 1} of {K}: {target_points} points, {len(args.resolutions)} maps", file=sys.stderr, flush=True)
    M = len(targets)
    Pinv = [np.linalg.inv(P) for _, P in targets]
    p, c, _ = cloud(K, 64, 256).download(covs=True, normals=False)
    keep = min(args.source_points, len(p))
    sel = (np.arange(keep) * (len(p) / keep)).astype(np.int64)
    sg = api.PointCloudGPU.clone(p[sel].astype(np.float64), covs=c[sel].astype(np.float64), ctx=ctx)
    for B in args.batches:
        X0 = [poses[K] @ lmr.expmap(rng.uniform(-1, 1, 6) * [0.01, 0.01, 0.01, 0.08, 0.08, 0.03]) for _ in range(B)]
        problems = [(sg, targets, X) for X in X0]
        prm, p_host = api.LMParams(), lmr.params()
        fset = api.NonlinearFactorSetGPU(ctx)
        for _ in range(B):
            for m, _ in targets:
                fset.add(api.IntegratedVGICPFactorGPU(np.eye(4), 1, m, sg))

        def device_batch():
            return api.vgicp_align_keyframes(problems, 0, prm)

        def host_loop():
            states, rounds = [lmr.new_state(X, p_host) for X in X0], 0
            while any(s["status"] == lmr.RUNNING for s in states):
                records = fset.linearize_poses(np.stack([api.pose12(Pi @ s["cand"]) for s in states for Pi in Pinv]))
                sums = [lmr.record_of_compact(kr.sum_compact([lmr.compact_of_record(L) for L in records[M * i:M * (i + 1)]])) for i in range(B)]
                states = [lmr.step(p_host, s, L) for s, L in zip(states, sums)]
                rounds += 1
            return states, rounds

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
        dev, (host, host_rounds) = last["device_batch"], last["host_loop"]
        row = {"source_points": int(keep), "target_points": target_points, "targets_per_problem": M, "factors": M * B, "B": B}
        used = {"device_batch": int(sum(M * (1 + r.trials) for r in dev)), "host_loop": int(sum(M * (1 + s["trials"]) for s in host))}
        rounds = {"device_batch": 1 + prm.resolved_max_trials(), "host_loop": host_rounds}
        for name in variants:
            w = float(np.median(wall[name]))
            row[name] = {"wall_ms_p50": w * 1e3, "wall_ms_min": float(min(wall[name]) * 1e3), "hip_events_ms_p50": float(np.median(events[name])),
                         "rounds": rounds[name], "factor_evaluations_used": used[name], "wall_us_per_round": w * 1e6 / rounds[name],
                         "wall_us_per_evaluation_used": w * 1e6 / used[name]}
        ran = int(max(1 + r.trials for r in dev))  # (like for like with the host loop, whose every round ran: wall time over the rounds that ran)
        row["device_batch"].update(rounds_that_ran_a_problem=ran, wall_us_per_round_that_ran=row["device_batch"]["wall_ms_p50"] * 1e3 / ran, trials=[r.trials for r in dev], status=[r.status_name for r in dev])
        row["host_loop"].update(evaluations_launched=host_rounds * M * B, trials=[s["trials"] for s in host], status=[api.ALIGN_STATUS[s["status"]] for s in host])
        row["max_pose_difference"] = float(max(np.abs(r.T_target_source - s["T"]).max() for r, s in zip(dev, host)))
        out["shapes"].append(row)
        fset.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
