"""Times the device side of the plane bundle-adjustment tool (include/glim_amd.h "Plane / edge bundle-adjustment factors and ball selection")
beside the NumPy restatement of the same steps, and writes profiles/plane_ba/plane_ba_time.json.

Workload: 24 sub-maps of 65 536 points within 25 m of one another, a wall through the centre, r0 = 1.  Steps: ball selection, ball
statistics, the whole radius search, factor creation from the ball, one linearize.  Every library call here is synchronous (it ends with
its own stream synchronisation), so the figures are host wall-clock times around the call, warm-up first, median of the repeats; the
clouds are resident before the clock starts.  One box, one run; no speed-up beyond these two programs is claimed.

    python tools/plane_ba_time.py [--repeats 20]
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


def make_workload(S=24, n=65536, seed=3):
    from glim_amd.se3 import se3_exp

    rng = np.random.default_rng(seed)
    center = np.array([40.0, -25.0, 2.0])
    clouds, poses = [], []
    for s in range(S):
        T = se3_exp(np.concatenate([rng.normal(size=3) * 0.3, center + rng.uniform(-12.0, 12.0, size=3)]))
        w = center + rng.uniform(-15.0, 15.0, size=(n, 3))  # the sub-map's surroundings
        wall = rng.random(n) < 0.5  # half of the points on a wall through the centre (x = centre_x, 2 cm thick)
        w[wall, 0] = center[0] + rng.uniform(-0.01, 0.01, size=int(wall.sum()))
        w[wall, 1:] = center[1:] + rng.uniform(-6.0, 6.0, size=(int(wall.sum()), 2))
        clouds.append((w - T[:3, 3]) @ T[:3, :3])
        poses.append(T)
    return clouds, poses, center


def median_ms(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_ba", "plane_ba_time.json"))
    args = ap.parse_args()
    import plane_ba_restatement as R
    from glim_amd import api

    clouds, poses, center = make_workload()
    ctx = api.Context(0, 1)
    gpu = [api.clone_exact(p, ctx=ctx) for p in clouds]
    r0 = 1.0
    prm = api.BundleAdjustmentParams()
    pairs, count = api.ba_ball_select(gpu, poses, center, r0)
    found = api.ba_auto_radius(gpu, poses, center, r0, prm, trace=True)
    factor = api.PlaneEVMFactor.from_ball(gpu, poses, center, r0)
    kept = factor.frames()
    kept_poses = [poses[s] for s in kept]
    dev = {
        "select_ms": median_ms(lambda: api.ba_ball_select(gpu, poses, center, r0), args.repeats),
        "stats_ms": median_ms(lambda: api.ba_ball_stats(gpu, poses, center, r0), args.repeats),
        "auto_radius_ms": median_ms(lambda: api.ba_auto_radius(gpu, poses, center, r0, prm), args.repeats),
        "factor_create_from_ball_ms": median_ms(lambda: api.PlaneEVMFactor.from_ball(gpu, poses, center, r0).close(), args.repeats),
        "linearize_ms": median_ms(lambda: factor.linearize(kept_poses), args.repeats),
        "error_ms": median_ms(lambda: factor.error(kept_poses), args.repeats),
    }

    # the NumPy restatement of the same steps (FP64, one thread of the interpreter driving vectorised operations)
    def np_eval(r):
        _, q = R.select(clouds, poses, center, r)
        return len(q), (np.linalg.eigvalsh(R.covariance(*R.sums(q))) if len(q) else np.full(3, np.nan))

    ref_pairs, _ = R.select(clouds, poses, center, r0)
    frames = [clouds[s][ref_pairs[ref_pairs[:, 0] == s, 1]] for s in kept]
    few = max(1, args.repeats // 10)
    host = {
        "select_ms": median_ms(lambda: R.select(clouds, poses, center, r0), few, warmup=1),
        "select_and_stats_ms": median_ms(lambda: np_eval(r0), few, warmup=1),
        "auto_radius_ms": median_ms(lambda: R.auto_radius(np_eval, r0, prm.min_radius, prm.max_radius, prm.plane_eps), few, warmup=1),
        "factor_linearize_point_form_ms": median_ms(lambda: R.factor(frames, kept_poses, 0), few, warmup=1),
    }
    out = {
        "what": "plane bundle-adjustment tool: device calls (synchronous, host wall clock, median) beside the NumPy restatement; one box, one run",
        "submaps": len(clouds), "points_per_submap": len(clouds[0]), "r0": r0, "selected_at_r0": int(count), "selection_equals_restatement": bool(np.array_equal(pairs, ref_pairs)),
        "frames_in_factor": int(len(kept)), "auto_radius": {"radius": found["radius"], "stop": found["stop"], "evaluations": sum(1 for t in found["trace"] if t["count"] >= 0)},
        "repeats": args.repeats, "device": dev, "numpy_restatement": host, "device_name": ctx.device_info()["name"],
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
