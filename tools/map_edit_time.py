"""Times the device side of the map editor (include/glim_amd.h "Map editing") beside the NumPy restatement of the same steps, alternating
the two in one process, and writes profiles/map_edit/map_edit_time.json.

Workload: 24 sub-maps of 65 536 points within 25 m of one another, a wall through the picked point.  Steps: the box and sphere gizmo, the
window, the radius selection, the outliers in a radius, region growing (in a small window, where the restatement's distance matrix still
fits, and in the editor's default window, device only), and the removal of the grown cluster.  Every library call here is synchronous, so
the figures are host wall-clock times around the call, warm-up first, median of the repeats; the clouds are resident before the clock
starts.  One box, one run; no speed-up beyond these two programs is claimed.

Min-cut segmentation runs at the editor's defaults (foreground 0.5 m, background 5 m, weight 10, k 20) on the same workload: the device call
beside scipy.sparse.csgraph.maximum_flow on the graph the device built and downloaded (the time inside maximum_flow alone; building the
matrix and reading the cut off the residuals are not counted), and whether the two agree.  --min-cut-only measures that line alone and
merges it into the existing file.

    python tools/map_edit_time.py [--repeats 20] [--out FILE] [--min-cut-only]
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
        w = center + rng.uniform(-15.0, 15.0, size=(n, 3))
        wall = rng.random(n) < 0.5  # half of the points on a wall through the centre (x = centre_x, 2 cm thick)
        w[wall, 0] = center[0] + rng.uniform(-0.01, 0.01, size=int(wall.sum()))
        w[wall, 1:] = center[1:] + rng.uniform(-6.0, 6.0, size=(int(wall.sum()), 2))
        clouds.append((w - T[:3, 3]) @ T[:3, :3])
        poses.append(T)
    return clouds, poses, center


def median_ms(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def min_cut_line(api, gpu, poses, center, repeats=3, save=None):
    """the device call at the editor's defaults beside scipy's maximum flow on the downloaded graph; save: called with the device's half of
    the line before scipy starts"""
    import min_cut_restatement as M

    prm = api.MinCutParams()
    got = api.edit_min_cut(gpu, poses, center, prm)
    print("min-cut:", {k: v for k, v in got.items() if k != "pairs"}, file=sys.stderr, flush=True)
    line = {k: got[k] for k in ("count", "num_candidates", "num_edges", "num_foreground", "num_background", "flow", "rounds", "looks", "status")}
    line.update(device_ms=median_ms(lambda: api.edit_min_cut(gpu, poses, center, prm), repeats, warmup=0), device_repeats=repeats,
                params={k: getattr(prm, k) for k in ("distance_sigma", "foreground_mask_radius", "background_mask_radius", "foreground_weight", "k_neighbors")})
    if save:
        save(line)
    g = api.diag_edit_min_cut_graph(gpu, poses, center, prm)
    times = {}
    flow, flags = M.judge(g["num_candidates"], g["edges"], g["edge_cap"], g["source_cap"], g["sink_cap"], times=times)
    line.update(scipy_maximum_flow_ms=times["maximum_flow_s"] * 1e3, scipy_flow=flow, scipy_count=int(flags.sum()),
                equal=bool(got["status"] == "ok" and got["flow"] == flow and np.array_equal(got["pairs"], g["candidates"][flags == 1])))
    print("min-cut: scipy", flow, int(flags.sum()), times, file=sys.stderr, flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_edit", "map_edit_time.json"))
    ap.add_argument("--min-cut-only", action="store_true", help="measure the min-cut line alone and merge it into the existing file")
    args = ap.parse_args()
    import map_edit_restatement as R
    from glim_amd import api

    clouds, poses, center = make_workload()
    ctx = api.Context(0, 1)
    gpu = [api.clone_exact(p, ctx=ctx) for p in clouds]
    if args.min_cut_only:
        out = json.load(open(args.out))
        assert out["submaps"] == len(clouds) and out["points_per_submap"] == len(clouds[0])
        def save(line):
            out["min_cut"] = line
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)

        save(min_cut_line(api, gpu, poses, center, save=save))
        print(json.dumps(out["min_cut"]))
        return
    from oracle import oracle as orc

    model = np.eye(4)
    model[:3, :3] *= 3.0
    model[:3, 3] = center
    local = api.edit_local_matrices(model, poses)
    radius, thr, few = 1.0, 0.05, max(1, args.repeats // 10)
    small = dict(resolution=0.2, window=2)  # a 1 m box: region growing where the restatement's candidates-squared matrix still fits
    prm = api.RegionGrowingParams(distance_threshold=thr, dilation_radius=thr)
    steps = {}

    def step(name, dev, ref, same, repeats=None):
        """device and restatement one after the other, the same inputs; `same` compares their results once"""
        got, want = dev(), (ref() if ref else None)
        steps[name] = {"device_ms": median_ms(dev, repeats or args.repeats, warmup=0 if repeats else 2), "device_repeats": repeats or args.repeats,
                       "numpy_restatement_ms": median_ms(ref, few, warmup=0) if ref else None, "equal": bool(same(got, want)) if ref else None}
        return got

    pair_eq = lambda g, w: np.array_equal(g[0], w[0])  # noqa: E731
    box = step("box", lambda: api.edit_select(gpu, poses, api.EDIT_BOX, model_matrix=model), lambda: R.select(clouds, local, R.BOX), pair_eq)
    step("sphere", lambda: api.edit_select(gpu, poses, api.EDIT_SPHERE, model_matrix=model), lambda: R.select(clouds, local, R.SPHERE), pair_eq)
    win = step("window", lambda: api.edit_select(gpu, poses, api.EDIT_WINDOW, center=center), lambda: R.select(clouds, poses, R.WINDOW, center), pair_eq)
    ball = step("radius", lambda: api.edit_select(gpu, poses, api.EDIT_WINDOW_BALL, center=center, radius=radius),
                lambda: R.select(clouds, poses, R.WINDOW_BALL, center, radius), pair_eq)
    out_dev = step("outliers", lambda: api.edit_select_outliers(gpu, poses, center, radius), lambda: R.select_outliers(orc, clouds, poses, center, radius),
                   pair_eq)
    grown = step("region_growing_small_window", lambda: api.edit_region_grow(gpu, poses, center, prm, **small),
                 lambda: R.region_grow(clouds, poses, center, thr, dilation_radius=thr, **small),
                 lambda g, w: np.array_equal(g["pairs"], w["pairs"]) and np.array_equal(g["levels"], w["levels"]))
    big = step("region_growing_default_window", lambda: api.edit_region_grow(gpu, poses, center, prm), None, None, repeats=3)
    step("remove_selected", lambda: api.edit_remove_selected(gpu, big["pairs"]), None, None, repeats=5)
    out = {
        "what": "map editor: device calls (synchronous, host wall clock, median) beside the NumPy restatement, alternating in one process; one box, one run",
        "submaps": len(clouds), "points_per_submap": len(clouds[0]), "radius": radius, "distance_threshold": thr, "repeats": args.repeats,
        "restatement_repeats": few, "rounds_per_look": api.EDIT_ROUNDS_PER_LOOK,
        "selected": {"box": box[1], "window": win[1], "radius": ball[1], "outliers": out_dev[1]},
        "region_growing_small_window": {k: grown[k] for k in ("count", "num_candidates", "rounds")},
        "region_growing_default_window": {k: big[k] for k in ("count", "num_candidates", "rounds")},
        "steps": steps, "device_name": ctx.device_info()["name"],
        "min_cut": min_cut_line(api, gpu, poses, center),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
