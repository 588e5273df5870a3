"""Times the resampling of resident clouds (include/glim_amd.h "Resampling a resident cloud") beside what a caller does without it, the
variants alternating in one process, and writes profiles/resample/resample_time.json.

Workload: a 65 536-point and a 1 048 576-point cloud whose covariances and normals were estimated on the device (plane form).  Device:
random_sampling at rates 0.1 and 0.5, sample at the same indices, transform by a rigid pose.  The route without these calls: for the two
samplings, download, the NumPy gather at the same indices and PointCloudGPU.clone of the subset; for transform, the NumPy restatement on
arrays that are already on the host, and the upload.  Every library call here is synchronous, so the figures are host wall-clock times
around the call, warm-up first, median of the repeats; the clouds are resident before the clock starts.  One box, one run; no speed-up
beyond these two programs is claimed.

The gather of the map editor's removal moved into a header this change shares with it, so the removal step of tools/map_edit_time.py
(edit_remove_selected of the grown cluster, 24 sub-maps of 65 536 points) is timed on this tree and on a library built from the parent
commit, in processes of their own, alternating: --parent-root DIR names a directory that holds the parent's glim_amd package with its
library built.  --removal-only is what such a process runs.

    python tools/resample_time.py [--repeats 20] [--out FILE] [--parent-root DIR --parent-commit HASH] [--removal-only [--package-root DIR]]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def median_ms(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def removal_line(repeats):
    """the removal step of tools/map_edit_time.py: edit_remove_selected of the cluster its default-window region growing finds"""
    import map_edit_time as M
    from glim_amd import api

    clouds, poses, center = M.make_workload()
    ctx = api.Context(0, 1)
    gpu = [api.clone_exact(p, ctx=ctx) for p in clouds]
    prm = api.RegionGrowingParams(distance_threshold=0.05, dilation_radius=0.05)
    big = api.edit_region_grow(gpu, poses, center, prm)
    return {"remove_selected_ms": median_ms(lambda: api.edit_remove_selected(gpu, big["pairs"]), repeats), "repeats": repeats,
            "removed_points": int(big["count"]), "submaps_touched": int(len(np.unique(big["pairs"][:, 0])))}


def removal_compare(parent_root, repeats, rounds=3):
    """this tree and the parent's package, `rounds` processes each, alternating"""
    runs = {"parent": [], "this": []}
    for _ in range(rounds):
        for name, root in (("parent", os.path.abspath(parent_root)), ("this", ROOT)):
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--removal-only", "--repeats", str(repeats), "--package-root", root],
                                 capture_output=True, text=True, timeout=600, check=True)
            runs[name].append(json.loads(res.stdout.strip().splitlines()[-1]))
    ms = {k: [r["remove_selected_ms"] for r in v] for k, v in runs.items()}
    return {"what": "edit_remove_selected of tools/map_edit_time.py's workload, median of the repeats per process; processes alternate",
            "repeats": repeats, "removed_points": runs["this"][0]["removed_points"], "submaps_touched": runs["this"][0]["submaps_touched"],
            "parent_ms": ms["parent"], "this_ms": ms["this"], "parent_median_ms": float(np.median(ms["parent"])),
            "this_median_ms": float(np.median(ms["this"])), "parent_spread_ms": float(max(ms["parent"]) - min(ms["parent"]))}


def cloud_lines(api, ctx, n, repeats, seed=5):
    import gnc_restatement as G
    import resample_restatement as R

    rng = np.random.default_rng(n)
    pts = rng.uniform(-40.0, 40.0, size=(n, 3)).astype(np.float32)
    pts[:, 2] = (0.05 * np.sin(0.3 * pts[:, 0]) + rng.uniform(-0.01, 0.01, size=n)).astype(np.float32)  # a gently waved floor
    cloud = api.PointCloudGPU.clone(pts, ctx=ctx)
    cloud.find_neighbors(10, download=False)
    cloud.estimate_covariances(10)
    c, s = np.cos(0.7), np.sin(0.7)
    T = np.array([[c, -s, 0.0, 21.5], [s, c, 0.0, -19.25], [0.0, 0.0, 1.0, 3.125], [0.0, 0.0, 0.0, 1.0]])
    few = max(3, repeats // 4)
    keys = (G.hashes(seed, np.arange(n)) >> np.uint64(32)).astype(np.uint32)
    order = np.lexsort((np.arange(n), keys))
    lines = {}
    for rate in (0.1, 0.5):
        idx = np.sort(order[: R.count(n, rate)]).astype(np.int32)

        def host_route():
            xyz, covs, normals = cloud.download()
            return api.PointCloudGPU.clone(xyz[idx], covs[idx], normals[idx], ctx=ctx)

        got, want = cloud.random_sampling(rate, seed).download(), host_route().download()
        lines[f"rate_{rate}"] = {
            "points_kept": int(len(idx)),
            "random_sampling_ms": median_ms(lambda: cloud.random_sampling(rate, seed), repeats),
            "sample_same_indices_ms": median_ms(lambda: cloud.sample(idx), repeats),
            "download_numpy_gather_clone_ms": median_ms(host_route, few, warmup=1), "host_route_repeats": few,
            "equal": bool(all(a.tobytes() == b.tobytes() for a, b in zip(got, want))),
        }
    xyz, covs, normals = cloud.download()

    def host_transform():
        p = np.concatenate([xyz.astype(np.float64), np.ones((n, 1))], axis=1)
        q, d, m = R.transform(p, R.cov6(covs.astype(np.float64)), normals.astype(np.float64), T)
        return api.PointCloudGPU.clone(q[:, :3].astype(np.float32), R.cov33(d).astype(np.float32), m.astype(np.float32), ctx=ctx)

    got, want = cloud.transform(T).download(), host_transform().download()
    lines["transform"] = {"transform_ms": median_ms(lambda: cloud.transform(T), repeats),
                          "numpy_restatement_and_clone_ms": median_ms(host_transform, few, warmup=1), "host_route_repeats": few,
                          "equal": bool(all(a.tobytes() == b.tobytes() for a, b in zip(got, want)))}
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample", "resample_time.json"))
    ap.add_argument("--parent-root", default=None, help="directory with the parent commit's glim_amd package, built: time the removal step on both")
    ap.add_argument("--package-root", default=None, help="with --removal-only: import glim_amd from this directory")
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--removal-only", action="store_true", help="time the removal step alone and print one JSON line")
    args = ap.parse_args()
    if args.removal_only:
        if args.package_root:
            sys.path.insert(0, os.path.abspath(args.package_root))
        print(json.dumps(removal_line(args.repeats)))
        return
    removal = None
    if args.parent_root:  # before this process opens the device: the processes of the comparison run alone
        removal = removal_compare(args.parent_root, args.repeats)
        removal["parent_commit"] = args.parent_commit
        print("removal:", removal, file=sys.stderr, flush=True)
    from glim_amd import api

    ctx = api.Context(0, 1)
    out = {
        "what": "resampling of resident clouds: device calls (synchronous, host wall clock, median) beside the route through the host, "
                "alternating in one process; one box, one run",
        "repeats": args.repeats, "device_name": ctx.device_info()["name"],
        "clouds": {str(n): cloud_lines(api, ctx, n, args.repeats) for n in (65536, 1048576)},
        "edit_remove_points_parent_vs_this": removal,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
