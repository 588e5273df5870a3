"""Wall time of the device iVox (glim_amd_ivox_*) and of the continuous-time GICP factor over it, next to the only route the library had
before: glim_amd_nn_index_create over the whole accumulated cloud once per frame, and the factor over that index.

Workload: the drive of tests/test_ivox.py (sweeps of a moving sensor through the shipped preprocessing, ~12 000 points each) accumulated until
the map holds ~300 000 points, or the walk ends (leaf 1.0, min_dist 0.05, lru_horizon 200, neighbour mode 1: config_odometry_ct.json).  Recorded, variants alternating in one process:
  insert            a ~12 000-point sweep / a raw 131 072-point sweep into a COPY of that map (rebuilt before every timed call, untimed)
  index_rebuild     glim_amd_nn_index_create over the map's points + one sweep (what a frame costs without the container)
  ct linearize / error of a ~12 000-point sweep over the map for neighbour modes 1 / 7 / 27, and over the rebuilt index
  frame             the whole frame of the frame-to-model loop: factor, 8 x (linearize + error), deskewed cloud, covariances, insert
Prints one JSON object; `--out` writes it too.

    python tools/ivox_time.py [--iters 30] [--out profiles/ivox/ivox_time.json]
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


def stats(t):
    t = np.array(t) * 1e6
    return {"p50_us": round(float(np.median(t)), 1), "p10_us": round(float(np.percentile(t, 10)), 1), "p90_us": round(float(np.percentile(t, 90)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--map-points", type=int, default=300000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from glim_amd import api, synth
    import ct_restatement as W

    ctx = api.Context(0, 1)
    scene = synth.Scene.default()
    # a long drive: the boustrophedon walk of the room, one sweep per step
    walk = synth.grid_trajectory(12, 12, spacing=1.5)
    sweeps, poses = [], []

    def new_map(mode=1):
        m = api.IncrementalVoxelMap(1.0, ctx=ctx)
        m.voxel_insertion_setting(min_dist=0.05, max_points=20)
        m.set_lru_horizon(200)
        m.set_neighbor_voxel_mode(mode)
        return m

    probe = new_map()
    for i in range(len(walk) - 3):
        p, t = synth.moving_scan(scene, walk[i], walk[i + 1], 64, 1024, duration=0.1, frame_id=200 + i)
        g = api.PointCloudGPU.preprocess(p.astype(np.float64), t, None, ctx=ctx)
        g.estimate_covariances(10)
        sweeps.append(g)
        poses.append(walk[i])
        probe.insert(g, walk[i])
        if probe.info()["num_points"] >= args.map_points:
            break
    base_info = probe.info()
    n_base = len(sweeps)
    # the sweep that arrives next (source of the factors, and the frame that gets inserted)
    i = n_base
    p, t = synth.moving_scan(scene, walk[i], walk[i + 1], 64, 1024, duration=0.1, frame_id=200 + i)
    src = api.PointCloudGPU.preprocess(p.astype(np.float64), t, None, ctx=ctx)
    src.estimate_covariances(10)
    X, Y = walk[i] @ W.expmap([0.002, -0.001, 0.003, 0.03, -0.02, 0.01]), walk[i + 1] @ W.expmap([-0.001, 0.002, -0.002, 0.02, 0.03, -0.01])
    values = {0: X, 1: Y}
    praw, _ = synth.moving_scan(scene, walk[i], walk[i + 1], 128, 1024, duration=0.1, frame_id=500)
    raw = api.PointCloudGPU.clone(praw, ctx=ctx)
    raw.find_neighbors(10, download=False)
    raw.estimate_covariances(10)

    # the accumulated cloud as the index route has to hold it: the map's own points and covariances (same target data for both routes)
    coords, counts, mp, mc = probe.download()
    keep = np.arange(mp.shape[1])[None, :] < counts[:, None]
    acc_xyz, acc_cov = mp[keep], mc[keep]
    acc = api.PointCloudGPU.clone(acc_xyz, covs=acc_cov, ctx=ctx)
    sx, sc, _ = src.download(covs=True, normals=False)
    Rw = walk[i][:3, :3]
    acc_plus = api.PointCloudGPU.clone(np.concatenate([acc_xyz, (sx @ Rw.T + walk[i][:3, 3]).astype(np.float32)]),
                                       covs=np.concatenate([acc_cov, np.einsum("ab,nbc,dc->nad", Rw, sc, Rw).astype(np.float32)]), ctx=ctx)

    res = {"note": "one box, not repeated", "map": base_info, "sweeps_in_map": n_base, "source_points": int(src.size()), "raw_points": int(raw.size()),
           "iters": args.iters}

    def rebuilt_map():
        m = new_map()
        for g, T in zip(sweeps, poses):
            m.insert(g, T)
        return m

    # ---- upkeep: insert vs index rebuild, alternating ----
    t_ins, t_raw, t_idx = [], [], []
    from glim_amd._lib import lib, check
    import ctypes as C

    for it in range(args.iters + 2):
        m = rebuilt_map()
        t0 = time.perf_counter()
        m.insert(src, walk[i])
        a = time.perf_counter() - t0
        m.close()
        m = rebuilt_map()
        t0 = time.perf_counter()
        m.insert(raw, walk[i])
        b = time.perf_counter() - t0
        m.close()
        h = C.c_void_p()
        t0 = time.perf_counter()
        check(lib().glim_amd_nn_index_create(acc_plus._h, 1.0, C.byref(h)), "glim_amd_nn_index_create")
        c = time.perf_counter() - t0
        lib().glim_amd_nn_index_destroy(h)
        if it >= 2:
            t_ins.append(a)
            t_raw.append(b)
            t_idx.append(c)
    res["insert_sweep"] = stats(t_ins)
    res["insert_raw_131072"] = stats(t_raw)
    res["index_rebuild_accumulated_cloud"] = dict(stats(t_idx), points=int(acc_plus.size()))

    # ---- the factor: modes 1 / 7 / 27 over the map and the exact search over the index, alternating ----
    maps = {mode: rebuilt_map() for mode in (1, 7, 27)}
    for mode, m in maps.items():
        m.set_neighbor_voxel_mode(mode)
    f = {f"ivox_mode{mode}": api.IntegratedCT_GICPFactor(0, 1, m, src, max_correspondence_distance=1.0) for mode, m in maps.items()}
    f["index"] = api.IntegratedCT_GICPFactor(0, 1, acc, src, max_correspondence_distance=1.0)
    tl = {k: [] for k in f}
    te = {k: [] for k in f}
    inl = {}
    n_it = max(args.iters * 4, 100)
    for it in range(n_it + 10):
        for k, fac in f.items():
            t0 = time.perf_counter()
            L = fac.linearize(values)
            a = time.perf_counter() - t0
            t0 = time.perf_counter()
            fac.error(values)
            b = time.perf_counter() - t0
            inl[k] = L["num_inliers"]
            if it >= 10:
                tl[k].append(a)
                te[k].append(b)
    res["ct_factor"] = {k: {"linearize": stats(tl[k]), "error": stats(te[k]), "num_inliers": inl[k]} for k in f}
    for fac in f.values():
        fac.close()

    # ---- the whole frame of the frame-to-model loop ----
    def frame(m):
        fac = api.IntegratedCT_GICPFactor(0, 1, m, src, max_correspondence_distance=1.0)
        Xi, Yi = X.copy(), Y.copy()
        for _ in range(8):
            L = fac.linearize({0: Xi, 1: Yi})
            H, b = W.full_system(L)
            dx = np.linalg.solve(H + 1e-6 * np.trace(H) / 12 * np.eye(12), -b)
            Xi, Yi = Xi @ W.expmap(dx[:6]), Yi @ W.expmap(dx[6:])
            fac.error({0: Xi, 1: Yi})
        d = fac.deskewed_cloud({0: Xi, 1: Yi}, local=True)
        d.estimate_covariances(10)
        fac.close()
        m.insert(d, Xi)
        d.close()

    t_frame = []
    for it in range(max(5, args.iters // 3) + 1):
        m = rebuilt_map()
        t0 = time.perf_counter()
        frame(m)
        if it:
            t_frame.append(time.perf_counter() - t0)
        m.close()
    res["frame_8_iterations_deskew_covariances_insert"] = stats(t_frame)
    res["insert_over_index_rebuild"] = round(res["insert_sweep"]["p50_us"] / res["index_rebuild_accumulated_cloud"]["p50_us"], 3)
    res["mode1_linearize_over_index_linearize"] = round(res["ct_factor"]["ivox_mode1"]["linearize"]["p50_us"] / res["ct_factor"]["index"]["linearize"]["p50_us"], 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
