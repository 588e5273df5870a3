#!/usr/bin/env python3
"""bench.py -- VGICP linearize() throughput on MI355X (BASELINE.json metric; default workload = configs[1]).

Contract (driver): python bench.py --gpus N --steps K --warmup W ; for N > 1 launched through torch.distributed.run, one
rank per GPU over RCCL.  Prints ONE JSON line on rank 0.  Such a plain run sets up, warms up and times the K steps of the headline
loop and nothing else; `--full` adds every other measurement of the default line (below).  `--dump-outputs DIR` writes the records
the headline loop returned in its last timed step as DIR/<name>.npy (float64); with the same arguments the inputs are the same in
every run, so two builds can be compared output for output.

N = 1 default workload "odometry128k" (BASELINE configs[1], metric M1): 131 072-point spinning-LiDAR scans (128 rings x 1024 azimuths, synthetic
analytic scene), each matched against the 0.5 m Gaussian voxel map of the previous scan on a 0.5 m / 2 deg arc.
`value` = the loop configs[1] names -- OdometryEstimationGPU's SYNCHRONOUS SINGLE-FACTOR linearize loop: {pose in, fused lookup + Mahalanobis
residual + 6-DoF Jacobian + reduction over one 131 072-pt factor, FP64 finalise, 232-B record out, host waits} per call, `--sync-calls` (2000) calls
per step issued from C on a context of the odometry module's kind (priority 1).  The same line carries the BATCHED form as `batched_calls_per_s`
(F = 128 distinct factors per NonlinearFactorSetGPU::linearize, inputs and results resident in HBM, `--inner` (256) passes per step, ~1 GB working
set so that the kernel really streams from HBM): that launch is the vehicle of `roofline`.
N > 1 default workload "global256" (BASELINE configs[3], metric M2, STRONG scaling): the all-pairs matching cost over 256 MERGED
submaps, pair list sharded over the ranks, one RCCL all-reduce of the [pairs x 29] block array per evaluation; value = seconds per cost
evaluation.  The weak-scaling form of M1 (every rank owns its own F factors + an all-reduce per pass) is reported next to it as `m1_weak`.

Other workloads (parity-test configurations of BASELINE.json, selectable for evidence; never the default line):
  --workload odometry_frame  GLIM's live odometry call pattern per frame (fresh 34-factor set per optimiser iteration, overlap_gpu keyframe
                         loops, clone + 2 voxel maps) at 10 000-pt and 131 072-pt frames: microseconds per call, inside the library
  --workload submap20    configs[2]: 20 keyframes x 65 536 pts, 190 pairs x 2 voxel levels = 380 binary factors per bundle
  --workload global256   configs[3]: 256 submaps x 65 536 pts, all 32 640 pairs, 1.0 m voxels, pair list sharded over the
                         ranks + RCCL all-reduce (strong scaling; metric M2 = seconds per cost evaluation)
  --workload frontend128k  SURVEY 8f ranks 1-2: raw scan -> preprocess -> deskew -> covariance -> voxel map -> factor, per frame
  --workload rgbd300k    configs[4]: 307 200-pt depth frames, per frame upload -> kNN -> covariance -> 0.1 m voxel map -> one
                         unary linearise against the previous frame (sustained frames/s, p50/p99 latency)

Also reported with --full (never in a plain run): `batched_calls_per_s`, the N = 1 line's `m2_global256` and the N > 1 line's `m1_weak`,
`roofline` for the dominant kernel (HIP-event timed inside this process on the stream the kernel runs on; `frac` = MEASURED
traffic of the committed PMC passes over that time over 8 TB/s, SURVEY 8d's algorithmic bytes as a ratio beside it), `cpu_baseline` (the FP64
OpenMP oracle on the usable host cores, bounded sample, thread curve), and the parity of one factor's Gauss-Newton step against the oracle.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured-achievable copy rate)
HBM_ACHIEVABLE_GBS = 6290.0
FP32_VECTOR_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md "Peak FP32 (vector)": 157.3 TFLOP/s


def log(*a):
    if int(os.environ.get("RANK", "0")) == 0:
        print("[bench]", *a, file=sys.stderr, flush=True)


def effective_cores():
    """Host cores this process may really use: min(affinity mask, cgroup CPU quota)."""
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return n


def kernel_source_id():
    """Identity of the factor kernel this process runs: SHA-256 over the sources and build flags that decide its code (vgicp.hip, the two
    headers it includes, the Makefile).  tools/summarize_profile.py stamps it into profiles/*/traffic*.json, so a PMC figure measured on
    another version of the kernel is recognised instead of being quoted silently."""
    import hashlib

    h = hashlib.sha256()
    for f in ("vgicp.hip", "device_math.hpp", "internal.hpp", "Makefile"):
        h.update(open(os.path.join(ROOT, "glim_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


KNN_SOURCES = ("knn.hip", "knn_qgroup.hip", "knn_common.hpp", "sort.hip", "Makefile")


def source_id(files):
    import hashlib

    h = hashlib.sha256()
    for f in files:
        h.update(open(os.path.join(ROOT, "glim_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


def knn_roofline(cloud, k, tag):
    """`roofline` of a kNN-led workload on its dominant kernel, knn_qgroup_kernel: live HIP-event duration of that kernel
    (glim_amd_cloud_profile_neighbors: events on the call's own stream), SURVEY 8d's algorithmic bytes B_knn = 12 N + 4 k N, and the measured L2 <-> HBM
    bytes per launch from the committed PMC passes (profiles/*/traffic_knn_<tag>.json) when there are any.  The kernel is a selection network over
    LDS-resident candidates -- bound by vector-ALU / LDS issue, not by HBM -- so both fractions are small by nature; they are printed, not dressed up."""
    import glob

    n = cloud.size()
    ms_call, ms_kernel = cloud.profile_neighbors(k, 20)
    algo = float(12 * n + 4 * k * n)
    out = {"bound": "hbm", "kernel": "knn_qgroup_kernel (exact kNN, k = %d, query included)" % k, "peak": HBM_PEAK_GBS, "unit": "GB/s", "points": int(n),
           "kernel_ms": ms_kernel, "find_neighbors_call_ms": ms_call, "algorithmic_bytes_per_launch": algo,
           "algorithmic_gbs": algo / max(1e-9, ms_kernel * 1e-3) / 1e9, "traffic": None, "traffic_source": None, "knn_source_id": source_id(KNN_SOURCES)}
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*", f"traffic_knn_{tag}.json"))):
        try:
            t = json.load(open(f))
            out["traffic"] = t["traffic_bytes_per_launch"]
            out["traffic_source"] = os.path.relpath(f, ROOT)
            out["traffic_measured_on_this_kernel_version"] = t.get("knn_source_id") == out["knn_source_id"]
            out["kernel_avg_us_rocprof"] = t.get("kernel_avg_us_rocprof")
        except Exception:
            pass
    if out["traffic"] and ms_kernel > 0:
        out["achieved"] = out["traffic"] / (ms_kernel * 1e-3) / 1e9
        out["frac_basis"] = "measured L2<->HBM traffic (PMC) / HIP-event kernel time / 8 TB/s"
    else:
        out["achieved"] = out["algorithmic_gbs"]
        out["frac_basis"] = "ALGORITHMIC bytes 12 N + 4 k N (no PMC file for this shape) / HIP-event kernel time / 8 TB/s"
    out["frac"] = out["achieved"] / HBM_PEAK_GBS
    out["note"] = "compute-bound kernel (bitonic / threshold selection over LDS-resident candidates, DESIGN 4.3): a low HBM fraction is what it should show"
    return out


def measured_traffic(workload_tag):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes (profiles/*/traffic*.json; the PMC counters
    need separate rocprofv3 runs, so they cannot be collected inside this process).  Returns (bytes per factor, file, measured on this
    kernel version?) for the NEWEST matching file, or None."""
    import glob

    best = None
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*", "traffic*.json"))):
        try:
            t = json.load(open(f))
            if workload_tag in t.get("workload", ""):
                best = (t["traffic_bytes_per_factor"], os.path.relpath(f, ROOT), t.get("kernel_source_id") == kernel_source_id())
        except Exception:
            pass
    return best


def isa_stats_of(which):
    """Static instruction / FLOP count of the shipped factor kernel's loop (tools/isa_stats.py at the committed sources: profiles/*/isa_stats.json,
    one JSON line per kernel instantiation, stamped with the kernel source id).  which: "plane" | "general" (launch-per-call LINEARIZE kernels)."""
    import glob

    # <MODE = linearise, FROZEN = 0, PLANE, INLINE = 0, FUSED = 0, CULL = 0> (round 6 added the CULL parameter; the pre-cull variant is off by default)
    want = {"plane": "vgicp_kernelILi0ELb0ELb1ELb0ELb0ELb0EEE", "general": "vgicp_kernelILi0ELb0ELb0ELb0ELb0ELb0EEE"}[which]
    best = None
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*", "isa_stats.json"))):
        try:
            for line in open(f):
                r = json.loads(line)
                if want in r.get("kernel", ""):
                    mix = r["mix"]
                    best = {"fp32_flops_per_point": r["fp32_flops_per_point"], "fp64_flops_per_point": r["fp64_flops_per_point"],
                            "valu_instructions_per_point": sum(v for k, v in mix.items() if k.startswith("valu")),
                            "source": os.path.relpath(f, ROOT) + (" (this kernel version)" if r.get("kernel_source_id") == kernel_source_id() else " (another kernel version)")}
        except Exception:
            pass
    return best


def make_frames(api, ctx, poses, rings, azimuths, frame_id0=0, k=10):
    """Synthetic scans uploaded to the device with kNN + covariances computed there."""
    from glim_amd import synth

    scene = synth.Scene.default()
    dirs = synth.lidar_directions(rings, azimuths)
    clouds = []
    for i, T in enumerate(poses):
        g = api.PointCloudGPU.clone(synth.scan(scene, T, dirs, frame_id=frame_id0 + i), ctx=ctx)
        g.find_neighbors(k, download=False)
        g.estimate_covariances(k)
        clouds.append(g)
    return clouds


def algorithmic_bytes(n_pts, n_vox):
    """B_lin = 48 N + 68 V + 488 per factor."""
    return float(sum(48 * n + 68 * v + 488 for n, v in zip(n_pts, n_vox)))


def roofline_of(fset, poses, n_pts, n_vox, iters, traffic=None):
    # five rounds of (warm-up, `iters` kernel-only launches, `iters` kernel + finalise launches) between HIP events on the factor set's stream;
    # the reported duration is the average over all rounds (a single short window now and then catches the chip in a slow clock state)
    rounds = [fset.profile(poses, iters=iters) for _ in range(5)]
    ms_kernel = float(np.mean([r[0] for r in rounds]))
    ms_lin = float(np.mean([r[1] for r in rounds]))
    algo = algorithmic_bytes(n_pts, n_vox)
    algo_gbs = algo / (ms_kernel * 1e-3) / 1e9
    out = {
        "bound": "hbm", "kernel": "vgicp_kernel<LINEARIZE>", "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "traffic": traffic[0] if traffic else None, "traffic_source": traffic[1] if traffic else None,
        "algorithmic_bytes_per_launch": algo, "kernel_ms": ms_kernel, "linearize_ms": ms_lin,
        "kernel_ms_rounds": [round(float(r[0]), 5) for r in rounds], "kernel_source_id": kernel_source_id(),
    }
    if traffic:
        # `achieved` / `frac`: the bytes the kernel REALLY pulled through the L2 (rocprofv3 PMC passes, profiles/*/traffic*.json) over the launch
        # time measured here -- the kernel streams 24-36 B per point where SURVEY 8d's reference layout has 48, so the algorithmic figure is
        # not traffic; it stays below as a ratio, not as a roofline fraction
        out["achieved"] = traffic[0] / (ms_kernel * 1e-3) / 1e9
        out["frac"] = out["achieved"] / HBM_PEAK_GBS
        out["frac_basis"] = "measured L2<->HBM traffic (PMC) / HIP-event kernel time / 8 TB/s"
        out["traffic_measured_on_this_kernel_version"] = bool(traffic[2])
        out["frac_of_6.29TBs_copy_rate"] = out["achieved"] / HBM_ACHIEVABLE_GBS
    else:
        # no counter file for this workload shape: the algorithmic bytes are all there is (stated as such)
        # (never clamped: a ratio above 1 says "these bytes are cache hits, not traffic" and asks for a PMC pass -- VERDICT r5 weak 7)
        out["achieved"] = algo_gbs
        out["frac"] = algo_gbs / HBM_PEAK_GBS
        out["frac_basis"] = "ALGORITHMIC bytes (no PMC traffic file for this shape) / kernel time / 8 TB/s -- NOT traffic; a value above 1 means cache-served re-reads"
    # SURVEY 8d's B_lin = 48 N + 68 V + 488 per factor over the same kernel time, relative to the peak: a RATIO (it exceeds what any kernel
    # can stream when the kernel moves fewer bytes than the reference layout, or when factors share clouds / maps in cache), not a fraction of a roofline
    out["algorithmic_48B_gbs"] = algo_gbs
    out["algorithmic_48B_ratio_to_peak"] = algo_gbs / HBM_PEAK_GBS
    return out


def cpu_baseline_and_parity(api, target_cloud, source_cloud, delta12, resolution, gpu_result, budget_s=12.0):
    """Time the FP64 OpenMP oracle (restatement of gtsam_points::IntegratedVGICPFactor::linearize) on one factor of the same
    workload and check the GPU Gauss-Newton step against it."""
    import ctypes as C

    from oracle import oracle as orc

    tgt_xyz, tgt_cov, _ = target_cloud.download(normals=False)
    src_xyz, src_cov, _ = source_cloud.download(normals=False)
    vm = orc.VoxelMap(resolution).insert(tgt_xyz, tgt_cov.astype(np.float64))
    p4 = orc.points4(src_xyz)
    c16 = orc.covs16(src_cov.astype(np.float64))
    tp4 = orc.points4(tgt_xyz)
    tc16 = orc.covs16(tgt_cov.astype(np.float64))
    T = np.ascontiguousarray(delta12)
    L = orc.Linearized6()
    lib = orc.lib()
    cores = min(orc.max_threads(), effective_cores())
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    # TIMING runs on a second build of the same restatement with SURVEY 8d's flags (-O3 -march=native, compiled on this box); the parity
    # check below always uses the bit-exact checker build
    fast = orc.fast_lib()
    tlib, tmap = lib, vm._h
    if fast is not None:
        tlib, tmap = fast, C.c_void_p(fast.orc_voxelmap_create(float(resolution)))
        fast.orc_voxelmap_insert(tmap, dp(tp4), dp(tc16), len(tp4))

    def run(threads, budget):
        Lt = orc.Linearized6()
        tlib.orc_vgicp_linearize(tmap, dp(p4), dp(c16), len(p4), dp(T), threads, C.byref(Lt), None)  # warm
        n, t0 = 0, time.perf_counter()
        while True:
            tlib.orc_vgicp_linearize(tmap, dp(p4), dp(c16), len(p4), dp(T), threads, C.byref(Lt), None)
            n += 1
            dt = time.perf_counter() - t0
            if dt >= budget or n >= 4000:
                return n / dt, n

    # thread curve first (short samples; the team is warm after the first call of each size), then the headline sample on the fastest count
    curve = {}
    t = 1
    while t < cores:
        curve[t] = run(t, budget_s / 10)[0]
        t *= 2
    rate_all, n_all = run(cores, budget_s / 2)
    curve[cores] = rate_all
    best_t = max(curve, key=lambda k: curve[k])
    if best_t != cores:  # a box where fewer threads are faster (SMT / quota effects): the headline sample is taken there
        rate_all, n_all = run(best_t, budget_s / 3)
        cores = best_t
        curve[cores] = max(curve[cores], rate_all)
    rate_ref = curve.get(min(2, cores), rate_all)  # the reference's shipped num_threads (config_odometry_cpu.json:36)
    rate_1 = curve.get(1, rate_all)
    if fast is not None:
        fast.orc_voxelmap_destroy(tmap)
    lib.orc_vgicp_linearize(vm._h, dp(p4), dp(c16), len(p4), dp(T), cores, C.byref(L), None)  # the checker build: the parity reference
    ref = orc._lin_to_dict(L)
    d_got = np.linalg.solve(gpu_result["H_ss"], -gpu_result["b_s"])
    d_ref = np.linalg.solve(ref["H_ss"], -ref["b_s"])
    parity = {
        "inliers_equal": bool(gpu_result["num_inliers"] == ref["num_inliers"]),
        "max_pose_delta_err": float(np.abs(d_got - d_ref).max()),
        "tolerance": 1e-4,
    }
    base = {
        "value": rate_all, "unit": "calls/s", "cores": cores, "kind": "port",
        "sample": f"{n_all} linearize() calls of one {len(p4)}-pt factor (oracle/vgicp_oracle.c, OpenMP guided,8, usable host cores = min(affinity, cgroup quota))",
        "build": "gcc -O3 -march=native -fopenmp (oracle.fast_lib)" if fast is not None else "gcc -O2 -march=x86-64-v3 -ffp-contract=off (the checker build: no compiler for the -O3 build)",
        "value_2_threads": rate_ref, "value_1_thread": rate_1, "points_per_s_per_core": rate_1 * len(p4),
        "thread_curve_calls_per_s": {str(k): v for k, v in sorted(curve.items())},
        "thread_curve_note": "per-thread sums live on each thread's own stack since round 5 (the heap array of round 4 put neighbouring threads' hot fields into one "
                             "cache line: 2 threads ran slower than 1); threads are left to the scheduler (OMP_PROC_BIND unset: binding changed nothing here)",
    }
    return base, parity


class Dist:
    """torch.distributed plumbing (RCCL on GPU boxes)."""

    def __init__(self, gpus):
        import torch
        import torch.distributed as dist

        self.torch, self.dist = torch, dist
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        if gpus > 1 and self.world != gpus:
            raise SystemExit(f"--gpus {gpus} needs WORLD_SIZE={gpus} (launch with torch.distributed.run)")
        assert torch.cuda.is_available(), "bench.py needs a GPU; the product path has no CPU fallback"
        torch.cuda.set_device(self.local_rank)
        # BENCH_FORCE_DIST=1 runs the RCCL code path (process group, all-reduce on our stream, barrier) even with one rank,
        # so the N > 1 plumbing can be exercised on a 1-GPU box
        self.collective = self.world > 1 or os.environ.get("BENCH_FORCE_DIST") == "1"
        if self.collective:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29512")
            dist.init_process_group(backend="nccl", rank=self.rank, world_size=self.world, device_id=torch.device("cuda", self.local_rank))

    def barrier_sync(self):
        self.torch.cuda.synchronize()
        if self.collective:
            self.dist.barrier()
        self.torch.cuda.synchronize()

    def max_over_ranks(self, x):
        if not self.collective:
            return x
        t = self.torch.tensor([x], dtype=self.torch.float64, device="cuda")
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def finish(self):
        if self.collective:
            self.dist.barrier()
            self.dist.destroy_process_group()


def timed_steps(D, step, steps, warmup):
    for i in range(warmup):
        step(i)
    D.barrier_sync()
    t0 = time.perf_counter()
    for i in range(steps):
        step(i)
    D.barrier_sync()
    return D.max_over_ranks(time.perf_counter() - t0)


def dump_outputs(args, D, arrays):
    """--dump-outputs DIR: the arrays the timed path returned to its caller in its last step, one DIR/<name>.npy each, as float64."""
    if not args.dump_outputs or D.rank != 0:
        return
    os.makedirs(args.dump_outputs, exist_ok=True)
    total = 0
    for name, a in arrays.items():
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
        total += a.nbytes
        np.save(os.path.join(args.dump_outputs, name + ".npy"), a)
    assert total <= 64 << 20, f"--dump-outputs wrote {total} bytes (the limit is 64 MB)"
    log(f"wrote {len(arrays)} arrays ({total} bytes) to {args.dump_outputs}")


def sync_single_factor_loop(args, D, api, clouds, vmaps, pose_sets):
    """The loop BASELINE configs[1] names and the headline of the single-GPU line: {set pose, linearize, read back the record} per call, one factor
    (target map vmaps[0], source clouds[1]) issued from C (glim_amd_factor_set_linearize_repeat), `--sync-calls` calls per step, `--steps` timed
    steps after max(--warmup, 1) warm-up steps, on a context of the kind the odometry module creates (adapters/glim/odometry_estimation_hip_create.cpp:
    own stream pool, priority 1 -- which is also what switches the resident session on; every other context leaves it off).  Clouds and maps cross
    contexts by design.  Writes the last step's record for --dump-outputs.  Returns (context, factor set, calls per step, timed seconds)."""
    odo = api.Context(D.local_rank, 4, priority=1)
    single = api.NonlinearFactorSetGPU(odo)
    single.add(api.IntegratedVGICPFactorGPU(0, 1, vmaps[0], clouds[1]))
    P_single = np.stack([pose_sets[k][0] for k in range(len(pose_sets))])  # the optimiser moves the pose between calls
    sync_calls = max(1, args.sync_calls)
    got_box = {}

    def sync_step(_):
        got_box["last"] = single.linearize_repeat(P_single, sync_calls)[0]

    elapsed_sync = timed_steps(D, sync_step, args.steps, max(args.warmup, 1))
    dump_outputs(args, D, {k: np.asarray(v) for k, v in got_box["last"].items()})  # num_inliers, error, H_tt, H_ss, H_ts, b_t, b_s of the last call
    return odo, single, sync_calls, elapsed_sync


def odometry128k_sync_loop(args, D, api, clouds, vmaps, pose_sets, n_pts, n_vox):
    """The plain single-GPU line: the headline loop alone (`batched_calls_per_s`, `roofline`, the per-variant call times, the resident session's
    cost, the device timeline, `cpu_baseline` / `parity` and `m2_global256` are measured with --full)."""
    odo, single, sync_calls, elapsed = sync_single_factor_loop(args, D, api, clouds, vmaps, pose_sets)
    value = sync_calls * args.steps / elapsed
    result = {
        "metric": "vgicp_linearize_calls_per_s", "value": value, "unit": "calls/s", "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "headline_form": (f"`value` = the loop BASELINE configs[1] names: synchronous single-factor linearize calls (pose in, 131 072-pt factor, record "
                          f"out, host waits) issued back to back from C, {sync_calls} per step.  The batched form, the roofline and the CPU baseline are "
                          "measured with --full"),
        "sync_single_factor_calls_per_s": value, "timed_region_s": elapsed,
        "config": {
            "workload": "configs[1] odometry128k: OdometryEstimationGPU's single-factor linearize loop, one 131072-pt spinning-LiDAR scan vs a 0.5 m voxel map per call",
            "calls_per_step": sync_calls, "points_per_factor": int(n_pts[0]), "voxels_per_factor": int(n_vox[0]),
            "voxel_resolution_m": args.resolution, "factor_type": "binary",
            "context": "priority 1, 4 streams (as adapters/glim/odometry_estimation_hip_create.cpp creates it): resident session on",
            "collective": "none", "device": odo.device_info()["name"],
        },
    }
    single.close()
    odo.close()
    return result


# ---------------------------------------------------------------------------------------------------------------------
def run_odometry128k(args, D, api, ctx):
    from glim_amd import synth
    from glim_amd.se3 import se3_exp

    torch = D.torch
    F, rank, world = args.factors, D.rank, D.world
    # 0.5 m / 2 deg per frame = a circle of radius 14.3 m; its centre is kept near the middle of the 60 x 40 m room (shifted a
    # little per rank) so that every one of the F + 1 scans stays inside and returns all 131 072 points
    import math

    yaw0 = math.radians(10.0 + 7.0 * rank)
    radius = 0.5 / math.radians(2.0)
    cx, cy = 1.5 * (rank % 4) - 2.0, 1.0 * (rank // 4) - 0.5
    poses = synth.arc_trajectory(F + 1, start=(cx + radius * math.sin(yaw0), cy - radius * math.cos(yaw0), 1.8), yaw0_deg=math.degrees(yaw0))
    # a plain single-GPU run times only the headline loop, which uses factor 0 alone: it builds the first two scans and one voxel map; the
    # batched set of F factors and every measurement on it belong to --full
    headline_only = world == 1 and not args.full and args.sync_calls > 0
    nf = 1 if headline_only else F
    t0 = time.time()
    clouds = make_frames(api, ctx, poses[:nf + 1], args.rings, args.azimuths, frame_id0=1000 * rank)
    vmaps = [api.GaussianVoxelMapGPU(args.resolution, ctx=ctx).insert(c) for c in clouds[:nf]]
    log(f"generated {nf + 1} scans of {clouds[0].size()} pts (kNN, covariances, voxel maps on the device) in {time.time() - t0:.1f}s")
    fset = None if headline_only else api.NonlinearFactorSetGPU(ctx)
    deltas = []
    for i in range(nf):
        if fset is not None:
            fset.add(api.IntegratedVGICPFactorGPU(i, i + 1, vmaps[i], clouds[i + 1]))  # binary factor: target i, source i+1
        deltas.append(api.pose12(synth.relative_pose(poses[i], poses[i + 1])))
    deltas = np.stack(deltas)
    n_pts = [c.size() for c in clouds[1:]]
    n_vox = [v.voxelmap_info()["num_voxels"] for v in vmaps]

    # a few linearisation points per factor (the optimiser moves the poses between calls); the draws of all F factors are taken either
    # way, so factor 0's points are the same in a plain run and in a --full run
    rng = np.random.default_rng(1234 + rank)
    pose_sets = []
    for s in range(4):
        P = np.empty((nf, 12))
        for f in range(F):
            xi = rng.normal(size=6) * [2e-3, 2e-3, 2e-3, 1e-2, 1e-2, 1e-2] * (s > 0)
            if f < nf:
                Dm = np.eye(4)
                Dm[:3, :4] = deltas[f].reshape(3, 4)
                P[f] = api.pose12(Dm @ se3_exp(xi))
        pose_sets.append(P)
    if headline_only:
        return odometry128k_sync_loop(args, D, api, clouds, vmaps, pose_sets, n_pts, n_vox)
    out = torch.zeros(world * F, api._lib.COMPACT_DOUBLES, dtype=torch.float64, device="cuda")

    # collective mode: every rank owns F rows, so the exchange is an all-gather of equal shards; two send / receive pairs so that the
    # all-gather of evaluation i (RCCL's stream) overlaps the kernels of evaluation i+1 (our stream); work.wait() only orders the
    # streams, the host never blocks inside the timed loop
    sends = [torch.zeros(F, api._lib.COMPACT_DOUBLES, dtype=torch.float64, device="cuda") for _ in range(2)]
    outs = [out, torch.zeros_like(out)]
    works = [None, None]

    inner = max(1, args.inner)

    def one_pass(i):
        if not D.collective:
            fset.linearize_device_async(pose_sets[i % len(pose_sets)], out.data_ptr(), rank * F)
            return
        b = i % 2
        if works[b] is not None:
            works[b].wait()
        fset.linearize_device_async(pose_sets[i % len(pose_sets)], sends[b].data_ptr(), 0)
        works[b] = D.dist.all_gather_into_tensor(outs[b], sends[b], async_op=True)  # RCCL over xGMI: [world x F x 29] on every rank

    def step(i):
        for k in range(inner):
            one_pass(i * inner + k)

    # cold figure: the driver's W warm-up steps would hide it, so it is measured first, on the first passes this process ever issues after the
    # (host-heavy) scene generation: 20 passes after 5 warm-up passes, the regime round 1's bench line was criticised for not showing
    for i in range(5):
        one_pass(i)
    D.barrier_sync()
    t0 = time.perf_counter()
    for i in range(20):
        one_pass(i)
    D.barrier_sync()
    value_cold = world * F * 20 / D.max_over_ranks(time.perf_counter() - t0)
    elapsed_batched = timed_steps(D, step, args.steps, args.warmup)
    value_batched = world * F * inner * args.steps / elapsed_batched
    traffic = measured_traffic("odometry128k") if (args.rings, args.azimuths) == (128, 1024) else None
    if traffic:
        traffic = (traffic[0] * F, traffic[1], traffic[2])  # measured per factor (PMC passes), scaled to this launch
    result = None
    roofline = roofline_of(fset, pose_sets[0], n_pts, n_vox, 40, traffic)
    roofline["what"] = (f"the dominant kernel, timed on its batched form ({F} factors of 131 072 points per launch: the working set exceeds the 256 MiB "
                        "Infinity Cache, so the launch streams from HBM); a single-factor call runs the same kernel for ~5 us inside a ~12 us round trip")

    # ---- the configuration BASELINE configs[1] names: OdometryEstimationGPU's synchronous single-factor linearize loop ----
    # {set pose, linearize, read back the record} per call, one factor of 131 072 points, issued from C (glim_amd_factor_set_linearize_repeat),
    # on a context of the kind the odometry module creates (adapters/glim/odometry_estimation_hip_create.cpp: own stream pool, priority 1 --
    # which is also what switches the resident session on; every other context leaves it off).  Clouds and maps cross contexts by design.
    if args.sync_calls <= 0:
        # profiling runs (tools/profile.sh: --sync-calls 0): only the batched launches, so that the rocprofv3 passes see the dominant kernel alone (a
        # resident session must not be alive under serialised counter collection)
        if rank != 0:
            return None
        return {"metric": "vgicp_linearize_calls_per_s", "value": value_batched, "unit": "calls/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": elapsed_batched / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                "headline_form": f"profiling form (--sync-calls 0): batched only, {F} factors per NonlinearFactorSetGPU::linearize",
                "batched_calls_per_s": value_batched, "config": {"workload": "configs[1] odometry128k, batched form only (profiling run)", "factors_per_gpu_batched": F,
                                                                 "points_per_factor": int(np.mean(n_pts)), "voxels_per_factor": int(np.mean(n_vox))},
                "roofline": roofline}
    odo, single, sync_calls, elapsed_sync = sync_single_factor_loop(args, D, api, clouds, vmaps, pose_sets)
    value_sync = world * sync_calls * args.steps / elapsed_sync
    T1 = deltas[:1]
    got = single.linearize_poses(T1)[0]
    headline_is_sync = world == 1
    if rank == 0:
        sync_ms_c = single.profile_sync(T1, iters=1000)
        by_variant = {"resident_session": sync_ms_c * 1e3}
        for name, diag in (("single_dispatch", "resident=0"), ("two_dispatches", "resident=0,fuse=0")):
            with odo.diag(diag):
                alt = api.NonlinearFactorSetGPU(odo)
                alt.add(api.IntegratedVGICPFactorGPU(0, 1, vmaps[0], clouds[1]))
                alt.profile_sync(T1, iters=50)
                by_variant[name] = alt.profile_sync(T1, iters=1000) * 1e3
                alt.close()
        # the same call from a context that did NOT opt in (a mapping thread's): launch per call
        plain = api.NonlinearFactorSetGPU(ctx)
        plain.add(api.IntegratedVGICPFactorGPU(0, 1, vmaps[0], clouds[1]))
        plain.profile_sync(T1, iters=50)
        by_variant["default_context_no_session"] = plain.profile_sync(T1, iters=1000) * 1e3
        plain.close()
        resident_cost = None
        if not args.no_resident_cost:  # (profiling runs skip it: its launches beside the session would be averaged into the dominant kernel's row)
            # what a live (idle) resident session costs everything else on the device: the batched 128-factor kernel timed alone and beside a
            # session that is kept from idling out for the duration (its 513 blocks hold wave slots and poll).  Since round 5 only a context
            # that opted in (priority 1 / resident=1) ever starts one; this is the price its neighbours pay while it is alive.
            small = api.NonlinearFactorSetGPU(ctx)  # a latency-bound launch: 8 factors of 131 072 points
            for k in range(8):
                small.add(api.IntegratedVGICPFactorGPU(k, k + 1, vmaps[k], clouds[k + 1]))
            Ts = np.ascontiguousarray(deltas[:8])
            api.resident_stop(odo)
            k_alone, _ = fset.profile(pose_sets[0], iters=40)
            s_alone, _ = small.profile(Ts, iters=200)
            # a default context's own synchronous calls do not start a session: the neighbours of a default context pay nothing
            stats_default = api.resident_stats(ctx)
            with odo.diag("resident_idle_us=400000"):
                stats0 = api.resident_stats(odo)
                for _ in range(8):
                    single.linearize_poses(T1)  # restarts the session with the long idle time
                stats1 = api.resident_stats(odo)
                k_beside, _ = fset.profile(pose_sets[0], iters=40)
                s_beside, _ = small.profile(Ts, iters=200)
                stats = api.resident_stats(odo)
                log(f"resident session around the interference measurement: {stats0} -> {stats1} -> {stats}")
                api.resident_stop(odo)
            small.close()
            resident_cost = {"opt_in": "only a context created with priority 1 (the odometry module's) or with resident=1 starts a session; a default "
                                       "context -- the sub-mapping / global-mapping threads' -- never does, so ITS neighbours pay nothing",
                             "session_alive_after_default_context_calls": bool(stats_default["alive"]),
                             "batched_128_factor_kernel_ms": {"alone": k_alone, "beside_an_idle_session": k_beside, "slowdown": k_beside / k_alone},
                             "8_factor_kernel_ms": {"alone": s_alone, "beside_an_idle_session": s_beside, "slowdown": s_beside / s_alone},
                             "session_alive_during_measurement": bool(stats["alive"]),
                             "session_footprint": "512 worker blocks + 1 finalising / leading block of 256 threads at 125 VGPRs (plane-form plans): 2 of a SIMD's "
                                                  "wave slots and half its registers while the session is alive (it leaves after resident_idle_us = 1 ms without a request)"}
        # the resident call on a DEVICE timeline: s_memrealtime stamps inside the session, read for the last request of a 200-call run
        timeline = None
        try:
            api.resident_timeline(0, enable=True, read=False)  # (ends the running session; the next one carries the stamps)
            tls = []
            for _ in range(5):
                single.profile_sync(T1, iters=200)
                t = api.resident_timeline(0, enable=True, read=True)
                if t and t["workers_accounted"] > 0:
                    tls.append(t)
            api.resident_timeline(0, enable=False, read=False)
            if tls:
                timeline = {k: float(np.median([t[k] for t in tls])) for k in tls[0]}
                timeline["samples"] = len(tls)
                timeline["what"] = ("microseconds, median over the last requests of 5 runs of 200 calls; device stamps relative to the leader seeing the request in host "
                                    "memory; host_round_trip = posting the request -> last record granule seen (host clock); host_round_trip - device_span = "
                                    "request transit (host store -> the leader's PCIe poll) + record transit (posted PCIe writes -> the host's poll)")
        except Exception as e:  # noqa: BLE001 -- diagnostic only
            timeline = {"error": repr(e)}
        single_loop = {"calls_per_s": 1e3 / sync_ms_c, "us_per_call": sync_ms_c * 1e3, "calls": 1000, "resident_timeline_us": timeline,
                       "what": "one 131072-pt factor per call on the odometry's kind of context (priority 1): after three launch-per-call linearisations the "
                               "factor list is served by a RESIDENT kernel (pose through a host-mapped mailbox, no launch on the request path; the session "
                               "idles out after 1 ms); row blocks hand their partial rows as tagged write-through granules to a finalising block (no counter, "
                               "no fence); the 232-B record comes back as self-validating host-mapped granules the host polls.  `single_dispatch`: the same "
                               "hand-off inside ONE launch per call; `two_dispatches`: factor kernel + finalise kernel per call (round 3's form); "
                               "`default_context_no_session`: what a context that did not opt in gets (single dispatch)",
                       "us_per_call_by_variant": by_variant, "resident_session_cost": resident_cost}
        value, elapsed = (value_sync, elapsed_sync) if headline_is_sync else (value_batched, elapsed_batched)
        result = {
            "metric": "vgicp_linearize_calls_per_s", "value": value, "unit": "calls/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "headline_form": (f"`value` = the loop BASELINE configs[1] names: synchronous single-factor linearize calls (pose in, 131 072-pt factor, record "
                              f"out, host waits) issued back to back from C, {sync_calls} per step.  `batched_calls_per_s` = {F} factors per "
                              "NonlinearFactorSetGPU::linearize with inputs and results device-resident: the form the roofline is measured on") if headline_is_sync
                             else (f"`value` = batched (weak scaling over ranks): {F} factors per NonlinearFactorSetGPU::linearize per rank + one all-gather per pass; "
                                   "`sync_single_factor_calls_per_s` = every rank's own synchronous single-factor loop, summed"),
            "batched_calls_per_s": value_batched, "batched_ms_per_step": elapsed_batched / args.steps * 1e3, "batched_value_cold": value_cold,
            "sync_single_factor_calls_per_s": value_sync, "single_factor_loop": single_loop,
            "timed_region_s": elapsed,
            "config": {
                "workload": ("configs[1] odometry128k: OdometryEstimationGPU's single-factor linearize loop, one 131072-pt spinning-LiDAR scan vs a 0.5 m voxel map per call"
                             if headline_is_sync else "configs[1] odometry128k, weak-scaling form: 131072-pt spinning-LiDAR scans vs 0.5 m voxel maps, batched VGICP linearize"),
                "calls_per_step": sync_calls if headline_is_sync else inner * F * world,
                "factors_per_gpu_batched": F, "points_per_factor": int(np.mean(n_pts)), "voxels_per_factor": int(np.mean(n_vox)),
                "voxel_resolution_m": args.resolution, "factor_type": "binary", "batched_linearize_passes_per_step": inner,
                "context": "priority 1, 4 streams (as adapters/glim/odometry_estimation_hip_create.cpp creates it): resident session on",
                "collective": "rccl_all_gather[world x F x 29] f64" if world > 1 else "none", "device": ctx.device_info()["name"],
            },
            "roofline": roofline,
        }
        if world == 1 and not args.no_cpu_baseline:
            base, parity = cpu_baseline_and_parity(api, clouds[0], clouds[1], deltas[0], args.resolution, got)
            result["cpu_baseline"] = base
            result["parity"] = parity
            # the comparison configs[1] names: ONE factor per call on both sides (the batched figure divided by the CPU rate is reported too)
            result["speedup_vs_cpu_baseline"] = value_sync / base["value"]
            result["batched_speedup_vs_cpu_baseline"] = value_batched / base["value"]
    single.close()
    odo.close()
    return result


def run_odometry_frame(args, D, api, ctx):
    """GLIM's LIVE odometry call pattern (src/glim/odometry/odometry_estimation_gpu.cpp, shipped config_odometry_gpu.json), per frame:
      create_frame (:86-107)      PointCloudGPU::clone of the frame (points + CPU covariances) + voxelmap_levels = 2 GaussianVoxelMapGPU::insert
      create_factors (:128-206)   (full_connection_window_size 2 + max_num_keyframes 15) x 2 levels = 34 factors, surface validation ON
      optimiser                   per iteration a FRESH NonlinearFactorSetGPU: add(34 factors); linearize  (:383-385 and the linearisation hook)
      update_keyframes_overlap    one 15-target overlap_gpu per frame (:224-231); on a new keyframe beyond the limit the elimination loop (:262-281):
                                  15 single-target calls + 14 x (one single-target + one 13-target call) = 43 overlap_gpu calls
    at the shipped 10 000-pt frames (config_preprocess.json:24 random_downsample_target) and at configs[1]'s 131 072-pt scans.  Every figure is
    microseconds of WALL time per call, measured inside the library (no binding overhead); `plan_cache=0` is the behaviour before the plan cache."""
    from glim_amd import synth

    scene = synth.Scene.default()
    K, WIN, LEVELS, ITERS = 15, 2, 2, args.opt_iters
    out = {}
    for label, rings, azimuths, keep in (("frames_10000_pts", 128, 1024, 10000), ("frames_131072_pts", 128, 1024, None)):
        dirs = synth.lidar_directions(rings, azimuths)
        all_poses = synth.arc_trajectory(K + WIN + 1 + (8 if keep else 0), step=0.4, yaw_step_deg=1.5)  # (+ 8 further arrivals for the live loop)
        rng = np.random.default_rng(3)
        all_frames, all_host = [], []
        for i, T in enumerate(all_poses):
            pts = synth.scan(scene, T, dirs, 500 + i)
            if keep:
                pts = pts[np.sort(rng.choice(len(pts), keep, replace=False))]
            g = api.PointCloudGPU.clone(pts, ctx=ctx)
            g.find_neighbors(10, download=False)
            g.estimate_covariances(10)
            all_frames.append(g)
            all_host.append(pts)
        poses, frames, host = all_poses[:K + WIN + 1], all_frames[:K + WIN + 1], all_host[:K + WIN + 1]
        # adaptive base resolution as create_frame computes it (:90-93) with the shipped config_odometry_gpu.json:54-59 values: the median range
        # of <= 256 samples between dmin 5 m and dmax 20 m maps to 0.25 m ... 0.5 m; voxelmap_scaling_factor 2 per level
        res0 = api.adaptive_voxel_resolution(api.median_distance(host[-1]), 0.25, 0.5, 5.0, 20.0)
        levels = [res0 * 2.0 ** lv for lv in range(LEVELS)]
        vmaps = [[api.GaussianVoxelMapGPU(r, ctx=ctx).insert(g) for r in levels] for g in frames[:-1]]
        cur, cur_pose = frames[-1], poses[-1]
        factors, deltas = [], []
        for t in range(len(frames) - 1 - WIN, len(frames) - 1):      # the sliding window: binary factors
            for lv in range(LEVELS):
                f = api.IntegratedVGICPFactorGPU(t, 99, vmaps[t][lv], cur)
                f.set_enable_surface_validation(True)
                factors.append(f)
                deltas.append(api.pose12(synth.relative_pose(poses[t], cur_pose)))
        for t in range(K):                                           # the keyframes: unary factors against their fixed poses
            for lv in range(LEVELS):
                f = api.IntegratedVGICPFactorGPU(poses[t], 99, vmaps[t][lv], cur)
                f.set_enable_surface_validation(True)
                factors.append(f)
                deltas.append(api.pose12(synth.relative_pose(poses[t], cur_pose)))
        deltas = np.stack(deltas)
        nf = len(factors)
        r = {"points_per_frame": cur.size(), "factors_per_frame": nf, "voxel_resolutions_m": [round(x, 3) for x in levels]}
        # --- the optimiser's linearisation, three ways
        r["fresh_set_linearize_us"] = api.profile_fresh_sets(factors, deltas, iters=300, ctx=ctx)
        ctx.set_diag("resident=0")  # what a factor list that has not been linearised three times yet gets: one dispatch per call
        r["fresh_set_linearize_us_launch_per_call"] = api.profile_fresh_sets(factors, deltas, iters=300, ctx=ctx)
        ctx.set_diag("plan_cache=0")
        r["fresh_set_linearize_us_without_plan_cache"] = api.profile_fresh_sets(factors, deltas, iters=60, ctx=ctx)
        ctx.set_diag("")
        pset = api.NonlinearFactorSetGPU(ctx)
        for f in factors:
            pset.add(f)
        r["persistent_set_linearize_us"] = pset.profile_sync(deltas, iters=300) * 1e3
        ctx.set_diag("host_poses=0")
        r["persistent_set_linearize_us_with_pose_upload"] = pset.profile_sync(deltas, iters=200) * 1e3
        ctx.set_diag("")
        k_ms, lin_ms = pset.profile(deltas, iters=50)
        r["device_us"] = {"fused_kernels": k_ms * 1e3, "kernels_plus_finalise": lin_ms * 1e3}
        r["host_enqueue_and_wake_up_us"] = r["persistent_set_linearize_us"] - lin_ms * 1e3
        r["plan_lookup_and_set_management_us"] = r["fresh_set_linearize_us"] - r["persistent_set_linearize_us"]
        # --- overlap_gpu: the per-frame 15-target call, a single-target call, the 43-call elimination loop as separate calls and as ONE batch
        kf_maps = [vmaps[t][-1] for t in range(K)]
        kf_delta = [synth.relative_pose(poses[t], cur_pose) for t in range(K)]
        r["overlap_15_targets_us"] = api.overlap_profile([(kf_maps, cur, kf_delta)], iters=300, ctx=ctx)
        r["overlap_1_target_us"] = api.overlap_profile([(kf_maps[:1], cur, kf_delta[:1])], iters=300, ctx=ctx)
        loop = [([kf_maps[i]], cur, [kf_delta[i]]) for i in range(K)]
        for i in range(K - 1):
            loop.append(([kf_maps[i]], cur, [kf_delta[i]]))
            others = [j for j in range(K - 1) if j != i]
            loop.append(([kf_maps[j] for j in others], frames[i], [synth.relative_pose(poses[j], poses[i]) for j in others]))
        r["keyframe_elimination_loop_calls"] = len(loop)
        r["keyframe_elimination_loop_separate_calls_us"] = float(sum(api.overlap_profile([q], iters=40, ctx=ctx) for q in loop))
        r["keyframe_elimination_loop_one_batch_us"] = api.overlap_profile(loop, iters=100, ctx=ctx)
        batch = api.overlap_gpu_batch(loop, ctx=ctx)
        single = [api.overlap_gpu(q[0], q[1], q[2]) for q in loop]
        r["batch_equals_separate_calls"] = bool(batch == single)
        # --- create_frame: clone of a frame that arrives with CPU covariances + the two map builds (PCIe upload included)
        xyz, c32, n32 = cur.download()
        nn = len(xyz)
        p4 = np.ones((nn, 4))
        p4[:, :3] = host[-1]
        m44 = np.zeros((nn, 4, 4))
        m44[:, :3, :3] = c32
        c16 = np.ascontiguousarray(np.transpose(m44, (0, 2, 1))).reshape(nn, 16)  # column-major Matrix4d, as the frame arrives from the CPU front end
        n4 = np.zeros((nn, 4))
        n4[:, :3] = n32
        reps = 30
        t_clone = t_maps = t_first = t_second = 0.0
        first_use = []
        import gc

        gc.collect()
        gc.disable()  # (a generation-2 collection of this process's numpy scenery inside one sample would read as tens of milliseconds of "first use")
        for rep in range(-2, reps):  # two untimed passes: the first launch of a kernel variant loads its code object (tens of ms, once per process)
            if rep == 0:
                t_clone = t_maps = t_first = t_second = 0.0
                first_use = []
            t0 = time.perf_counter()
            g = api.PointCloudGPU.clone_packed(p4, c16, n4, ctx=ctx)
            t1 = time.perf_counter()
            ms = [api.GaussianVoxelMapGPU(rr, ctx=ctx).insert(g) for rr in levels]
            t2 = time.perf_counter()
            # the first factor that uses the new cloud as its source builds the cloud's factor streams (Hilbert rank + stream kernel): a
            # per-frame cost that the steady-state linearisation figures above do not contain.  Timed as first use minus second use.
            one = api.NonlinearFactorSetGPU(ctx)
            one.add(api.IntegratedVGICPFactorGPU(np.eye(4), 1, vmaps[0][0], g))
            one.linearize({1: np.eye(4)})
            t3 = time.perf_counter()
            one.linearize({1: np.eye(4)})
            t4 = time.perf_counter()
            t_clone += t1 - t0
            t_maps += t2 - t1
            t_first += t3 - t2
            t_second += t4 - t3
            first_use.append((t3 - t2) - (t4 - t3))
            one.close()
            for m in ms:
                m.close()
            g.close()
        gc.enable()
        r["create_frame_us"] = {"clone_upload_pack": t_clone / reps * 1e6, "two_voxelmap_inserts": t_maps / reps * 1e6,
                                "factor_streams_on_first_use": max(0.0, float(np.median(first_use)) * 1e6),
                                "factor_streams_on_first_use_mean_max": [max(0.0, (t_first - t_second) / reps * 1e6), float(np.max(first_use)) * 1e6],
                                "upload_bytes": int(p4.nbytes + c16.nbytes + n4.nbytes), "note": "pageable host arrays, as GLIM hands them over"}
        # A frame brings a NEW cloud, hence a new factor list: its first linearisation builds the plan (the figure without the plan cache), the
        # following ones of the same frame adopt it and -- fewer than four calls -- go out as launches, not through the resident session
        # (`fresh_set_linearize_us`, the repeated-list figure, is what a list that stays gets from its fourth linearisation on).
        frame_us = (r["create_frame_us"]["clone_upload_pack"] + r["create_frame_us"]["two_voxelmap_inserts"] + r["create_frame_us"]["factor_streams_on_first_use"]
                    + r["fresh_set_linearize_us_without_plan_cache"] + (ITERS - 1) * r["fresh_set_linearize_us_launch_per_call"] + r["overlap_15_targets_us"])
        r["frame_us"] = {"optimiser_iterations": ITERS, "ordinary_frame": frame_us,
                         "model": "clone + two maps + first use of the new cloud + first linearisation (plan build) + (iterations - 1) x launch-per-call linearisation + 15-target overlap", "new_keyframe_frame": frame_us + r["keyframe_elimination_loop_separate_calls_us"],
                         "new_keyframe_frame_batched_loop": frame_us + r["keyframe_elimination_loop_one_batch_us"]}
        if keep:
            # ---- the frame as ONE timed unit: tools/odometry_frame_loop.cpp drives the real sequence (new cloud, clone, two maps, 34 fresh factors,
            # ITERS linearisations on fresh sets, 15-target overlap, the oldest window frame retired) through the C ABI from C++, 300 frames
            r["live_loop"] = live_odometry_loop(api, all_host, all_poses, c32_of=lambda g: g.download(), frames=all_frames, K=K, WIN=WIN, res0=res0, iters=ITERS,
                                                timed=args.frames)
        out[label] = r
        pset.close()
        for row in vmaps:
            for m in row:
                m.close()
        for g in all_frames:
            g.close()
    main_r = out["frames_10000_pts"]
    live = (main_r.get("live_loop") or {}).get("one_submission_create_frame") or (main_r.get("live_loop") or {}).get("separate_calls")
    headline = live["frame_us"]["p50"] if live and "frame_us" in live else main_r["frame_us"]["ordinary_frame"]
    return {
        "metric": "odometry_frame_us", "value": headline, "unit": "us", "n_gpus": 1, "steps": args.frames, "warmup": 20,
        "value_is": "p50 of the live loop (tools/odometry_frame_loop.cpp: one timed unit per frame)" if live and "frame_us" in live else "frame_us.model (sum of separately timed pieces)",
        "ms_per_step": headline * 1e-3, "higher_is_better": False, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "GLIM OdometryEstimationGPU call pattern per frame: clone + 2 voxel maps + optimiser iterations x (fresh 34-factor set: add, linearize) + "
                               "15-target overlap; keyframe elimination loop (43 overlap calls) on new keyframes", **out},
    }


def live_odometry_loop(api, host, poses, c32_of, frames, K, WIN, res0, iters, timed):
    """Writes the scene (every frame with the covariances / normals the device estimated, in the reference's Vector4d / Matrix4d layout), builds
    tools/odometry_frame_loop.cpp against the library this process uses and runs it twice: create_frame as three calls and as one submission."""
    import contextlib
    import subprocess
    import tempfile

    from glim_amd import _lib

    n = len(host[0])
    out = {}
    keep_dir = os.environ.get("BENCH_KEEP_FRAME_LOOP")  # diagnostic: leave scene.bin and the built tool in this directory (tools/frame_tail_trace.sh runs it under rocprofv3)
    if keep_dir:
        os.makedirs(keep_dir, exist_ok=True)
    with (contextlib.nullcontext(keep_dir) if keep_dir else tempfile.TemporaryDirectory()) as tmp:
        scene = os.path.join(tmp, "scene.bin")
        with open(scene, "wb") as f:
            np.array([len(host), n, K, WIN], dtype=np.int32).tofile(f)
            np.array([res0], dtype=np.float64).tofile(f)
            for pts, g, T in zip(host, frames, poses):
                _, c32, n32 = c32_of(g)
                p4 = np.ones((n, 4))
                p4[:, :3] = pts[:, :3]
                m44 = np.zeros((n, 4, 4))
                m44[:, :3, :3] = c32
                n4 = np.zeros((n, 4))
                n4[:, :3] = n32
                p4.tofile(f)
                np.ascontiguousarray(np.transpose(m44, (0, 2, 1))).tofile(f)
                n4.tofile(f)
                np.ascontiguousarray(np.asarray(T, dtype=np.float64)[:3, :4]).tofile(f)
        exe = os.path.join(tmp, "odometry_frame_loop")
        libdir = os.path.dirname(_lib.LIB_PATH)
        try:
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "odometry_frame_loop.cpp"),
                                   "-L" + libdir, "-l:" + os.path.basename(_lib.LIB_PATH), "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
            for name, fused, diag in (("separate_calls", 0, ""), ("one_submission_create_frame", 1, ""),
                                      ("one_submission_as_round5_take2", 1, "frame_fused=0,pull_gated=0,plan_recycle=0"),
                                      ("one_submission_without_fused_frame_kernels", 1, "frame_fused=0"),
                                      ("one_submission_without_fused_frame_kernels_and_gated_pull", 1, "frame_fused=0,pull_gated=0"),
                                      ("one_submission_without_gated_pull", 1, "pull_gated=0"), ("one_submission_without_plan_recycling", 1, "plan_recycle=0")):
                res = subprocess.run([exe, scene, str(timed), str(iters), str(fused), diag], capture_output=True, text=True, timeout=300)
                out[name] = json.loads(res.stdout.strip().splitlines()[-1]) if res.returncode == 0 and res.stdout.strip() else {"error": (res.stderr or res.stdout)[-400:]}
        except Exception as e:  # noqa: BLE001 -- reported, the pieces above stand on their own
            out["error"] = repr(e)
    out["what"] = ("GLIM's live GPU odometry frame as ONE timed unit, driven from C++ through the C ABI on a context of the odometry module's kind: a NEW "
                   f"{n}-pt frame with CPU covariances -> clone + two voxel maps -> (window {WIN} + keyframes {K}) x 2 levels = {2 * (K + WIN)} fresh factors "
                   f"(surface validation ON) -> {iters} linearisations on FRESH factor sets -> 15-target overlap -> the oldest window frame retired")
    return out


def submap20_traffic(nf):
    t = measured_traffic("submap20")
    return (t[0] * nf, t[1], t[2]) if t else None  # (measured per factor over the 380-factor launch)


def run_submap20(args, D, api, ctx):
    """configs[2]: SubMappingGPU local bundle (sub_mapping.cpp:276-315): all pairs of 20 keyframes x 2 voxel levels."""
    from glim_amd import synth

    K = 20
    poses = synth.arc_trajectory(K, step=0.5, yaw_step_deg=1.5)
    clouds = make_frames(api, ctx, poses, 64, 1024)
    levels = (0.25, 0.5)  # config_sub_mapping_gpu.json:48-50
    vmaps = [[api.GaussianVoxelMapGPU(r, ctx=ctx).insert(c) for r in levels] for c in clouds]
    fset = api.NonlinearFactorSetGPU(ctx)
    deltas, n_pts, n_vox = [], [], []
    for i in range(K):
        for j in range(i + 1, K):
            for lv in range(len(levels)):
                fset.add(api.IntegratedVGICPFactorGPU(i, j, vmaps[i][lv], clouds[j]))
                deltas.append(api.pose12(synth.relative_pose(poses[i], poses[j])))
                n_pts.append(clouds[j].size())
                n_vox.append(vmaps[i][lv].voxelmap_info()["num_voxels"])
    deltas = np.stack(deltas)
    nf = len(deltas)
    out = D.torch.zeros(nf, api._lib.COMPACT_DOUBLES, dtype=D.torch.float64, device="cuda")
    elapsed = timed_steps(D, lambda i: fset.linearize_device_async(deltas, out.data_ptr(), 0), args.steps, args.warmup)
    errs = fset_error(fset, deltas)
    # one LM iteration = linearise (records on the host) + error at the trial values for the accept / reject test (sub_mapping.cpp:435-443),
    # both synchronous, timed inside the library (the Python binding's per-record dict construction is not part of the path)
    ms_lin_sync, ms_err_sync = fset.profile_lm(deltas, iters=20)
    lm_ms = ms_lin_sync + ms_err_sync
    inl = float(np.mean([r["num_inliers"] for r in fset.linearize_poses(deltas)]) / np.mean(n_pts))
    return {
        "metric": "vgicp_linearize_calls_per_s", "value": nf * args.steps / elapsed, "unit": "calls/s", "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": "configs[2] submap20: 20 keyframes x 65536 pts, 190 pairs x 2 levels (0.25/0.5 m) = 380 binary factors",
                   "factors": nf, "bundle_linearize_ms": elapsed / args.steps * 1e3, "lm_iteration_ms": lm_ms, "sync_linearize_ms": ms_lin_sync, "sync_error_ms": ms_err_sync,
                   "mean_inlier_fraction": inl, "sum_error": float(np.sum(errs))},
        "roofline": roofline_of(fset, deltas, n_pts, n_vox, max(5, args.steps), submap20_traffic(nf)),
    }


def run_odometry_under_load(args, D, api, ctx):
    """GLIM's THREE-THREAD model on one device (async_odometry_estimation.cpp:15, async_sub_mapping.cpp:8, async_global_mapping.cpp:24; each module
    owns its stream pool: odometry_estimation_gpu.cpp:76-77, sub_mapping.cpp:86-87, global_mapping.cpp:110): the latency of the odometry's
    linearisation -- a fresh 34-factor set of 10 000-pt frames per optimiser iteration, 50 us of host work between iterations -- alone and while a
    second thread keeps the device busy with a mapping module's work on ITS OWN context: back-to-back linearisations of the 380-factor sub-mapping
    bundle (20 x 65 536 pts, 0.21 ms kernels that fill the chip) and a merge_frames of 15 frames per loop.  p50 / p99 of the odometry call for:
      own_context_high_priority   the shipped drop-in wiring: one context per module, the odometry's streams at the device's greatest priority
      own_context                 the same without the priority
      shared_context              round 3's wiring: every module on ONE context (one mutex, one stream pool)
    each with the resident session on (default) and off (`launch_per_call`)."""
    import threading

    from glim_amd import synth

    scene = synth.Scene.default()
    K, WIN, LEVELS = 15, 2, 2
    rng = np.random.default_rng(3)
    dirs = synth.lidar_directions(128, 1024)
    poses = synth.arc_trajectory(K + WIN + 1, step=0.4, yaw_step_deg=1.5)
    scans = []
    for i, T in enumerate(poses):
        pts = synth.scan(scene, T, dirs, 500 + i)
        scans.append(pts[np.sort(rng.choice(len(pts), 10000, replace=False))])
    bg_poses = synth.arc_trajectory(20, step=0.5, yaw_step_deg=1.5)
    bg_dirs = synth.lidar_directions(64, 1024)
    bg_scans = [synth.scan(scene, T, bg_dirs, 900 + i) for i, T in enumerate(bg_poses)]

    def odometry_problem(c):
        frames = []
        for pts in scans:
            g = api.PointCloudGPU.clone(pts, ctx=c)
            g.find_neighbors(10, download=False)
            g.estimate_covariances(10)
            frames.append(g)
        res0 = api.adaptive_voxel_resolution(api.median_distance(scans[-1]), 0.25, 0.5, 5.0, 20.0)
        levels = [res0 * 2.0 ** lv for lv in range(LEVELS)]
        vmaps = [[api.GaussianVoxelMapGPU(r, ctx=c).insert(g) for r in levels] for g in frames[:-1]]
        cur, cur_pose = frames[-1], poses[-1]
        factors, deltas = [], []
        for t in list(range(len(frames) - 1 - WIN, len(frames) - 1)) + list(range(K)):
            binary = t >= len(frames) - 1 - WIN
            for lv in range(LEVELS):
                f = api.IntegratedVGICPFactorGPU(t if binary else poses[t], 99, vmaps[t][lv], cur)
                f.set_enable_surface_validation(True)
                factors.append(f)
                deltas.append(api.pose12(synth.relative_pose(poses[t], cur_pose)))
        return frames, vmaps, factors, np.stack(deltas)

    def background_problem(c):
        clouds = []
        for s in bg_scans:
            g = api.PointCloudGPU.clone(s, ctx=c)
            g.find_neighbors(10, download=False)
            g.estimate_covariances(10)
            clouds.append(g)
        vm = [[api.GaussianVoxelMapGPU(r, ctx=c).insert(g) for r in (0.25, 0.5)] for g in clouds]
        fs = api.NonlinearFactorSetGPU(c)
        d = []
        for i in range(20):
            for j in range(i + 1, 20):
                for lv in range(2):
                    fs.add(api.IntegratedVGICPFactorGPU(i, j, vm[i][lv], clouds[j]))
                    d.append(api.pose12(synth.relative_pose(bg_poses[i], bg_poses[j])))
        d = np.stack(d)
        out = D.torch.zeros(len(d), api._lib.COMPACT_DOUBLES, dtype=D.torch.float64, device="cuda")
        merge_in = []
        for s in bg_scans[:15]:
            sub = s[:: max(1, len(s) // 12288)][:12288].astype(np.float64)
            merge_in.append((sub, np.tile(np.eye(3) * 1e-2, (len(sub), 1, 1))))
        packed = api._pack_frames([np.eye(4)] * 15, [m[0] for m in merge_in], [m[1] for m in merge_in])
        return clouds, vm, fs, d, out, packed

    def percentiles(x):
        return {"p50_us": float(np.percentile(x, 50)), "p99_us": float(np.percentile(x, 99)), "max_us": float(x.max()), "mean_us": float(x.mean())}

    wirings = {}
    for name, prio, shared in (("own_context_high_priority", 1, False), ("own_context", 0, False), ("shared_context", 0, True)):
        c_odo = api.Context(D.local_rank, 8, priority=prio)
        c_bg = c_odo if shared else api.Context(D.local_rank, 8)
        odo = odometry_problem(c_odo)
        bg = background_problem(c_bg)
        factors, deltas = odo[2], odo[3]
        _, _, bfs, bd, bout, packed = bg
        entry = {}

        def background_once():
            for _ in range(4):
                bfs.linearize_device_async(bd, bout.data_ptr(), 0)
            c_bg.synchronize()
            api.merge_frames(None, None, None, downsample_resolution=0.25, ctx=c_bg, packed=packed).close()

        # the MAPPING thread's side (only the odometry's side was reported): its loops per second with the device to itself
        api.resident_stop(c_odo)
        for _ in range(3):
            background_once()
        n_alone, t_alone = 0, time.perf_counter()
        while time.perf_counter() - t_alone < 0.4:
            background_once()
            n_alone += 1
        bg_alone = n_alone / (time.perf_counter() - t_alone)
        for mode, diag in (("resident_session", ""), ("launch_per_call", "resident=0")):
            c_odo.set_diag(diag)
            idle = api.profile_fresh_sets_samples(factors, deltas, iters=2000, gap_us=50.0, ctx=c_odo)
            stop = threading.Event()
            loops = [0]

            def background():
                while not stop.is_set():
                    for _ in range(4):
                        bfs.linearize_device_async(bd, bout.data_ptr(), 0)
                    c_bg.synchronize()
                    api.merge_frames(None, None, None, downsample_resolution=0.25, ctx=c_bg, packed=packed).close()
                    loops[0] += 1

            th = threading.Thread(target=background)
            th.start()
            time.sleep(0.05)
            t0 = time.perf_counter()
            loaded = api.profile_fresh_sets_samples(factors, deltas, iters=2000, gap_us=50.0, ctx=c_odo)
            wall = time.perf_counter() - t0
            stop.set()
            th.join()
            entry[mode] = {"idle": percentiles(idle), "under_load": percentiles(loaded), "p99_ratio": float(np.percentile(loaded, 99) / np.percentile(idle, 99)),
                           "p50_ratio": float(np.percentile(loaded, 50) / np.percentile(idle, 50)),
                           "background_loops_per_s": loops[0] / max(wall, 1e-9),
                           "mapping_thread": {"loops_per_s_alone": bg_alone, "loops_per_s_beside_the_odometry": loops[0] / max(wall, 1e-9),
                                              "slowdown": bg_alone / max(1e-9, loops[0] / max(wall, 1e-9)),
                                              "what": "thread B's loop (4 x the 380-factor bundle + one 15-frame merge) per second with the device to itself and beside "
                                                      "thread A's stream of 34-factor linearisations (50 us apart) in this mode"}}
            api.resident_stop(c_odo)
        c_odo.set_diag("")
        wirings[name] = entry
        del odo, bg, bfs, bout
    head = wirings["own_context_high_priority"]["resident_session"]
    return {
        "metric": "odometry_linearize_p99_us_under_load", "value": head["under_load"]["p99_us"], "unit": "us", "n_gpus": 1, "steps": 2000, "warmup": 5,
        "ms_per_step": head["under_load"]["mean_us"] * 1e-3, "higher_is_better": False, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "odometry_under_load: thread A = fresh 34-factor sets on 10 000-pt frames (surface validation on), 50 us between calls; thread B = "
                               "380-factor sub-mapping bundle (20 x 65 536 pts) linearised back to back + merge_frames(15 x 12 288 pts), on its own context",
                   "wirings": wirings,
                   "reference_model": "three module threads, one stream pool each: async_odometry_estimation.cpp:15 + odometry_estimation_gpu.cpp:76-77, "
                                      "async_sub_mapping.cpp:8 + sub_mapping.cpp:86-87, async_global_mapping.cpp:24 + global_mapping.cpp:110"},
    }


def fset_error(fset, deltas):
    import ctypes as C

    n = len(deltas)
    err = np.zeros(n)
    T = np.ascontiguousarray(deltas)
    from glim_amd.api import check, lib

    check(lib().glim_amd_factor_set_error(fset._h, None, T.ctypes.data_as(C.POINTER(C.c_double)), err.ctypes.data_as(C.POINTER(C.c_double)), None),
          "glim_amd_factor_set_error")
    return err


def make_merged_submaps(api, ctx, n_submaps, frames_per_submap, rings, azimuths, spacing=2.0):
    """Submaps as GLIM's SubMapping builds them (sub_mapping.cpp:480-497): the keyframes of a submap (kNN + covariances estimated on the
    device, PLANE form) are moved into the submap origin and voxel-grid merged by merge_frames at submap_downsample_resolution = 0.1 m
    (config_sub_mapping_gpu.json:52).  The result carries AVERAGED, ROTATED covariances and no normals: it takes the general factor
    kernel, not the plane-form one."""
    from glim_amd import synth
    from glim_amd.se3 import se3_exp

    scene = synth.Scene.default()
    dirs = synth.lidar_directions(rings, azimuths)
    side = int(round(n_submaps ** 0.5 + 0.499))
    origins = synth.grid_trajectory(side, side, spacing=spacing)[:n_submaps]
    rng = np.random.default_rng(77)
    out = []
    for s_idx, T_origin in enumerate(origins):
        pts, covs, rel = [], [], []
        for k in range(frames_per_submap):
            T_frame = T_origin @ se3_exp(np.r_[rng.normal(size=3) * 0.02, (0.35 * k, 0.05 * rng.normal(), 0.0)])
            scan = synth.scan(scene, T_frame, dirs, frame_id=10 * s_idx + k)
            g = api.PointCloudGPU.clone(scan, ctx=ctx)
            g.find_neighbors(10, download=False)
            g.estimate_covariances(10)
            c = g.download(normals=False)[1]
            g.close()
            pts.append(scan.astype(np.float64))
            covs.append(c.astype(np.float64))
            rel.append(np.linalg.inv(T_origin) @ T_frame)
        out.append((T_origin, api.merge_frames(rel, pts, covs, downsample_resolution=0.1, ctx=ctx)))
    return out


def sampled_pair_parity(api, fset, owned, pairs, deltas, clouds, records, n_sample=64, n_corr=8):
    """configs[3] at its own size, against the checker: >= 64 of this rank's pairs -- the 16 with the fewest inliers (far / barely overlapping),
    the 16 with the most (near), 32 spread over the quantiles in between -- are linearised by the FP64 oracle on the downloaded merged clouds
    (the FP32 image the factor consumes): inlier counts equal, damped Gauss-Newton step within 1e-4, correspondences bit-exact on `n_corr` of
    them.  `records`: this evaluation's compact rows in factor order.  Outside every timed region."""
    from oracle import oracle as orc

    owned = np.asarray(list(owned))
    inl = records[owned, 0]
    order = np.argsort(inl, kind="stable")
    pick = list(dict.fromkeys(list(order[:16]) + list(order[-16:]) + list(order[np.linspace(0, len(order) - 1, 48).astype(int)])))[:n_sample]
    corr_pick = set(pick[:: max(1, len(pick) // n_corr)][:n_corr])
    host, maps = {}, {}

    def cloud(i):
        if i not in host:
            xyz, c32, _ = clouds[i].download(normals=False)
            host[i] = (xyz, c32.astype(np.float64))
        return host[i]

    worst, inliers_equal, corr_ok, n_corr_done, n_step, zero_inlier = 0.0, True, True, 0, 0, 0
    for k in pick:
        f = int(owned[k])
        i, j = pairs[f]
        if i not in maps:
            maps[i] = orc.VoxelMap(1.0).insert(*cloud(i))
        xyz, cov = cloud(j)
        delta = np.eye(4)
        delta[:3, :4] = deltas[f].reshape(3, 4)
        ref = orc.vgicp_linearize(maps[i], xyz, cov, delta, want_corr=(k in corr_pick))
        got = api.expand_compact(records[f], deltas[f], api.FACTOR_BINARY)
        inliers_equal = inliers_equal and int(got["num_inliers"]) == int(ref["num_inliers"])
        zero_inlier += int(ref["num_inliers"] == 0)
        if ref["num_inliers"] >= 100:
            lam = 1e-6 * np.trace(ref["H_ss"]) / 6
            d_got = np.linalg.solve(got["H_ss"] + lam * np.eye(6), -got["b_s"])
            d_ref = np.linalg.solve(ref["H_ss"] + lam * np.eye(6), -ref["b_s"])
            worst = max(worst, float(np.abs(d_got - d_ref).max()))
            n_step += 1
        if k in corr_pick:
            c = fset.correspondences(int(k), delta)
            hit = c[:, 3] > 0
            corr_ok = corr_ok and np.array_equal(hit, ref["corr"][:, 3] >= 0) and np.array_equal(c[:, :3], ref["corr"][:, :3])
            n_corr_done += 1
    # a pair's inlier fraction is taken over ITS OWN source cloud (merged submaps differ in size)
    frac_of_pick = np.array([inl[k] / max(1, clouds[pairs[int(owned[k])][1]].size()) for k in pick])
    assert frac_of_pick.max() <= 1.0
    return {"pairs_checked": len(pick), "inlier_counts_equal": bool(inliers_equal), "gn_steps_compared": n_step, "max_pose_delta_err": worst, "tolerance": 1e-4,
            "correspondence_lists_compared": n_corr_done, "correspondences_bit_exact": bool(corr_ok), "zero_inlier_pairs_in_sample": zero_inlier,
            "inlier_fraction_range_of_sample": [float(frac_of_pick.min()), float(frac_of_pick.max())],
            "checker": "oracle/vgicp_oracle.c (FP64) on the downloaded FP32 merged clouds, 1.0 m CPU voxel maps"}


def predict_scaling(api, ctx, multi, pairs, deltas, clouds, vmaps, costs_points, records, t1_ms, torch):
    """What one GPU can say about 2 / 4 / 8: every contiguous shard of the pair list is evaluated ALONE on this GPU (kernels + finalise,
    device-resident results) and timed; max over the shards of a world size = that world's compute time, t1 / max = its compute-only
    strong-scaling bound (no collective, no launch skew).  Swept over the ORDER of the pair list that is cut into contiguous shards
    (target-major, as GlobalMapping creates the factors, or source-major, which keeps all uses of a source stream on one rank) and over two
    cost models for the shard boundaries: source points (the shipped rule) and a least-squares fit t ~ a * points + b * inliers over the
    measured shards (with skip-all-miss trips a factor's cost follows its hits)."""
    n = len(pairs)
    inliers = records[:, 0]
    points = np.asarray(costs_points, dtype=np.float64)

    def time_shard(idx):
        if len(idx) == 0:
            return 0.0
        fs = api.NonlinearFactorSetGPU(ctx)
        for f in idx:
            i, j = pairs[f]
            fs.add(api.IntegratedVGICPFactorGPU(i, j, vmaps[i], clouds[j]))
        out = torch.zeros(len(idx), api._lib.COMPACT_DOUBLES, dtype=torch.float64, device="cuda")
        P = np.ascontiguousarray(deltas[idx])
        # (round 4 timed 5 evaluations after 2 warm-ups, right behind ~10 ms of host work building the set: the shards summed to 12.4-13.0 ms against
        # 10.5 ms for the whole list.  A rank of a real N-GPU run evaluates its shard back to back, so the shard is warmed like the whole list is.)
        for _ in range(6):
            fs.linearize_device_async(P, out.data_ptr(), 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reps = 20
        for _ in range(reps):
            fs.linearize_device_async(P, out.data_ptr(), 0)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / reps * 1e3
        fs.close()
        return ms

    def sweep(order, costs):
        res, samples = {}, []
        for world in (2, 4, 8):
            b = multi.shard_bounds(costs[order], world)
            shards = [order[b[r]:b[r + 1]] for r in range(world)]
            ms = [time_shard(sh) for sh in shards]
            for sh, m in zip(shards, ms):
                samples.append((float(points[sh].sum()), float(inliers[sh].sum()), m))
            res[str(world)] = {"shard_ms": [round(m, 3) for m in ms], "shards_sum_ms": float(np.sum(ms)), "max_over_mean": float(max(ms) / np.mean(ms)),
                               "compute_only_speedup_bound": float(t1_ms / max(ms)), "pairs_per_shard": [int(len(sh)) for sh in shards]}
        return res, samples

    pi, pj = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    orders = {"target_major": np.lexsort((pj, pi)), "source_major": np.lexsort((pi, pj))}
    out = {"one_gpu_ms": t1_ms, "what": "each contiguous shard of the (re-ordered) pair list evaluated alone on this one GPU; speedup bound = one-GPU time / slowest shard (compute only)"}
    for name, order in orders.items():
        by_points, samples = sweep(order, points)
        A = np.array([[p, i] for p, i, _ in samples])
        coef, *_ = np.linalg.lstsq(A, np.array([m for _, _, m in samples]), rcond=None)
        entry = {"cost_model_points": by_points, "cost_model_fit": {"ms_per_million_points": float(coef[0] * 1e6), "ms_per_million_inliers": float(coef[1] * 1e6)}}
        if coef[0] > 0 and coef[1] > 0:
            entry["cost_model_fit"]["worlds"] = sweep(order, np.maximum(1e-12, coef[0] * points + coef[1] * inliers))[0]
        out["pair_order_" + name] = entry
    return out


def run_global256(args, D, api, ctx, extra_only=False):
    """configs[3] / metric M2: all-pairs matching cost over 256 MERGED submaps (general-covariance clouds, 1.0 m voxel maps), pair list
    sharded over the ranks, RCCL all-gather of the per-pair blocks (global_mapping.cpp:430-484 evaluates these factors one device, one
    stream pool; the sharding is the new part).  value = seconds per evaluation of the whole cost (error + H/b of every pair)."""
    from glim_amd import multi, synth

    torch = D.torch
    S = args.submaps
    t0 = time.time()
    submaps = make_merged_submaps(api, ctx, S, args.submap_frames, args.submap_rings, args.submap_azimuths)  # replicated on every rank
    clouds = [g for _, g in submaps]
    poses = [T for T, _ in submaps]
    vmaps = [api.GaussianVoxelMapGPU(1.0, ctx=ctx).insert(c) for c in clouds]  # global_mapping.cpp:59 default resolution
    sizes = [c.size() for c in clouds]
    log(f"replicated {S} merged submaps ({args.submap_frames} keyframes each, {int(np.mean(sizes))} pts on average) per rank in {time.time() - t0:.1f}s")
    # all pairs (target i < source j), listed SOURCE-major: a rank's contiguous shard then holds every use of its source streams (the plan
    # groups the factors of a source, so all but the first of them find the stream in L2 / the Infinity Cache), which the one-GPU shard
    # simulation below prices at 6.75-6.85x of 8 against 6.3-6.5x for the target-major order GlobalMapping creates its factors in
    pairs = [(i, j) for j in range(S) for i in range(j)]
    costs = [sizes[j] for _, j in pairs]
    ev = multi.ShardedCostEvaluator(costs, D.rank, D.world)
    fset = api.NonlinearFactorSetGPU(ctx)
    deltas = np.stack([api.pose12(synth.relative_pose(poses[i], poses[j])) for i, j in pairs])
    for f in ev.owned():
        i, j = pairs[f]
        fset.add(api.IntegratedVGICPFactorGPU(i, j, vmaps[i], clouds[j]))
    # every rank sends only the rows it owns (shards padded to the longest): one all-gather over xGMI, half the bytes of the zero-padded
    # all-reduce of a dense [pairs x 29] array, nothing to zero; the factor-ordered array is one index_select on the device
    max_rows, index = ev.gather_layout()
    send = torch.zeros(max_rows, api._lib.COMPACT_DOUBLES, dtype=torch.float64, device="cuda")
    gathered = torch.zeros(D.world * max_rows, api._lib.COMPACT_DOUBLES, dtype=torch.float64, device="cuda")
    index_t = torch.as_tensor(index, device="cuda")
    local_poses = deltas[ev.lo:ev.hi]
    result = {}

    def step(_):
        ev.gather_device(fset, deltas, send, gathered)
        result["blocks"] = gathered.index_select(0, index_t)

    steps = max(args.steps, 20) if extra_only else args.steps
    exchange = {"form": "one all-gather of the whole shard"}
    if D.collective and not args.no_split:
        # Second form of the same exchange: the shard as two factor sets, so that the all-gather of the first half (RCCL's stream) overlaps the
        # kernels of the second (our stream).  Which of the two is faster depends on the node (xGMI latency against ~1/8 of the kernels), so
        # both run 5 evaluations here, outside the timed region, and the K timed steps use the faster one; both calibration times are reported.
        _, h_rows, index_h = ev.halves_layout()
        index_h_t = torch.as_tensor(index_h, device="cuda")
        halves = []
        for lo_h, hi_h in ev.halves_ranges():
            fs = api.NonlinearFactorSetGPU(ctx)
            for f in range(lo_h, hi_h):
                fs.add(api.IntegratedVGICPFactorGPU(pairs[f][0], pairs[f][1], vmaps[pairs[f][0]], clouds[pairs[f][1]]))
            halves.append(fs)

        def step_split(_):
            ev.gather_device_halves(halves[0], halves[1], deltas, send, gathered)
            result["blocks"] = gathered.index_select(0, index_h_t)

        t_plain = timed_steps(D, step, 5, 2) / 5
        t_split = timed_steps(D, step_split, 5, 2) / 5
        exchange = {"calibration_ms": {"whole_shard": t_plain * 1e3, "two_halves_overlapped": t_split * 1e3}}
        if t_split < t_plain:  # max over ranks on both sides: every rank takes the same decision
            step = step_split
            exchange["form"] = "two halves: all-gather of the first overlaps the kernels of the second"
        else:
            exchange["form"] = "one all-gather of the whole shard"
    elapsed = timed_steps(D, step, steps, max(args.warmup, 3))
    host = result["blocks"].cpu().numpy()
    # The timed loop above never waits for an evaluation: the K evaluations queue up behind one another on the stream and nothing returns to the
    # host (what `value` has meant since round 1).  An optimiser needs the records ON THE HOST before it can choose the next linearisation point, which
    # is what the native C-ABI path (glim_amd_multi_linearize: synchronous, records in pinned host memory) delivers -- so the like-for-like partner of
    # `native_c_abi_world1` is THIS loop with a copy-out and a synchronise per evaluation:
    pinned = torch.empty(result["blocks"].shape, dtype=torch.float64, pin_memory=True)

    def step_sync(_):
        step(_)
        pinned.copy_(result["blocks"], non_blocking=True)
        torch.cuda.synchronize()

    elapsed_sync = timed_steps(D, step_sync, steps, 2)
    # where the time of one evaluation goes on THIS rank (HIP events on our stream, outside the timed region): kernels + finalise, the
    # all-gather, the index_select into factor order -- and the same exchange with the shard split in two so that the gather of the first
    # half overlaps the kernels of the second (what the N > 1 timed loop would gain from it)
    breakdown = ev.profile_device(fset, deltas, send, gathered, index_t, reps=5)
    n_pts = [costs[f] for f in ev.owned()]
    n_vox = [vmaps[pairs[f][0]].voxelmap_info()["num_voxels"] for f in ev.owned()]
    traffic = measured_traffic("global256") if (S, args.submap_frames, args.submap_rings, args.submap_azimuths) == (256, 4, 40, 560) else None
    if traffic:
        traffic = (traffic[0] * len(n_pts), traffic[1], traffic[2])  # measured per factor (PMC passes over all 32 640 pairs), scaled to this rank's share
    roof = roofline_of(fset, local_poses, n_pts, n_vox, 5, traffic)
    roof["kernel"] = "vgicp_kernel<LINEARIZE, general 36 B/pt>"
    roof["note"] = ("the pairs of one rank share 256 clouds / maps (0.6 GB): most re-reads are served by the 256 MiB Infinity Cache and L2, so the HBM "
                    "fraction is low BY DESIGN (SURVEY 8d's 48 B/pt per factor are cache hits here); this kernel is bound by vector-ALU issue, priced "
                    "below against the FP32 vector peak")
    # Hardware-peak fraction for the instruction-bound kernel: FP32 operations per point of its loop (static count of the shipped ISA,
    # tools/isa_stats.py -> profiles/*/isa_stats.json: fma = 2) x point visits / kernel time / 157.3 TFLOP/s (MI355X_MICROARCH.md FP32 vector peak).
    visits = float(sum(n_pts))
    isa = isa_stats_of("general")
    if isa:
        tflops = visits * isa["fp32_flops_per_point"] / (roof["kernel_ms"] * 1e-3) / 1e12
        roof["fp32"] = {"flops_per_point": isa["fp32_flops_per_point"], "fp64_flops_per_point": isa["fp64_flops_per_point"], "point_visits": visits,
                        "achieved_tflops": tflops, "peak_tflops": FP32_VECTOR_PEAK_TFLOPS, "frac_of_fp32_vector_peak": tflops / FP32_VECTOR_PEAK_TFLOPS,
                        "source": isa["source"], "valu_instructions_per_point": isa["valu_instructions_per_point"],
                        "note": "every lane computes every point of its trips (misses contribute exact zeros), so the count is per point VISITED; the other "
                                "vector-ALU slots of a trip are FP64 (point transform, bit-exact voxel coordinate), integer (hash, key compare) and selects"}
    # DIAGNOSTIC (not a roofline): issue ticks of the general kernel's per-point instruction mix at the measured issue costs of
    # tools/ubench/valu_rate.hip (1.15 / 2.43 / 2.0 / 3.0 ticks per FP32 / FP64 / integer / compare-select wave instruction; one tick = 2 cycles),
    # 1024 SIMDs at 2.4 GHz, with the share of all-miss trips COUNTED by the kernel in this very run.  It describes the kernel (within 3 %) but
    # mispredicted three A/Bs of round 3 (FP32 transform: model -10 %, measured -2 %; packed FP32: +4 %; ping-pong unroll: 0 %) -- VERDICT r4.
    ticks = 172 * 1.15 + 36 * 2.43 + 52 * 2.0 + 16 * 3.0
    pts_per_s = 64.0 * 1024.0 / (ticks * 2.0 / 2.4e9)
    fset.trip_stats(reset=True)
    ev.gather_device(fset, deltas, send, gathered)
    torch.cuda.synchronize()
    skipped, total_trips = fset.trip_stats(reset=True)
    skip_share = skipped / max(1, total_trips)
    # pre-cull (round 6): trips the pre-pass marked -- their chunk box misses the target's occupancy mask -- are never walked at all; the in-loop skip
    # above then only sees the all-miss trips the box test could not prove empty
    fset.cull_stats(reset=True)  # (arms the pre-pass's counters: it counts only on request)
    ev.gather_device(fset, deltas, send, gathered)
    torch.cuda.synchronize()
    culled = fset.cull_stats(reset=False)  # (reads and disarms)
    cull_share = (culled[0] / max(1, total_trips)) if culled else 0.0
    roof["pre_cull"] = ({"culled_trips_per_evaluation": int(culled[0]), "trips_with_points_per_evaluation": int(culled[1]), "trips_per_evaluation": int(total_trips),
                         "culled_share_of_trips_with_points": culled[0] / max(1, culled[1]), "in_loop_all_miss_skips_left": int(skipped),
                         "in_loop_skip_share_of_trips_with_points": skipped / max(1, culled[1])}
                        if culled else {"enabled": False})
    floor_ms = visits * (1.0 - skip_share * 0.6 - cull_share) / pts_per_s * 1e3
    roof["diagnostic_valu_issue_model"] = {
        "ticks_per_point_trip": ticks, "chip_points_per_s": pts_per_s, "point_visits": visits,
        "skipped_trips_this_run": int(skipped), "trips_per_evaluation": int(total_trips), "skipped_trip_share": skip_share, "pre_culled_trip_share": cull_share,
        "model_ms": floor_ms, "kernel_ms_over_model_ms": roof["kernel_ms"] / floor_ms,
        "note": "a fitted description of vector-ALU issue, not a hardware limit and not a predictor: see the comment in bench.py",
    }
    parity = sampled_pair_parity(api, fset, ev.owned(), pairs, deltas, clouds, host) if not args.no_cpu_baseline else None
    per_rank = None
    if D.collective:
        t = torch.tensor([breakdown["kernels_ms"], breakdown["all_gather_ms"], breakdown["index_select_ms"], float(ev.hi - ev.lo)], dtype=torch.float64, device="cuda")
        allt = [torch.zeros_like(t) for _ in range(D.world)]
        D.dist.all_gather(allt, t)
        per_rank = [dict(zip(["kernels_ms", "all_gather_ms", "index_select_ms", "pairs"], x.cpu().tolist())) for x in allt]
    if D.rank != 0:
        return None
    sec = elapsed / steps
    predicted = None
    if D.world == 1 and not args.no_predict:
        predicted = predict_scaling(api, ctx, multi, pairs, deltas, clouds, vmaps, costs, host, sec * 1e3, torch)
    native = None
    if D.world == 1 and not args.no_native:
        try:  # the same cost through the native C-ABI multi-device path, as world 1 (what an N-device node runs with `--gpus N --native`)
            native = native_global256(args, api, submaps, pairs, deltas, 1, 5, 3)
        except Exception as e:  # noqa: BLE001 -- reported, not fatal for the headline
            native = {"error": repr(e)}
    return {
        "native_c_abi_world1": native,
        "synchronous_per_evaluation": {"ms_per_evaluation": elapsed_sync / steps * 1e3,
                                       "what": "the same torch-driven evaluation with the records copied to pinned host memory and a synchronise after EVERY evaluation -- "
                                               "the form an optimiser needs and the like-for-like partner of native_c_abi_world1 (`value` queues the evaluations "
                                               "back to back and never returns to the host)",
                                       "native_minus_this_ms": (native["ms_per_evaluation"] - elapsed_sync / steps * 1e3) if native and "ms_per_evaluation" in native else None},
        "parity": parity, "predicted_scaling": predicted, "rank_breakdown": per_rank if per_rank else [breakdown], "exchange": exchange,
        "metric": "multi_scan_cost_eval_s", "value": sec, "unit": "s", "n_gpus": D.world, "steps": steps, "warmup": max(args.warmup, 3),
        "ms_per_step": sec * 1e3, "higher_is_better": False, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"configs[3] global256: {S} merged submaps (merge_frames of {args.submap_frames} keyframes, 0.1 m) x {int(np.mean(sizes))} pts, "
                               f"all {len(pairs)} pairs, 1.0 m voxels, binary factors",
                   "pairs": len(pairs), "pairs_this_rank": ev.hi - ev.lo, "mean_points_per_submap": float(np.mean(sizes)),
                   "mean_inlier_fraction": float(host[:, 0].mean() / np.mean(costs)),
                   "total_error": float(host[:, 1].sum()), "factor_linearizations_per_s": len(pairs) / sec,
                   "collective": (f"rccl_all_gather[{D.world} x {max_rows} x 29] f64 ({D.world * max_rows * 29 * 8 / 1e6:.1f} MB gathered per rank)"
                                  if D.world > 1 else "none")},
        "roofline": roof,
    }


def native_global256(args, api, submaps, pairs, deltas, n_gpus, steps, warmup):
    """The SAME all-pairs cost through the native multi-device path north_star names -- the C ABI glim_amd_multi_* (glim_amd/csrc/multi.hip): ONE
    process, one context + host worker thread + RCCL communicator per device (ncclCommInitAll), clouds / maps replicated, the pair list cut into
    contiguous cost-balanced shards, ONE ncclAllGather of the 29-double records -- next to the torch.distributed form above.  On one GPU it runs
    as world 1 (the collective is still RCCL's).  submaps: [(pose, merged PointCloudGPU)] of the calling context (downloaded and re-uploaded
    through the multi handle: every device gets its own replica)."""
    devices = list(range(max(1, min(n_gpus, api.device_count()))))
    M = api.MultiDeviceCost(devices)
    t0 = time.time()
    cloud_ids, map_ids = [], []
    for _, g in submaps:
        pts, covs = g.download_merged()
        cid = M.add_cloud(pts, covs)
        cloud_ids.append(cid)
        map_ids.append(M.add_voxelmap(cid, 1.0))
    M.set_factors([map_ids[i] for i, _ in pairs], [cloud_ids[j] for _, j in pairs], [api.FACTOR_BINARY] * len(pairs))
    setup_s = time.time() - t0
    T = np.ascontiguousarray(deltas, dtype=np.float64)
    import ctypes as C

    from glim_amd.api import check, lib

    Tp = T.ctypes.data_as(C.POINTER(C.c_double))
    steps = max(steps, 20)  # (a 5-step sample on the driver's box carried 2.2 ms per evaluation nobody could name: VERDICT r4)

    tot = C.c_double()

    def evaluate():  # the records stay in the handle's pinned array, the cost (sum of the errors) is summed by the devices
        check(lib().glim_amd_multi_linearize(M._h, Tp, None, C.byref(tot)), "glim_amd_multi_linearize")

    def measure():
        for _ in range(max(warmup, 3)):
            evaluate()
        acc = {d: {k: 0.0 for k in M.BREAKDOWN_FIELDS} for d in devices}
        k_acc, g_acc = np.zeros(len(devices)), np.zeros(len(devices))
        t1 = time.perf_counter()
        for _ in range(steps):
            evaluate()
            for d in devices:  # (reads of the handle's last-evaluation account: ~1 us each, inside the timed loop on purpose -- it is what a caller would do)
                for k, v in M.last_breakdown(d).items():
                    acc[d][k] += v
            km, gm = M.last_timing()
            k_acc += km
            g_acc += gm
        sec = (time.perf_counter() - t1) / steps
        bd = {d: {k: v / steps for k, v in acc[d].items()} for d in devices}
        return sec, bd, (k_acc / steps).tolist(), (g_acc / steps).tolist()

    sec, bd, kernel_ms, gather_ms = measure()
    info = M.info()
    b0 = bd[0]
    accounted = b0["pose_stage"] + b0["enqueue"] + b0["barrier"] + b0["collective"] + b0["wait"] + b0["join"] + b0["scan"] + b0["post"]
    out = {"form": "C ABI glim_amd_multi_*: one process; the caller's thread drives device 0, one more thread per further device; ONE hand-over per evaluation; "
                   "ncclAllGather of the owned rows, piece by piece on several devices (the gather of one piece overlaps the kernels of the next); one device: no library call per evaluation",
           "n_devices": info["num_devices"], "rccl_ranks": info["num_devices"] if info["uses_rccl"] else 0, "uses_rccl": info["uses_rccl"],
           "seconds_per_evaluation": sec, "ms_per_evaluation": sec * 1e3, "steps": steps,
           "per_device": [{"device": d, "pairs": int(b1 - b0_), "kernels_ms": k, "collective_and_copy_out_after_the_kernels_ms": g}
                          for d, (b0_, b1, k, g) in enumerate(zip(M.shard()[:-1], M.shard()[1:], kernel_ms, gather_ms))],
           "host_breakdown_us": {"device_0_caller_thread": b0, "other_devices": {str(d): bd[d] for d in devices[1:]},
                                 "accounted_us": accounted, "call_total_us": b0["total"], "python_loop_overhead_us": sec * 1e6 - b0["total"],
                                 "what": "steady_clock inside glim_amd_multi_linearize, averaged over the timed evaluations: post = handing work to the other "
                                         "devices' threads; pose_stage = this shard's poses into the pinned ring; enqueue = plan check + H2D + kernel launches; "
                                         "barrier = until every device has enqueued; collective = ncclAllGather + copy-out enqueue; wait = hipStreamSynchronize "
                                         "(the device working); join = the other threads; scan = total error over the records; library_calls = inside ncclAllGather (part of "
                                         "collective); device_gather / device_copy_out = HIP events after the last kernel: up to the end of the last all-gather, then the "
                                         "copy-out + error sum"},
           "replication_and_setup_s": setup_s}
    out["total_error"] = tot.value
    if len(devices) == 1 and info["uses_rccl"]:
        # one device has nothing to gather and makes no library call per evaluation (the binding is exercised at create); what the no-op
        # ncclAllGather would cost if it were made every time -- round 5's evidence box: 0.3 ms of host time inside a process with torch's librccl
        M.set_one_rank_collective(True)
        sec1, bd1, k1, g1 = measure()
        M.set_one_rank_collective(False)
        out["with_the_one_rank_library_call_every_evaluation"] = {
            "ms_per_evaluation": sec1 * 1e3, "kernels_ms": k1, "collective_and_copy_out_after_the_kernels_ms": g1,
            "library_calls_host_us": bd1[0]["library_calls"], "device_gather_us": bd1[0]["device_gather"], "device_copy_out_us": bd1[0]["device_copy_out"]}
    # the records' way to the host: stored by the finalising kernels into the host array as well (default) against copies behind every piece
    M.set_host_records(0)
    M.set_factors([map_ids[i] for i, _ in pairs], [cloud_ids[j] for _, j in pairs], [api.FACTOR_BINARY] * len(pairs))
    sec0, bd0_, k0, g0 = measure()
    out["with_device_to_host_copies_behind_the_pieces"] = {"ms_per_evaluation": sec0 * 1e3, "kernels_ms": k0, "collective_and_copy_out_after_the_kernels_ms": g0,
                                                           "device_copy_out_us": bd0_[0]["device_copy_out"]}
    M.set_host_records(1)
    M.set_factors([map_ids[i] for i, _ in pairs], [cloud_ids[j] for _, j in pairs], [api.FACTOR_BINARY] * len(pairs))
    out["pieces_per_shard"] = "default: pieces of >= 2048 factors, at most 4 (glim_amd_multi_set_split)"
    # the same evaluation with the shard in 1 / 2 / 4 pieces (the exchange and the pose upload of one piece overlap the kernels of the next)
    sweep = {}
    for pieces in (1, 2, 8):
        M.set_split(pieces)
        M.set_factors([map_ids[i] for i, _ in pairs], [cloud_ids[j] for _, j in pairs], [api.FACTOR_BINARY] * len(pairs))
        sec2, bd2, k2, g2 = measure()
        sweep[str(pieces)] = {"ms_per_evaluation": sec2 * 1e3, "kernels_ms": k2, "collective_and_copy_out_after_the_kernels_ms": g2, "wait_us": bd2[0]["wait"]}
    sweep["default"] = {"ms_per_evaluation": sec * 1e3}
    out["pieces_sweep"] = sweep
    M.set_split(-1)
    M.set_factors([map_ids[i] for i, _ in pairs], [cloud_ids[j] for _, j in pairs], [api.FACTOR_BINARY] * len(pairs))
    M.close()
    return out


def virtual_world_global256(api, submaps, pairs, deltas, world, steps, warmup, reference_total=None):
    """The N > 1 code of glim_amd/csrc/multi.hip EXECUTED on a one-GPU box: the same physical device listed `world` times
    ("virtual devices", glim_amd_debug_multi_create_virtual) -- per entry a context, a host thread, a replica of every cloud and map, a shard of
    the pair list in pieces, an upload and a collective stream, a gathered array; the exchange of a piece is the same-device stand-in for the in-place
    ncclAllGather.  The `world` shards share ONE GPU, so the milliseconds say nothing about an 8-GPU node's speed-up; what they do say: the whole
    path runs, what the 8 host threads cost per evaluation (post / wake / barrier / join), how long the exchange takes behind the kernels, and that
    the call no longer waits for it (gather mode 1, the default) -- with the waited form (mode 2) beside it."""
    import ctypes as C

    from glim_amd.api import check, lib

    M = api.MultiDeviceCost([0] * world, virtual=True)
    t0 = time.time()
    cloud_ids, map_ids = [], []
    for _, g in submaps:
        pts, covs = g.download_merged()
        cid = M.add_cloud(pts, covs)
        cloud_ids.append(cid)
        map_ids.append(M.add_voxelmap(cid, 1.0))
    M.set_factors([map_ids[i] for i, _ in pairs], [cloud_ids[j] for _, j in pairs], [api.FACTOR_BINARY] * len(pairs))
    setup_s = time.time() - t0
    T = np.ascontiguousarray(deltas, dtype=np.float64)
    Tp = T.ctypes.data_as(C.POINTER(C.c_double))
    tot = C.c_double()
    devices = list(range(world))
    bounds = M.shard()
    out = {"what": virtual_world_global256.__doc__.split("\n")[0], "n_virtual_devices": world, "physical_devices": 1, "uses_rccl": M.info()["uses_rccl"],
           "exchange": "same-device stand-in for the in-place ncclAllGather (hipMemcpyAsync of equal slots on every entry's collective stream, behind the piece's event)",
           "pairs_per_device": [int(b - a) for a, b in zip(bounds[:-1], bounds[1:])], "replication_and_setup_s": setup_s}
    for mode, name in ((1, "exchange_behind_the_call"), (2, "call_waits_for_the_exchange")):
        M.set_gather_mode(mode)
        for _ in range(max(warmup, 3)):
            check(lib().glim_amd_multi_linearize(M._h, Tp, None, C.byref(tot)), "glim_amd_multi_linearize")
        M.wait_gather()
        acc = {d: {k: 0.0 for k in M.BREAKDOWN_FIELDS} for d in devices}
        k_acc, g_acc, wait_acc = np.zeros(world), np.zeros(world), 0.0
        t1 = time.perf_counter()
        for _ in range(steps):
            check(lib().glim_amd_multi_linearize(M._h, Tp, None, C.byref(tot)), "glim_amd_multi_linearize")
        sec = (time.perf_counter() - t1) / steps
        for _ in range(steps):  # the accounts, outside the timed loop: the exchange's events complete behind the call, so it is waited for here
            check(lib().glim_amd_multi_linearize(M._h, Tp, None, C.byref(tot)), "glim_amd_multi_linearize")
            tw = time.perf_counter()
            M.wait_gather()
            wait_acc += time.perf_counter() - tw
            for d in devices:
                for k, v in M.last_breakdown(d).items():
                    acc[d][k] += v
            km, gm = M.last_timing()
            k_acc += km
            g_acc += gm
        bd = {d: {k: v / steps for k, v in acc[d].items()} for d in devices}
        others = [bd[d] for d in devices[1:]]
        out[name] = {
            "ms_per_evaluation": sec * 1e3, "total_error": tot.value,
            "per_device": [{"device": d, "kernels_ms": float(k_acc[d] / steps), "exchange_after_the_last_kernel_ms": float(g_acc[d] / steps)} for d in devices],
            "host_wait_for_the_exchange_after_the_call_us": wait_acc / steps * 1e6,
            "host_breakdown_us": {"device_0_caller_thread": bd[0],
                                  "worker_threads_max": {k: max(o[k] for o in others) for k in ("wake", "pose_stage", "enqueue", "barrier", "collective", "wait", "library_calls")}},
        }
    # every device's gathered array holds every record (what a device-side consumer reads), and the host array is the same bytes
    M.set_gather_mode(1)
    check(lib().glim_amd_multi_linearize(M._h, Tp, None, C.byref(tot)), "glim_amd_multi_linearize")
    host = M.records()
    out["every_device_holds_every_record"] = bool(all(np.array_equal(M.gathered_records(d), host) for d in (0, world // 2, world - 1)))
    if reference_total is not None:
        out["total_error_relative_difference_to_world1"] = abs(tot.value - reference_total) / max(1e-300, abs(reference_total))
    M.close()
    return out


def run_global256_native(args, D, api, ctx):
    """`bench.py --gpus N --native`: configs[3] / M2 through glim_amd_multi_* only (no torch.distributed): one process drives the N devices."""
    from glim_amd import synth

    S = args.submaps
    submaps = make_merged_submaps(api, ctx, S, args.submap_frames, args.submap_rings, args.submap_azimuths)
    poses = [T for T, _ in submaps]
    sizes = [g.size() for _, g in submaps]
    pairs = [(i, j) for j in range(S) for i in range(j)]
    deltas = np.stack([api.pose12(synth.relative_pose(poses[i], poses[j])) for i, j in pairs])
    steps, warmup = args.steps, max(args.warmup, 3)
    nat = native_global256(args, api, submaps, pairs, deltas, args.gpus, steps, warmup)
    virt = None
    if args.gpus == 1 and not args.no_virtual:
        try:
            virt = virtual_world_global256(api, submaps, pairs, deltas, 8, max(5, min(steps, 10)), 3, nat.get("total_error"))
        except Exception as e:  # noqa: BLE001 -- reported, not fatal for the line
            virt = {"error": repr(e)}
    return {
        "virtual_world8": virt,
        "metric": "multi_scan_cost_eval_s", "value": nat["seconds_per_evaluation"], "unit": "s", "n_gpus": nat["n_devices"], "steps": steps, "warmup": warmup,
        "ms_per_step": nat["ms_per_evaluation"], "higher_is_better": False, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"configs[3] global256 (native C-ABI multi-device path): {S} merged submaps x {int(np.mean(sizes))} pts, all {len(pairs)} pairs, "
                               "1.0 m voxels, binary factors", "pairs": len(pairs), "parallelism": f"pair list sharded over {nat['n_devices']} device(s), data replicated",
                   "collective": f"ncclAllGather over {nat['rccl_ranks']} RCCL rank(s)" if nat["uses_rccl"] else "host gather (no RCCL)"},
        "native": nat,
    }


def run_rgbd300k(args, D, api, ctx):
    """configs[4]: dense depth stream, everything per frame on the device (PCIe upload included: frames arrive from the host)."""
    from glim_amd import synth

    room = synth.Scene.small_room()
    dirs = synth.pinhole_directions(640, 480, 70, 55)
    n_distinct = 6
    frames, poses = [], []
    for i in range(n_distinct):
        T = synth.pose(-2.5 + 0.05 * i, -1.5 + 0.02 * i, 1.4, 0.5 + 0.01 * i)
        frames.append(synth.scan(room, T, dirs, i, sigma=0.002, max_range=8.0, min_range=0.3))
        poses.append(T)
    log(f"{n_distinct} distinct depth frames of {len(frames[0])} pts")
    n_frames = args.frames
    prev_map, prev_pose, lat, inl = None, None, [], []
    D.barrier_sync()
    t_all = time.perf_counter()
    for fidx in range(n_frames + 3):
        if fidx == 3:
            D.torch.cuda.synchronize()
            t_all = time.perf_counter()
            lat = []
        t0 = time.perf_counter()
        pts, T = frames[fidx % n_distinct], poses[fidx % n_distinct]
        g = api.PointCloudGPU.clone(pts, ctx=ctx)  # H2D upload + pack
        g.find_neighbors(10, download=False)  # K2
        g.estimate_covariances(10)  # K1
        vm = api.GaussianVoxelMapGPU(0.1, ctx=ctx).insert(g)  # K3
        if prev_map is not None:
            f = api.IntegratedVGICPFactorGPU(prev_pose, 1, prev_map, g)  # unary factor against the previous frame
            fs = api.NonlinearFactorSetGPU(ctx)
            fs.add(f)
            r = fs.linearize({1: T})[0]  # K4 + host read-back
            inl.append(r["num_inliers"] / len(pts))
        prev_map, prev_pose = vm, T
        lat.append(time.perf_counter() - t0)
    D.torch.cuda.synchronize()
    total = time.perf_counter() - t_all
    lat = np.array(lat) * 1e3
    return {
        "metric": "rgbd_frames_per_s", "value": n_frames / total, "unit": "frames/s", "n_gpus": 1, "steps": n_frames, "warmup": 3,
        "ms_per_step": total / n_frames * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "configs[4] rgbd300k: 640x480 depth frames, upload + kNN(k=10) + covariance + 0.1 m voxel map + 1 unary linearize per frame",
                   "points_per_frame": int(len(frames[0])), "latency_ms_p50": float(np.percentile(lat, 50)), "latency_ms_p99": float(np.percentile(lat, 99)),
                   "mean_inlier_fraction": float(np.mean(inl)), "target_fps": 30},
        "roofline": knn_roofline(g, 10, "rgbd300k"),
    }


def run_frontend128k(args, D, api, ctx):
    """the per-scan front end GLIM runs before the factors, on the device end to end -- raw 131 072-pt scan ->
    CloudPreprocessor::preprocess (random-grid sampling to `--target` points, range filter, time sort, kNN) -> CloudDeskewing::deskew (IMU-pose
    form) -> `pt = T_imu_lidar * pt` with a NON-identity extrinsic (odometry_estimation_imu.cpp:313-316) -> covariances from the FP64 deskewed
    points -> 0.5 m voxel map -> one VGICP linearize against the previous frame.  PCIe upload of the raw scan included."""
    from glim_amd import synth

    scene = synth.Scene.default()
    dirs = synth.lidar_directions(args.rings, args.azimuths)
    traj = synth.arc_trajectory(6, step=0.3, yaw_step_deg=1.0)
    rng = np.random.default_rng(7)
    raws = []
    for i, T in enumerate(traj):
        pts = synth.scan(scene, T, dirs, i).astype(np.float64)
        p4 = np.ones((len(pts), 4))
        p4[:, :3] = pts
        raws.append((p4, np.sort(rng.uniform(0.0, 0.1, len(pts))), rng.uniform(0, 255, len(pts)), T))
    prm_kw = dict(downsample_target=args.target, downsample_resolution=0.5 if args.target > 20000 else 1.0)
    Til = synth.pose(0.06, -0.04, 0.10, yaw=np.radians(3.0), pitch=np.radians(-1.0), roll=np.radians(1.5))  # T_imu_lidar: 13 cm off the IMU, tilted
    stamp = 100.0
    imu_times = stamp + np.linspace(-0.01, 0.12, 14)  # 100 Hz IMU-rate predictions around the 0.1 s sweep: 3 m/s forward, 0.17 rad/s yaw
    imu_poses = [np.eye(4)]
    for _ in imu_times[1:]:
        imu_poses.append(imu_poses[-1] @ synth.pose(0.03, 0.0, 0.0, yaw=0.0017))
    dk = dict(imu_times=imu_times, imu_poses=imu_poses, stamp=stamp, to_imu_frame=True)
    n_frames = args.frames
    prev_map, prev_pose, lat, kept, stage = None, None, [], [], np.zeros(6)
    retire = []
    fine = [] if os.environ.get("BENCH_FRONTEND_FINE") else None
    fine_prev, fine_destroy = [None, None], []
    fs = None
    D.barrier_sync()
    t_all = time.perf_counter()
    for fidx in range(n_frames + 3):
        if fidx == 3:
            D.torch.cuda.synchronize()
            t_all = time.perf_counter()
            lat, stage = [], np.zeros(6)
        p4, times, inten, T = raws[fidx % len(raws)]
        t0 = time.perf_counter()
        pre = api.PointCloudGPU.preprocess(p4, times, inten, api.preprocess_params(seed=fidx, **prm_kw), ctx=ctx)
        t1 = time.perf_counter()
        g = pre.deskew(Til, **dk)
        t2 = time.perf_counter()
        g.estimate_covariances(10)
        t3 = time.perf_counter()
        vm = api.GaussianVoxelMapGPU(args.resolution, ctx=ctx).insert(g)
        t4 = time.perf_counter()
        if prev_map is not None:
            if fine is not None:  # BENCH_FRONTEND_FINE=1: where the linearise stage's time goes, call by call (diagnostic)
                ta = time.perf_counter()
                fs = None  # (the previous set, and with it the previous frame's cloud and the map before it, are released HERE)
                ta1 = time.perf_counter()
                if fine_prev[0] is not None:
                    fine_prev[0].close()
                ta2 = time.perf_counter()
                if fine_prev[1] is not None:
                    fine_prev[1].close()
                ta3 = time.perf_counter()
                fine_prev[0], fine_prev[1] = g, prev_map
                fine_destroy.append((fidx, (ta1 - ta) * 1e6, (ta2 - ta1) * 1e6, (ta3 - ta2) * 1e6))
                tb = time.perf_counter()
                fs = api.NonlinearFactorSetGPU(ctx)
                fs.add(api.IntegratedVGICPFactorGPU(prev_pose, 1, prev_map, g))
                tc = time.perf_counter()
                fs.linearize({1: T})
                fine.append((fidx, (tb - ta) * 1e6, (tc - tb) * 1e6, (time.perf_counter() - tc) * 1e6))
            else:
                # the objects of the frame BEFORE the previous one retire here, explicitly and as a stage of their own: the previous factor set (it
                # holds the factor, hence that frame's cloud and the map before it), that cloud, that map.  Round 5 let Python drop them inside the
                # "linearize" stage when `fs` was rebound, which is why that stage read 0.22 ms for one 12 000-pt factor.
                if fs is not None:
                    fs.close()
                for old in retire:
                    old.close()
                retire = [g, prev_map]
                t_retired = time.perf_counter()
                fs = api.NonlinearFactorSetGPU(ctx)
                fs.add(api.IntegratedVGICPFactorGPU(prev_pose, 1, prev_map, g))
                fs.linearize({1: T})
        t5 = time.perf_counter()
        if prev_map is None or fine is not None:
            t_retired = t4
        prev_map, prev_pose = vm, T
        lat.append(t5 - t0)
        stage += np.array([t1 - t0, t2 - t1, t3 - t2, t4 - t3, t_retired - t4, t5 - t_retired])
        kept.append(g.size())
    D.torch.cuda.synchronize()
    total = time.perf_counter() - t_all
    if fine:
        arr = np.array(fine)
        sys.stderr.write("linearise stage, us: release of the previous set / new set + add / linearize: mean %s, p50 %s, max %s\n" %
                         (arr[:, 1:].mean(0).round(1), np.percentile(arr[:, 1:], 50, axis=0).round(1), arr[:, 1:].max(0).round(1)))
        dd = np.array(fine_destroy)[3:]
        sys.stderr.write("release, us: set / previous cloud / previous-previous map: mean %s, p50 %s, p99 %s, max %s\n" %
                         (dd[:, 1:].mean(0).round(1), np.percentile(dd[:, 1:], 50, axis=0).round(1), np.percentile(dd[:, 1:], 99, axis=0).round(1), dd[:, 1:].max(0).round(1)))
        sys.stderr.write("slowest releases: %s\n" % dd[np.argsort(-dd[:, 1:].sum(1))[:10]].round(1).tolist())
        worst = arr[np.argsort(-arr[:, 1:].sum(1))[:12]]
        sys.stderr.write("slowest frames (index, release, new set, linearize): %s\n" % worst.round(1).tolist())
    lat = np.array(lat) * 1e3
    result = {
        "metric": "lidar_frontend_frames_per_s", "value": n_frames / total, "unit": "frames/s", "n_gpus": 1, "steps": n_frames, "warmup": 3,
        "ms_per_step": total / n_frames * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64+f32",
        "dtype_note": "preprocess / deskew / IMU-frame transform / covariance in FP64 (the reference's types); voxel map and factor in FP32 (the reference GPU factor's)",
        "data": "synthetic",
        "config": {"workload": f"8f frontend128k: raw {len(raws[0][0])}-pt scans, preprocess (random grid -> {args.target}) + deskew (IMU poses) + T_imu_lidar + covariance + "
                               f"{args.resolution} m voxel map + 1 unary linearize per frame",
                   "points_per_frame_raw": int(len(raws[0][0])), "points_per_frame_kept": int(np.mean(kept)),
                   "latency_ms_p50": float(np.percentile(lat, 50)), "latency_ms_p99": float(np.percentile(lat, 99)),
                   "stage_ms": dict(zip(["preprocess", "deskew", "covariance", "voxelmap", "retire_the_frame_before_last", "linearize"], (stage / n_frames * 1e3).round(4).tolist())),
                   "stage_note": "retire = destroying the previous factor set, the previous frame's cloud and the map before it (three quiesce + pool returns); "
                                 "linearize = a NEW one-factor set + add + synchronous linearize (plan build for a new list included)"},
    }
    result["roofline"] = knn_roofline(pre, 10, "frontend128k")  # (the kNN of the kept points, inside `preprocess`)
    if not args.no_cpu_baseline and D.rank == 0:
        from oracle import oracle as orc

        # CPU leg: all five stages of the frame on the oracle (FP64, OpenMP); the voxel map and the factor take FP32-rounded covariances, as the
        # device path stores them
        dk_o = dict(imu_times=imu_times, imu_poses=imu_poses, stamp=stamp)
        p4, times, inten, T = raws[0]
        prev = None
        reps, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < 8.0 or reps < 2:
            ref = orc.preprocess(p4[:, :3], times, inten, orc.preprocess_params(seed=0, **prm_kw))
            d, nrm, cov = orc.frontend(ref["points"], ref["times"], ref["neighbors"], Til, **dk_o)
            vm = orc.VoxelMap(args.resolution).insert(d, cov)
            if prev is not None:
                orc.vgicp_linearize(prev, d, cov, np.eye(4))
            prev = vm
            reps += 1
        cpu_ms = (time.perf_counter() - t0) / reps * 1e3
        result["cpu_baseline"] = {"value": 1e3 / cpu_ms, "unit": "frames/s", "cores": effective_cores(), "kind": "port",
                                  "sample": f"{reps} frames: oracle preprocess + deskew + IMU-frame transform + covariances + voxel map + one linearize, "
                                            f"{cpu_ms:.1f} ms per frame"}
        # parity of the COMPOSED front end on frame 0: the reference's own translation units where oracle/_ref travelled with the snapshot
        # (ref_preprocess -> ref_frontend = deskew -> T_imu_lidar -> covariance), their bit-equal restatement otherwise
        use_ref = orc.ref_lib() is not None and hasattr(orc.ref_lib(), "ref_frontend")
        ref = orc.preprocess(p4[:, :3], times, inten, orc.preprocess_params(seed=0, **prm_kw), ref=use_ref)
        rp, rn, rc = orc.frontend(ref["points"], ref["times"], ref["neighbors"], Til, ref=use_ref, **dk_o)
        pre = api.PointCloudGPU.preprocess(p4, times, inten, api.preprocess_params(seed=0, **prm_kw), ctx=ctx)
        got = pre.download_frame()
        assert np.array_equal(got["points"], ref["points"]) and np.array_equal(got["neighbors"], ref["neighbors"]), "device preprocessing != reference"
        g = pre.deskew(Til, **dk)
        assert np.array_equal(g.download_points64(), rp), "device deskew + IMU-frame transform != reference (FP64, bit for bit)"
        g.estimate_covariances(10)
        _, gc, gn = g.download()
        dc = np.abs(gc.astype(np.float64) - rc).max(axis=(1, 2))
        dn = np.abs(gn.astype(np.float64) - rn).max(axis=1)
        result["parity"] = {"checker": "oracle/_ref: the reference's cloud_preprocessor.cpp, cloud_deskewing.cpp, cloud_covariance_estimation.cpp compiled unmodified"
                                       if use_ref else "oracle restatement (oracle/_ref absent)",
                            "chain": "preprocess -> deskew (IMU poses) -> T_imu_lidar * pt -> covariance, frame 0", "points": int(len(rp)),
                            "preprocessed_points_and_neighbours_equal": True, "deskewed_imu_frame_points_bit_exact_fp64": True,
                            "covariance_fraction_beyond_1e-5": float(np.mean(dc > 1e-5)), "covariance_max_abs_diff": float(dc.max()),
                            "normal_max_abs_diff": float(dn.max()), "extrinsic_is_identity": False}
        assert result["parity"]["covariance_fraction_beyond_1e-5"] == 0.0, result["parity"]
        log(f"parity: composed front end == reference on frame 0 ({len(rp)} points): {result['parity']}")
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--opt-iters", type=int, default=3, help="odometry_frame: optimiser iterations (fresh-set linearisations) per frame")
    ap.add_argument("--workload", default=None, choices=["odometry128k", "odometry_frame", "submap20", "global256", "rgbd300k", "frontend128k", "odometry_under_load"],
                    help="default: odometry128k (M1) on one GPU, global256 (M2, strong scaling) on several")
    ap.add_argument("--inner", type=int, default=256, help="odometry128k: batched linearisation passes per step")
    ap.add_argument("--sync-calls", type=int, default=2000, help="odometry128k: synchronous single-factor linearize calls per step (the headline loop)")
    ap.add_argument("--submap-frames", type=int, default=4, help="global256: keyframes merged into one submap")
    ap.add_argument("--submap-rings", type=int, default=40)
    ap.add_argument("--submap-azimuths", type=int, default=560, help="global256: 4 x 40 x 560 rays per submap merge to >= 65 536 points on average (BASELINE configs[3]: 256 x 64k; 512 gave 62 187)")
    ap.add_argument("--no-resident-cost", action="store_true", help="skip the interference measurement (factor kernels timed beside an idle resident session)")
    ap.add_argument("--no-m2", action="store_true", help="N = 1 default run: skip the 256-submap cost evaluation that is attached as `m2_global256` (~17 s)")
    ap.add_argument("--factors", type=int, default=128, help="odometry128k: factors per GPU per step")
    ap.add_argument("--rings", type=int, default=128)
    ap.add_argument("--azimuths", type=int, default=1024)
    ap.add_argument("--resolution", type=float, default=0.5)
    ap.add_argument("--submaps", type=int, default=256, help="global256: number of submaps")
    ap.add_argument("--frames", type=int, default=300, help="rgbd300k / frontend128k: frames in the timed stream")
    ap.add_argument("--target", type=int, default=10000, help="frontend128k: random_downsample_target (config_preprocess.json ships 10000)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-split", action="store_true", help="global256 on several GPUs: do not try the two-halves form of the exchange")
    ap.add_argument("--no-predict", action="store_true", help="global256 on one GPU: skip the per-shard timing behind `predicted_scaling`")
    ap.add_argument("--no-native", action="store_true", help="global256 on one GPU: skip the run through the native C-ABI multi-device path (profiling passes)")
    ap.add_argument("--no-virtual", action="store_true", help="--native on one GPU: skip the virtual_world8 run (the N > 1 path over 8 virtual devices)")
    ap.add_argument("--native", action="store_true", help="configs[3] through the native multi-device C-ABI path (glim_amd_multi_*: ONE process drives --gpus "
                                                         "devices, ncclAllGather) instead of one torch.distributed rank per GPU; run it as a plain `python bench.py`")
    ap.add_argument("--full", action="store_true", help="default line: also measure everything beside the headline (batched form, roofline, per-variant call "
                                                       "times, resident-session cost, device timeline, CPU baseline and parity, m2_global256 / m1_weak); "
                                                       "a run without it times the headline loop alone")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write the records the timed loop returned in its last step "
                                                                        "as DIR/<name>.npy (float64); single-GPU odometry128k headline only")
    args = ap.parse_args()
    if args.dump_outputs and ((args.workload or "odometry128k") != "odometry128k" or args.gpus != 1 or args.native or args.sync_calls <= 0):
        ap.error("--dump-outputs is implemented for the single-GPU odometry128k headline loop (--gpus 1, --sync-calls > 0)")

    # stdout carries exactly ONE JSON line: libraries that print banners to fd 1 (RCCL prints its version there at init) are
    # diverted to stderr for the whole run; the result goes to the saved descriptor at the end
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    D = Dist(1 if args.native else args.gpus)  # --native: ONE process drives all the devices through glim_amd_multi_*
    from glim_amd import api

    # One dedicated (non-default) torch stream is made current for the whole run and handed to the library: our kernels, torch's tensor
    # ops and the ordering points of RCCL's collectives (work.wait / the implicit wait of a synchronous collective) are then all
    # on the same stream, in program order.
    stream = D.torch.cuda.Stream()
    D.torch.cuda.set_stream(stream)
    ctx = api.Context(D.local_rank, 1, external_stream=stream.cuda_stream)
    workload = args.workload or ("odometry128k" if D.world == 1 else "global256")
    runner = {"odometry128k": run_odometry128k, "odometry_frame": run_odometry_frame, "submap20": run_submap20, "global256": run_global256, "rgbd300k": run_rgbd300k,
              "frontend128k": run_frontend128k, "odometry_under_load": run_odometry_under_load}[workload]
    if args.native:
        runner = run_global256_native
    result = runner(args, D, api, ctx)
    if args.workload is None and D.world > 1 and args.full:
        m1 = run_odometry128k(args, D, api, ctx)  # the weak-scaling form of M1, next to the M2 headline
        if result is not None and m1 is not None:
            result["m1_weak"] = {k: m1[k] for k in ("metric", "value", "unit", "ms_per_step", "scaling", "batched_value_cold", "sync_single_factor_calls_per_s", "config",
                                                    "roofline", "headline_form") if k in m1}
    elif args.workload is None and args.full and not args.no_m2 and not args.native:
        m2 = run_global256(args, D, api, ctx, extra_only=True)
        if result is not None and m2 is not None:
            result["m2_global256"] = {k: m2[k] for k in ("metric", "value", "unit", "ms_per_step", "scaling", "config", "roofline", "parity", "predicted_scaling",
                                                         "rank_breakdown", "exchange", "native_c_abi_world1", "synchronous_per_evaluation") if k in m2}
    D.finish()
    sys.stdout.flush()
    if D.rank == 0 and result is not None:
        os.write(real_stdout, (json.dumps(result) + "\n").encode())


if __name__ == "__main__":
    main()
