"""The scenes and builders that the global-registration tests share (test_fpfh*, test_ransac*, test_gnc*): a plain module beside the
*_restatement.py files, no fixtures.  Every array comes from a fixed seed, so two test modules that ask for the same case see the same bytes."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def motion(yaw, pitch, t):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    M = np.eye(4)
    M[:3, :3] = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    M[:3, 3] = t
    return M


def rot(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def room_scan(sigma):
    """one LiDAR scan of the small room (floor, ceiling, four walls, boxes), range noise sigma"""
    from glim_amd import synth

    return synth.scan(synth.Scene.small_room(), synth.pose(0.5, -0.3, 1.2, yaw=0.3), synth.lidar_directions(32, 256), 0, sigma=sigma)[:, :3]


def room_points(n, seed):
    pts = room_scan(0.01)
    return pts[np.sort(np.random.default_rng(seed).choice(len(pts), n, replace=False))].astype(np.float32)


def make_case(source, seed, clutter, extent, redirected=0.30, unmatched=0.05, noise=0.0, pitch=0.25):
    """target = rigid copy of the source (+ Gaussian noise) + `clutter` random points; nearest = identity with a share redirected at random and a
    share set to -1"""
    rng = np.random.default_rng(seed)
    M = motion(0.6, pitch, [1.5, -2.0, 0.4])
    copy = (source.astype(np.float64) @ M[:3, :3].T + M[:3, 3] + noise * rng.normal(size=(len(source), 3))).astype(np.float32)
    target = np.concatenate([copy, rng.uniform(-extent, extent, (clutter, 3)).astype(np.float32)])
    n = len(source)
    nearest = np.arange(n, dtype=np.int32)
    pick = rng.permutation(n)
    k1, k2 = int(redirected * n), int(unmatched * n)
    nearest[pick[:k1]] = rng.integers(0, len(target), k1)
    nearest[pick[k1:k1 + k2]] = -1
    return {"source": source, "target": target, "nearest": nearest, "M": M}


def upload(ctx, case):
    from glim_amd import api

    return api.PointCloudGPU.clone(case["target"], ctx=ctx), api.PointCloudGPU.clone(case["source"], ctx=ctx)


def result_bytes(r):
    return r.T_target_source.tobytes() + struct.pack("<dqii", r.inlier_rate, r.num_inliers, r.best_iteration, r.iterations_run)


def crop_points():
    """two overlapping crops along x of 2 000 points of a room scan: 1 537 target and 1 000 source points, 537 in both"""
    pts = room_points(2000, 11)
    order = np.argsort(pts[:, 0], kind="stable")
    return {"target": pts[np.sort(order[:1537])], "source": pts[np.sort(order[-1000:])]}


def described_crops(ctx):
    """crop_points() on the device with normals (kNN 10) and FPFH descriptors (r = 0.6 m): name -> (cloud, descriptors, points)"""
    from glim_amd import api

    out = {}
    for name, pts in crop_points().items():
        c = api.PointCloudGPU.clone(pts, ctx=ctx)
        c.find_neighbors(10, download=False)
        c.estimate_covariances(10)
        out[name] = (c, c.estimate_fpfh(0.6), pts)
    return out


def write_drop_in_case(path, described, dof, seed, result):
    """case.bin of tests/cpp/registration_case.hpp: the two crops, their descriptors and the result the C++ drop-in has to reproduce"""
    (_, tf, tp), (_, sf, sp) = described["target"], described["source"]
    with open(path, "wb") as fh:
        fh.write(struct.pack("<iiiQ", len(tp), len(sp), dof, seed))
        for p in (tp, sp):
            p4 = np.ones((len(p), 4))
            p4[:, :3] = p
            fh.write(p4.tobytes())
        for f in (tf, sf):
            fh.write(f.download().astype(np.float64).tobytes())
        fh.write(np.ascontiguousarray(result.T_target_source[:3]).tobytes())
        fh.write(struct.pack("<d", result.inlier_rate))


def build_drop_in_cpp(tmp_path, name):
    """tests/cpp/<name>.cpp over the drop-in tree and the stand-in GLIM headers"""
    from glim_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "adapters", "gtsam_points_hip"), "-I" + os.path.join(ROOT, "adapters", "gtsam"),
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "cpp", "glim_standin"), os.path.join(ROOT, "tests", "cpp", name + ".cpp"),
           "-o", exe, "-L" + os.path.join(ROOT, "glim_amd"), "-lglim_amd", "-Wl,-rpath," + os.path.join(ROOT, "glim_amd"), "-Wl,-rpath,/opt/rocm/lib",
           "-L/opt/rocm/lib", "-lamdhip64"]
    subprocess.check_call(cmd)
    return exe


def build_pose_program(tmp_path_factory, name):
    """tests/cpp/test_<name>.cpp (a pose header on the CPU) built plain and under -fsanitize=address,undefined: (directory, (plain, sanitized))"""
    d = tmp_path_factory.mktemp(name)
    src = os.path.join(ROOT, "tests", "cpp", "test_" + name + ".cpp")
    plain, san = str(d / "pose"), str(d / "pose_san")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", src, "-o", plain])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", san])
    return d, (plain, san)
