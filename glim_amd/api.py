"""Host-side mirror of the gtsam_points GPU interface GLIM uses for the VGICP hot path.

Same names and argument meaning as the reference-side classes so that tests read like the reference's call sites:

    frame     = PointCloudGPU.clone(points, covs)                    # odometry_estimation_gpu.cpp:96
    voxelmap  = GaussianVoxelMapGPU(resolution); voxelmap.insert(frame)   # :103-104
    factor    = IntegratedVGICPFactorGPU(target_key, source_key, voxelmap, frame)   # :144  (binary)
    factor    = IntegratedVGICPFactorGPU(fixed_target_pose, source_key, voxelmap, frame)   # :161  (unary)
    factor.set_enable_surface_validation(True)                       # :145
    fset      = NonlinearFactorSetGPU(); fset.add(factor); fset.linearize(values)   # :383-386
    overlap   = overlap_gpu(voxelmap, frame, delta)                  # :248

Everything below is a thin ctypes shim over the C ABI (include/glim_amd.h); all arithmetic happens in the HIP kernels.
`Values` is a plain dict {key: 4x4 pose}; a linearised factor is returned as the HessianFactor ingredients.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import CtLinearized, FACTOR_BINARY, FACTOR_SURFACE_VALIDATION, GlimAmdError, Linearized6, PreprocessParams, check, lib  # noqa: F401

_default_ctx = None
STREAM_LEGACY = 1  # hipStreamLegacy ((hipStream_t)1): the null stream, as an explicit handle
STREAM_PER_THREAD = 2  # hipStreamPerThread


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None


def pose12(T):
    T = np.asarray(T, dtype=np.float64)
    if T.size == 12:
        return np.ascontiguousarray(T).reshape(12)
    return np.ascontiguousarray(T[:3, :4]).reshape(12)


def device_count():
    return lib().glim_amd_device_count()


class Context:
    """Device + stream pool (gtsam_points::CUDAStream / StreamTempBufferRoundRobin)."""

    def __init__(self, device=0, num_streams=1, external_stream=None, priority=0):
        """priority: 0 default, 1 = the device's greatest stream priority (the odometry's context), -1 = its least."""
        h = C.c_void_p()
        ext = None
        if external_stream is not None:
            # 0 is the legacy default stream (what torch.cuda.current_stream().cuda_stream returns for torch's default stream): the C ABI
            # takes the HIP handle for it, hipStreamLegacy, because NULL means "create private streams"
            ext = C.c_void_p(int(external_stream) if int(external_stream) != 0 else STREAM_LEGACY)
        check(lib().glim_amd_ctx_create_ex(int(device), int(num_streams), ext, int(priority), C.byref(h)), "glim_amd_ctx_create_ex")
        self._h = h
        self.device = device

    def synchronize(self):
        check(lib().glim_amd_ctx_synchronize(self._h), "glim_amd_ctx_synchronize")

    def set_diag(self, key_values=""):
        """Diagnostic switches of this context ("key=value,key=value"; "" restores the process defaults): include/glim_amd.h."""
        check(lib().glim_amd_ctx_set_diag(self._h, key_values.encode()), "glim_amd_ctx_set_diag")

    def diag(self, key_values=""):
        """Context manager: the process defaults + `key_values` inside the block, the process defaults again on the way out -- whatever
        happens inside.  (set_diag ADDS to the switches in force; tests and measurements that flip kernel paths use this instead, so that a
        failure between two set_diag calls cannot leave a shared context in the wrong mode.)"""
        import contextlib

        @contextlib.contextmanager
        def scope():
            self.set_diag("")
            try:
                if key_values:
                    self.set_diag(key_values)
                yield self
            finally:
                if self._h:
                    self.set_diag("")

        return scope()

    def get_diag(self):
        buf = C.create_string_buffer(1024)
        check(lib().glim_amd_ctx_get_diag(self._h, buf, 1024), "glim_amd_ctx_get_diag")
        return dict(kv.split("=", 1) for kv in buf.value.decode().split(","))

    def device_info(self):
        name = C.create_string_buffer(256)
        free, total, cus = C.c_size_t(), C.c_size_t(), C.c_int()
        check(lib().glim_amd_device_info(self._h, name, 256, C.byref(free), C.byref(total), C.byref(cus)), "glim_amd_device_info")
        return {"name": name.value.decode(), "free_bytes": free.value, "total_bytes": total.value, "num_cus": cus.value}

    def close(self):
        """Destroys the context.  Refused (GlimAmdError, the context stays usable) while clouds / maps / factor sets made from it are alive."""
        if self._h:
            check(lib().glim_amd_ctx_destroy(self._h), "glim_amd_ctx_destroy")
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0, 1)
    return _default_ctx


class PointCloudGPU:
    """gtsam_points::PointCloudGPU -- device-resident FP32 SoA copy of a frame."""

    def __init__(self, handle, ctx):
        self._h = handle
        self.ctx = ctx

    @staticmethod
    def clone(points, covs=None, normals=None, ctx=None):
        """points: N x 3 or N x 4 (homogeneous); covs: N x 3 x 3 or N x 4 x 4 (Matrix4d); normals: N x 3 / N x 4.
        float64 inputs travel in the reference's Vector4d / Matrix4d layout and are packed on the device; float32 inputs use
        the compact entry point."""
        ctx = ctx or default_context()
        points = np.asarray(points)
        n = points.shape[0]
        h = C.c_void_p()
        if points.dtype == np.float32 and (covs is None or np.asarray(covs).dtype == np.float32):
            xyz = np.ascontiguousarray(points[:, :3], dtype=np.float32)
            c = None if covs is None else np.ascontiguousarray(np.asarray(covs, dtype=np.float32)[:, :3, :3]).reshape(n, 9)
            nr = None if normals is None else np.ascontiguousarray(np.asarray(normals, dtype=np.float32)[:, :3])
            check(lib().glim_amd_cloud_create_f32(ctx._h, n, _fp(xyz), _fp(c), _fp(nr), C.byref(h)), "glim_amd_cloud_create_f32")
        else:
            p4 = np.ones((n, 4), dtype=np.float64)
            p4[:, : min(4, points.shape[1])] = points[:, :4]
            p4[:, 3] = 1.0
            c16 = None
            if covs is not None:
                covs = np.asarray(covs, dtype=np.float64)
                m = np.zeros((n, 4, 4))
                m[:, :3, :3] = covs[:, :3, :3]
                c16 = np.ascontiguousarray(np.transpose(m, (0, 2, 1))).reshape(n, 16)  # column-major Matrix4d
            n4 = None
            if normals is not None:
                normals = np.asarray(normals, dtype=np.float64)
                n4 = np.zeros((n, 4))
                n4[:, :3] = normals[:, :3]
            check(lib().glim_amd_cloud_create(ctx._h, n, _dp(p4), _dp(c16), _dp(n4), C.byref(h)), "glim_amd_cloud_create")
        return PointCloudGPU(h, ctx)

    @staticmethod
    def clone_packed(points4, covs16=None, normals4=None, ctx=None):
        """PointCloudGPU::clone of arrays that already have the reference's layout (n x Vector4d, n x column-major Matrix4d): nothing is
        repacked on the Python side, so timing this call times the library."""
        ctx = ctx or default_context()
        h = C.c_void_p()
        check(lib().glim_amd_cloud_create(ctx._h, len(points4), _dp(points4), _dp(covs16), _dp(normals4), C.byref(h)), "glim_amd_cloud_create")
        return PointCloudGPU(h, ctx)

    @staticmethod
    def clone_deskewed(points, times, T_imu_lidar, imu_times=None, imu_poses=None, stamp=0.0, linear_vel=None, angular_vel=None, ctx=None,
                       to_imu_frame=False):
        """CloudDeskewing::deskew (cloud_deskewing.cpp) fused with PointCloudGPU::clone: IMU-pose form when imu_times / imu_poses are
        given, constant-velocity form otherwise.  to_imu_frame: also apply `pt = T_imu_lidar * pt` (odometry_estimation_imu.cpp:314-316),
        the step both reference callers take before estimating covariances."""
        ctx = ctx or default_context()
        points = np.asarray(points, dtype=np.float64)
        n = points.shape[0]
        p4 = np.ones((n, 4), dtype=np.float64)
        p4[:, :3] = points[:, :3]
        t = np.ascontiguousarray(times, dtype=np.float64).reshape(n)
        Til = pose12(T_imu_lidar)
        it = ip = None
        n_imu = 0
        if imu_times is not None and len(imu_times) > 0:
            it = np.ascontiguousarray(imu_times, dtype=np.float64)
            ip = np.ascontiguousarray(np.stack([pose12(P) for P in imu_poses]))
            n_imu = len(it)
        lv = None if linear_vel is None else np.ascontiguousarray(linear_vel, dtype=np.float64)
        av = None if angular_vel is None else np.ascontiguousarray(angular_vel, dtype=np.float64)
        h = C.c_void_p()
        check(lib().glim_amd_cloud_create_deskewed(ctx._h, n, _dp(p4), _dp(t), _dp(Til), n_imu, _dp(it), _dp(ip), float(stamp), _dp(lv), _dp(av),
                                                   int(bool(to_imu_frame)), C.byref(h)), "glim_amd_cloud_create_deskewed")
        return PointCloudGPU(h, ctx)

    @staticmethod
    def preprocess(points, times, intensities=None, params=None, ctx=None):
        """CloudPreprocessor::preprocess (cloud_preprocessor.cpp:92-188) on the device: returns the preprocessed cloud (points, times,
        intensities, kNN resident in HBM); `download_frame()` gives the PreprocessedFrame fields."""
        ctx = ctx or default_context()
        prm = params if params is not None else preprocess_params()
        points = np.asarray(points, dtype=np.float64)
        n = points.shape[0]
        if points.ndim == 2 and points.shape[1] == 4 and points.flags.c_contiguous:
            p4 = points  # already the reference's Vector4d layout: handed over as it is (a 131 072-point copy costs as much as the whole call)
        else:
            p4 = np.ones((n, 4), dtype=np.float64)
            p4[:, : points.shape[1]] = points
        t = np.ascontiguousarray(times, dtype=np.float64).reshape(n)
        it = None if intensities is None else np.ascontiguousarray(intensities, dtype=np.float64).reshape(n)
        h = C.c_void_p()
        check(lib().glim_amd_preprocess(ctx._h, n, _dp(p4), _dp(t), _dp(it), C.byref(prm), C.byref(h)), "glim_amd_preprocess")
        g = PointCloudGPU(h, ctx)
        g._k = prm.k_correspondences
        g._has_intensities = it is not None
        return g

    def download_frame(self):
        """PreprocessedFrame fields (include/glim/preprocess/preprocessed_frame.hpp:26-39) of a preprocessed cloud."""
        n, k = self.size(), getattr(self, "_k", 0)
        p4, t = np.zeros((n, 4)), np.zeros(n)
        it = np.zeros(n) if getattr(self, "_has_intensities", False) else None
        nb = np.zeros((n, k), dtype=np.int32) if k > 0 else None
        check(lib().glim_amd_cloud_download_frame(self._h, _dp(p4), _dp(t), _dp(it), _ip(nb)), "glim_amd_cloud_download_frame")
        return dict(points=p4[:, :3].copy(), times=t, intensities=it, neighbors=nb, k_neighbors=k)

    def save_compact(self, directory):
        """gtsam_points::PointCloud::save_compact (sub_map.cpp:62): *_compact.bin files inside `directory`."""
        check(lib().glim_amd_cloud_save_compact(self._h, str(directory).encode()), "glim_amd_cloud_save_compact")

    @staticmethod
    def load_compact(directory, ctx=None):
        """gtsam_points::PointCloudCPU::load (sub_map.cpp:142) + clone."""
        ctx = ctx or default_context()
        h = C.c_void_p()
        check(lib().glim_amd_cloud_load_compact(ctx._h, str(directory).encode(), C.byref(h)), "glim_amd_cloud_load_compact")
        return PointCloudGPU(h, ctx)

    def download_merged(self):
        """The merged submap as PointCloudCPU holds it: (points N x 3, covs N x 3 x 3), exact FP64."""
        n = self.size()
        p4, c16 = np.zeros((n, 4)), np.zeros((n, 16))
        check(lib().glim_amd_cloud_download_merged(self._h, _dp(p4), _dp(c16)), "glim_amd_cloud_download_merged")
        return p4[:, :3].copy(), np.transpose(c16.reshape(n, 4, 4)[:, :3, :3], (0, 2, 1)).copy()

    def download_points64(self):
        """The exact FP64 points a preprocessed / deskewed / merged cloud keeps next to its FP32 image (N x 3)."""
        p4 = np.zeros((self.size(), 4))
        check(lib().glim_amd_cloud_download_frame(self._h, _dp(p4), None, None, None), "glim_amd_cloud_download_frame")
        return p4[:, :3].copy()

    def deskew(self, T_imu_lidar, imu_times=None, imu_poses=None, stamp=0.0, linear_vel=None, angular_vel=None, to_imu_frame=False):
        """CloudDeskewing::deskew of a preprocessed cloud that is already on the device; the raw-scan neighbours are carried over.
        to_imu_frame: followed by `pt = T_imu_lidar * pt` (odometry_estimation_imu.cpp:314-316, sub_mapping.cpp:368-370)."""
        Til = pose12(T_imu_lidar)
        it = ip = None
        n_imu = 0
        if imu_times is not None and len(imu_times) > 0:
            it = np.ascontiguousarray(imu_times, dtype=np.float64)
            ip = np.ascontiguousarray(np.stack([pose12(P) for P in imu_poses]))
            n_imu = len(it)
        lv = None if linear_vel is None else np.ascontiguousarray(linear_vel, dtype=np.float64)
        av = None if angular_vel is None else np.ascontiguousarray(angular_vel, dtype=np.float64)
        h = C.c_void_p()
        check(lib().glim_amd_cloud_deskew(self._h, _dp(Til), n_imu, _dp(it), _dp(ip), float(stamp), _dp(lv), _dp(av), int(bool(to_imu_frame)), C.byref(h)),
              "glim_amd_cloud_deskew")
        g = PointCloudGPU(h, self.ctx)
        g._k = getattr(self, "_k", 0)
        return g

    def size(self):
        n = C.c_int64()
        check(lib().glim_amd_cloud_size(self._h, C.byref(n)), "glim_amd_cloud_size")
        return n.value

    def memory_usage_gpu(self):
        b = C.c_size_t()
        check(lib().glim_amd_cloud_memory_usage(self._h, C.byref(b)), "glim_amd_cloud_memory_usage")
        return b.value

    def find_neighbors(self, k, download=True):
        """CloudPreprocessor::find_neighbors on the device; returns N x k int32 when download."""
        out = np.zeros((self.size(), k), dtype=np.int32) if download else None
        check(lib().glim_amd_cloud_find_neighbors(self._h, int(k), _ip(out)), "glim_amd_cloud_find_neighbors")
        return out

    def set_neighbors(self, neighbors):
        nb = np.ascontiguousarray(neighbors, dtype=np.int32)
        check(lib().glim_amd_cloud_set_neighbors(self._h, nb.shape[1], _ip(nb)), "glim_amd_cloud_set_neighbors")

    def profile_neighbors(self, k=10, iters=20):
        """(wall ms per find_neighbors call, HIP-event ms of the query-group kernel inside it): glim_amd_cloud_profile_neighbors."""
        a, b = C.c_float(), C.c_float()
        check(lib().glim_amd_cloud_profile_neighbors(self._h, int(k), int(iters), C.byref(a), C.byref(b)), "glim_amd_cloud_profile_neighbors")
        return a.value, b.value

    def estimate_covariances(self, k_neighbors):
        """CloudCovarianceEstimation::estimate on the device (fills covs + normals)."""
        check(lib().glim_amd_cloud_estimate_covariances(self._h, int(k_neighbors)), "glim_amd_cloud_estimate_covariances")

    def estimate_fpfh(self, search_radius):
        """gtsam_points::estimate_fpfh on the device (the cloud needs normals): FPFHFeatures, row i = point i."""
        h = C.c_void_p()
        check(lib().glim_amd_fpfh_estimate(self._h, float(search_radius), C.byref(h)), "glim_amd_fpfh_estimate")
        return FPFHFeatures(h, self.ctx)

    def download(self, covs=True, normals=True):
        n = self.size()
        xyz = np.zeros((n, 3), dtype=np.float32)
        c = np.zeros((n, 9), dtype=np.float32) if covs else None
        nr = np.zeros((n, 3), dtype=np.float32) if normals else None
        check(lib().glim_amd_cloud_download(self._h, _fp(xyz), _fp(c), _fp(nr), None), "glim_amd_cloud_download")
        return xyz, (c.reshape(n, 3, 3) if covs else None), nr

    def _derived(self, h):
        """a cloud one of the resampling calls made of this one: neighbours are not carried over, intensities are"""
        g = PointCloudGPU(h, self.ctx)
        g._k = 0
        g._has_intensities = getattr(self, "_has_intensities", False)
        return g

    def random_sampling(self, rate, seed=0):
        """gtsam_points::random_sampling on the device: a NEW cloud of int(size * rate) points in their original order, with every per-point
        array this one holds (rate >= 0.99: a copy of the whole cloud).  The draw is glim_amd_cloud_random_sample's, a function of (seed, size)."""
        h = C.c_void_p()
        check(lib().glim_amd_cloud_random_sample(self._h, float(rate), int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(h)), "glim_amd_cloud_random_sample")
        return self._derived(h)

    def sample(self, indices):
        """gtsam_points::sample on the device: a NEW cloud whose point j is this one's point indices[j] (any order, duplicates allowed)."""
        idx = np.ascontiguousarray(np.asarray(indices, dtype=np.int32).reshape(-1))
        h = C.c_void_p()
        check(lib().glim_amd_cloud_sample(self._h, len(idx), _ip(idx) if len(idx) else None, C.byref(h)), "glim_amd_cloud_sample")
        return self._derived(h)

    def transform(self, T):
        """gtsam_points::transform on the device: a NEW cloud with points, covariances and normals moved by T (4 x 4 or 3 x 4; the linear part
        need not be a rotation), in FP64 with the operation order include/glim_amd.h states."""
        T12 = np.ascontiguousarray(np.asarray(T, dtype=np.float64)[:3, :4]).reshape(12)
        h = C.c_void_p()
        check(lib().glim_amd_cloud_transform(self._h, _dp(T12), C.byref(h)), "glim_amd_cloud_transform")
        return self._derived(h)

    def close(self):
        if self._h:
            lib().glim_amd_cloud_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


FPFH_DIM = 33
FPFH_RECIPROCAL = 0x1


class FPFHFeatures:
    """n x 33 FP32 FPFH descriptors on the device (glim_amd_fpfh; semantics in include/glim_amd.h)."""

    def __init__(self, handle, ctx):
        self._h = handle
        self.ctx = ctx

    def size(self):
        n = C.c_int64()
        check(lib().glim_amd_fpfh_size(self._h, C.byref(n)), "glim_amd_fpfh_size")
        return n.value

    def download(self):
        out = np.zeros((self.size(), FPFH_DIM), dtype=np.float32)
        check(lib().glim_amd_fpfh_download(self._h, _fp(out)), "glim_amd_fpfh_download")
        return out

    @classmethod
    def from_host(cls, descriptors, ctx=None):
        """descriptors that are already on the host (n x 33, narrowed to FP32) as a device object: glim_amd_fpfh_create"""
        ctx = ctx or default_context()
        d = np.ascontiguousarray(descriptors, dtype=np.float32).reshape(-1, FPFH_DIM)
        h = C.c_void_p()
        check(lib().glim_amd_fpfh_create(ctx._h, len(d), _fp(d), C.byref(h)), "glim_amd_fpfh_create")
        return cls(h, ctx)

    def close(self):
        if self._h:
            lib().glim_amd_fpfh_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def match_fpfh(target, source, reciprocal=False):
    """Nearest target descriptor of every source descriptor (squared L2, ties to the smaller index): (nearest int32, sqdist float32), one entry
    per source row.  reciprocal: nearest is -1 unless the source row is also the nearest source of its target (GNC's reciprocal_check)."""
    n = source.size()
    nearest = np.full(n, -1, dtype=np.int32)
    sqdist = np.full(n, np.inf, dtype=np.float32)
    check(lib().glim_amd_fpfh_match(target._h, source._h, FPFH_RECIPROCAL if reciprocal else 0, _ip(nearest), _fp(sqdist)), "glim_amd_fpfh_match")
    return nearest, sqdist


class RansacParams:
    """gtsam_points::RANSACParams (glim_amd_ransac_params); the defaults are the loop-close modal's."""

    def __init__(self, max_iterations=5000, early_stop_inlier_rate=0.9, poly_error_thresh=0.5, inlier_voxel_resolution=1.0, dof=6, seed=0):
        self.max_iterations = max_iterations
        self.early_stop_inlier_rate = early_stop_inlier_rate
        self.poly_error_thresh = poly_error_thresh
        self.inlier_voxel_resolution = inlier_voxel_resolution
        self.dof = dof
        self.seed = seed

    def _c(self):
        return _lib.RansacParams(int(self.max_iterations), float(self.early_stop_inlier_rate), float(self.poly_error_thresh),
                                 float(self.inlier_voxel_resolution), int(self.dof), int(self.seed) & 0xFFFFFFFFFFFFFFFF)


class RegistrationResult:
    """gtsam_points::RegistrationResult: T_target_source (4 x 4), inlier_rate; plus num_inliers, best_iteration (-1: none), iterations_run"""

    def __init__(self, c):
        self.T_target_source = np.eye(4)
        self.T_target_source[:3, :4] = np.array(c.T_target_source[:], dtype=np.float64).reshape(3, 4)
        self.inlier_rate = c.inlier_rate
        self.num_inliers = c.num_inliers
        self.best_iteration = c.best_iteration
        self.iterations_run = c.iterations_run


def _c_params(params, default):
    """the C block of `params`, or of default() when the caller passed none"""
    return (params or default())._c()


def _nearest(nearest, source=None):
    """`nearest` as contiguous int32; with `source` (the *_align functions) it must hold one entry per source point"""
    near = np.ascontiguousarray(nearest, dtype=np.int32)
    if source is not None and near.shape != (source.size(),):
        raise ValueError("nearest must hold one entry per source point")
    return near


def ransac_align(target, source, nearest, params=None):
    """gtsam_points::estimate_pose_ransac on the device: nearest[i] = target point matched to source point i, or -1 (match_fpfh's output)."""
    prm = _c_params(params, RansacParams)
    near = _nearest(nearest, source)
    out = _lib.RegistrationResult()
    check(lib().glim_amd_ransac_align(target._h, source._h, _ip(near), C.byref(prm), C.byref(out)), "glim_amd_ransac_align")
    return RegistrationResult(out)


def ransac_align_fpfh(target, source, target_fpfh, source_fpfh, params=None, reciprocal=False):
    """The same with the nearest-descriptor correspondences found on the device (they never visit the host)."""
    prm = _c_params(params, RansacParams)
    out = _lib.RegistrationResult()
    check(lib().glim_amd_ransac_align_fpfh(target._h, source._h, target_fpfh._h, source_fpfh._h, FPFH_RECIPROCAL if reciprocal else 0, C.byref(prm),
                                           C.byref(out)), "glim_amd_ransac_align_fpfh")
    return RegistrationResult(out)


def ransac_debug_hypotheses(target, source, nearest, params, first, count):
    """Test window (glim_amd_ransac_debug_hypotheses): every hypothesis of [first, first + count) scored, no early stop."""
    prm = params._c()
    near = _nearest(nearest)
    samples = np.zeros((count, 3), dtype=np.int32)
    status = np.zeros(count, dtype=np.int32)
    poses = np.zeros((count, 12), dtype=np.float64)
    inliers = np.zeros(count, dtype=np.int32)
    slots, in_lds = C.c_int32(), C.c_int32()
    check(lib().glim_amd_ransac_debug_hypotheses(target._h, source._h, _ip(near), C.byref(prm), int(first), int(count), _ip(samples), _ip(status),
                                                 _dp(poses), _ip(inliers), C.byref(slots), C.byref(in_lds)), "glim_amd_ransac_debug_hypotheses")
    return {"samples": samples, "status": status, "poses": poses, "inliers": inliers, "table_slots": slots.value, "table_in_lds": in_lds.value}


def ransac_profile(target, source, nearest, params, iters=20):
    """microseconds of the hypothesis / scoring / fold kernels of one round (HIP events inside the library)"""
    prm = params._c()
    near = _nearest(nearest)
    us = [C.c_float() for _ in range(3)]
    slots, in_lds = C.c_int32(), C.c_int32()
    check(lib().glim_amd_ransac_profile(target._h, source._h, _ip(near), C.byref(prm), int(iters), C.byref(us[0]), C.byref(us[1]), C.byref(us[2]),
                                        C.byref(slots), C.byref(in_lds)), "glim_amd_ransac_profile")
    return {"hypothesis_us": us[0].value, "score_us": us[1].value, "fold_us": us[2].value, "table_slots": slots.value, "table_in_lds": in_lds.value}


class GncParams:
    """gtsam_points::GNCParams (glim_amd_gnc_params; include/glim_amd.h "GNC").  reciprocal_check is gnc_align_fpfh's `reciprocal` argument."""

    def __init__(self, max_init_samples=5000, tuple_check=False, tuple_thresh=0.9, max_num_tuples=1000, div_factor=1.4, max_iterations=64,
                 max_corr_dist=0.0, inlier_voxel_resolution=1.0, dof=6, seed=0):
        self.max_init_samples = max_init_samples
        self.tuple_check = tuple_check
        self.tuple_thresh = tuple_thresh
        self.max_num_tuples = max_num_tuples
        self.div_factor = div_factor
        self.max_iterations = max_iterations
        self.max_corr_dist = max_corr_dist
        self.inlier_voxel_resolution = inlier_voxel_resolution
        self.dof = dof
        self.seed = seed

    def _c(self):
        return _lib.GncParams(int(self.max_init_samples), 1 if self.tuple_check else 0, float(self.tuple_thresh), int(self.max_num_tuples),
                              float(self.div_factor), int(self.max_iterations), float(self.max_corr_dist), float(self.inlier_voxel_resolution),
                              int(self.dof), int(self.seed) & 0xFFFFFFFFFFFFFFFF)


def _gnc_result(out, info):
    r = RegistrationResult(out)
    r.info = {k: getattr(info, k) for k, _ in _lib.GncInfo._fields_}
    return r


def gnc_align(target, source, nearest, params=None):
    """gtsam_points::estimate_pose_gnc on the device: nearest[i] = target point matched to source point i, or -1 (match_fpfh's output).
    Returns a RegistrationResult with `info` (glim_amd_gnc_info as a dict)."""
    prm = _c_params(params, GncParams)
    near = _nearest(nearest, source)
    out, info = _lib.RegistrationResult(), _lib.GncInfo()
    check(lib().glim_amd_gnc_align(target._h, source._h, _ip(near), C.byref(prm), C.byref(out), C.byref(info)), "glim_amd_gnc_align")
    return _gnc_result(out, info)


def gnc_align_fpfh(target, source, target_fpfh, source_fpfh, params=None, reciprocal=True):
    """The same with the nearest-descriptor correspondences found on the device (they never visit the host); reciprocal = GNCParams::reciprocal_check."""
    prm = _c_params(params, GncParams)
    out, info = _lib.RegistrationResult(), _lib.GncInfo()
    check(lib().glim_amd_gnc_align_fpfh(target._h, source._h, target_fpfh._h, source_fpfh._h, FPFH_RECIPROCAL if reciprocal else 0, C.byref(prm),
                                        C.byref(out), C.byref(info)), "glim_amd_gnc_align_fpfh")
    return _gnc_result(out, info)


def gnc_debug_trace(target, source, nearest, params):
    """Test window (glim_amd_gnc_debug_trace): the final list (n x 2: source, target index), c_s, c_t, D2, per completed iteration mu / W / cost /
    pose (3 x 4), the last iteration's weights, and the result gnc_align returns on the same arguments."""
    prm = params._c()
    near = _nearest(nearest)
    cap = max(source.size(), 3 * int(params.max_num_tuples) if params.tuple_check else 0, 1)
    pairs = np.zeros((cap, 2), dtype=np.int32)
    length = C.c_int64()
    frame = np.zeros(7)
    iters = np.zeros((int(params.max_iterations), 15))
    weights = np.zeros(cap)
    out, info = _lib.RegistrationResult(), _lib.GncInfo()
    check(lib().glim_amd_gnc_debug_trace(target._h, source._h, _ip(near), C.byref(prm), cap, _ip(pairs), C.byref(length), _dp(frame), _dp(iters),
                                         _dp(weights), C.byref(out), C.byref(info)), "glim_amd_gnc_debug_trace")
    r = _gnc_result(out, info)
    k, n = r.iterations_run, length.value
    return {"list": pairs[:n].copy(), "c_s": frame[0:3].copy(), "c_t": frame[3:6].copy(), "D2": float(frame[6]), "mu": iters[:k, 0].copy(),
            "W": iters[:k, 1].copy(), "cost": iters[:k, 2].copy(), "poses": iters[:k, 3:].reshape(k, 3, 4).copy(),
            "weights": weights[:n].copy() if k > 0 else np.zeros(0), "result": r}


def gnc_profile(target, source, nearest, params, iters=20):
    """microseconds of the stages of one gnc_align (HIP events inside the library)"""
    prm = params._c()
    near = _nearest(nearest)
    us = [C.c_float() for _ in range(5)]
    check(lib().glim_amd_gnc_profile(target._h, source._h, _ip(near), C.byref(prm), int(iters), *[C.byref(u) for u in us]), "glim_amd_gnc_profile")
    return dict(zip(("select_us", "tuples_us", "gather_and_solve_us", "table_us", "score_us"), (u.value for u in us)))


class GaussianVoxelMapGPU:
    """gtsam_points::GaussianVoxelMapGPU(resolution, init_num_buckets, max_bucket_scan_count, target_points_drop_rate)."""

    def __init__(self, resolution, init_num_buckets=8192 * 2, max_bucket_scan_count=10, target_points_drop_rate=1e-3, ctx=None):
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        check(lib().glim_amd_voxelmap_create(self.ctx._h, float(resolution), int(init_num_buckets), int(max_bucket_scan_count),
                                             float(target_points_drop_rate), C.byref(h)), "glim_amd_voxelmap_create")
        self._h = h
        self._frame = None

    def voxel_resolution(self):
        return self.voxelmap_info()["voxel_resolution"]

    def insert(self, frame):
        check(lib().glim_amd_voxelmap_insert(self._h, frame._h), "glim_amd_voxelmap_insert")
        return self

    def set_lru_horizon(self, lru_horizon, lru_clear_cycle=10):
        """GaussianVoxelMapCPU::set_lru_horizon (odometry_estimation_cpu.cpp:67): voxels untouched for more than `lru_horizon` inserts are dropped
        every `lru_clear_cycle` inserts; <= 0 switches eviction off (default)."""
        check(lib().glim_amd_voxelmap_set_lru_horizon(self._h, int(lru_horizon), int(lru_clear_cycle)), "glim_amd_voxelmap_set_lru_horizon")
        return self

    def voxelmap_info(self):
        nv, nb, res, by = C.c_int32(), C.c_int32(), C.c_double(), C.c_size_t()
        check(lib().glim_amd_voxelmap_info(self._h, C.byref(nv), C.byref(nb), C.byref(res), C.byref(by)), "glim_amd_voxelmap_info")
        return {"num_voxels": nv.value, "num_buckets": nb.value, "voxel_resolution": res.value, "bytes": by.value}

    def voxels(self):
        """(coords V x 3, counts V, means V x 3, covs V x 3 x 3), unspecified order."""
        v = self.voxelmap_info()["num_voxels"]
        coords = np.zeros((v, 3), dtype=np.int32)
        counts = np.zeros(v, dtype=np.int32)
        means = np.zeros((v, 3), dtype=np.float32)
        covs = np.zeros((v, 9), dtype=np.float32)
        check(lib().glim_amd_voxelmap_download(self._h, _ip(coords), _ip(counts), _fp(means), _fp(covs)), "glim_amd_voxelmap_download")
        return coords, counts, means, covs.reshape(v, 3, 3)

    def close(self):
        if self._h:
            lib().glim_amd_voxelmap_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IncrementalVoxelMap:
    """gtsam_points::IncrementalVoxelMap<FlatContainer> (gtsam_points::iVox) on the device: the incremental target model of the continuous-time
    odometry (odometry_estimation_ct.cpp:56-63, :229-235).  A flat list of at most `max_points` points per voxel of edge `leaf`; the target
    of IntegratedGICPFactor / IntegratedCT_GICPFactor (pass it as `target` / `target_tree`).  Semantics: include/glim_amd.h."""

    def __init__(self, leaf, ctx=None):
        self.ctx = ctx or default_context()
        self._h = None
        h = C.c_void_p()
        check(lib().glim_amd_ivox_create(self.ctx._h, float(leaf), C.byref(h)), "glim_amd_ivox_create")
        self._h = h
        self.leaf = float(leaf)
        self.min_dist, self.max_points = 0.1, 20
        self.lru_horizon, self.lru_clear_cycle = 10, 10

    def voxel_insertion_setting(self, min_dist=None, max_points=None):
        """voxel_insertion_setting().min_sq_dist_in_cell = min_dist^2 / .max_num_points_in_cell = max_points (1..64); before the first insert."""
        md = self.min_dist if min_dist is None else float(min_dist)
        mp = self.max_points if max_points is None else int(max_points)
        check(lib().glim_amd_ivox_set_insertion(self._h, md, mp), "glim_amd_ivox_set_insertion")
        self.min_dist, self.max_points = md, mp
        return self

    def set_lru_horizon(self, horizon):
        check(lib().glim_amd_ivox_set_lru(self._h, int(horizon), self.lru_clear_cycle), "glim_amd_ivox_set_lru")
        self.lru_horizon = int(horizon)
        return self

    def set_lru_clear_cycle(self, cycle):
        check(lib().glim_amd_ivox_set_lru(self._h, self.lru_horizon, int(cycle)), "glim_amd_ivox_set_lru")
        self.lru_clear_cycle = int(cycle)
        return self

    def set_neighbor_voxel_mode(self, mode):
        check(lib().glim_amd_ivox_set_neighbor_voxel_mode(self._h, int(mode)), "glim_amd_ivox_set_neighbor_voxel_mode")
        return self

    def insert(self, frame, T=None):
        """insert(frame); T (4 x 4 or 12): the frame's pose in the map, applied to points and covariances on the device."""
        t = None if T is None else pose12(T)
        check(lib().glim_amd_ivox_insert(self._h, frame._h, _dp(t)), "glim_amd_ivox_insert")
        return self

    def info(self):
        nv, npts, cnt, leaf = C.c_int32(), C.c_int64(), C.c_int32(), C.c_double()
        check(lib().glim_amd_ivox_info(self._h, C.byref(nv), C.byref(npts), C.byref(cnt), C.byref(leaf)), "glim_amd_ivox_info")
        return {"num_voxels": nv.value, "num_points": npts.value, "lru_counter": cnt.value, "leaf_size": leaf.value}

    def download(self):
        """(coords V x 3, counts V, points V x cap x 3, covs V x cap x 3 x 3) in slot order; places beyond a voxel's count are zero."""
        v, cap = self.info()["num_voxels"], self.max_points
        coords = np.zeros((v, 3), dtype=np.int32)
        counts = np.zeros(v, dtype=np.int32)
        points = np.zeros((v, cap, 3), dtype=np.float32)
        covs = np.zeros((v, cap, 9), dtype=np.float32)
        check(lib().glim_amd_ivox_download(self._h, _ip(coords), _ip(counts), _fp(points), _fp(covs)), "glim_amd_ivox_download")
        return coords, counts, points, covs.reshape(v, cap, 3, 3)

    def voxel_points(self):
        """voxel_points(): every stored point (N x 3, FP64), voxels in slot order (odometry_estimation_ct.cpp:302)."""
        p4 = np.zeros((self.info()["num_points"], 4))
        check(lib().glim_amd_ivox_voxel_points(self._h, _dp(p4)), "glim_amd_ivox_voxel_points")
        return p4[:, :3].copy()

    def debug_set_initial_capacity(self, slots):
        check(lib().glim_amd_debug_ivox_set_initial_capacity(self._h, int(slots)), "glim_amd_debug_ivox_set_initial_capacity")
        return self

    def debug_capacity(self):
        a, b = C.c_int32(), C.c_int32()
        check(lib().glim_amd_debug_ivox_capacity(self._h, C.byref(a), C.byref(b)), "glim_amd_debug_ivox_capacity")
        return {"slots": a.value, "table": b.value}

    def close(self):
        """Destroys the map.  Refused (GlimAmdError, the map stays usable) while a continuous-time factor built on it is alive."""
        if self._h:
            check(lib().glim_amd_ivox_destroy(self._h), "glim_amd_ivox_destroy")
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def frame_create(points4, covs16, normals4, resolutions, ctx=None):
    """glim_amd_frame_create: PointCloudGPU::clone + one GaussianVoxelMapGPU per resolution as ONE submission with one synchronise (create_frame of
    the GPU odometry).  Arrays in the reference's layout (n x Vector4d, n x column-major Matrix4d, n x Vector4d).  Returns (cloud, [maps])."""
    ctx = ctx or default_context()
    res = np.ascontiguousarray(resolutions, dtype=np.float64)
    hc = C.c_void_p()
    hm = (C.c_void_p * len(res))()
    check(lib().glim_amd_frame_create(ctx._h, len(points4), _dp(points4), _dp(covs16), _dp(normals4), len(res), _dp(res), C.byref(hc),
                                      C.cast(hm, C.POINTER(C.c_void_p))), "glim_amd_frame_create")
    maps = []
    for h in hm:
        m = GaussianVoxelMapGPU.__new__(GaussianVoxelMapGPU)
        m.ctx, m._h, m._frame = ctx, C.c_void_p(h), None
        maps.append(m)
    return PointCloudGPU(hc, ctx), maps


def _lin_to_dict(L):
    # one buffer view of the 976-byte struct (int64 + 121 doubles) instead of five element-wise ctypes -> numpy conversions
    a = np.frombuffer(L, dtype=np.float64, count=122).copy()
    return {
        "num_inliers": int(L.num_inliers),
        "error": float(a[1]),
        "H_tt": a[2:38].reshape(6, 6),
        "H_ss": a[38:74].reshape(6, 6),
        "H_ts": a[74:110].reshape(6, 6),
        "b_t": a[110:116],
        "b_s": a[116:122],
    }


class IntegratedVGICPFactorGPU:
    """gtsam_points::IntegratedVGICPFactorGPU.

    IntegratedVGICPFactorGPU(target_key, source_key, target_voxelmap, source)            binary
    IntegratedVGICPFactorGPU(fixed_target_pose(4x4), source_key, target_voxelmap, source)  unary
    """

    def __init__(self, target, source_key, target_voxelmap, source, stream=None, temp_buffer=None):
        self.is_binary = not (isinstance(target, np.ndarray) or isinstance(target, (list, tuple)))
        if self.is_binary:
            self.target_key = target
            self.fixed_target_pose = None
        else:
            self.target_key = None
            self.fixed_target_pose = np.array(target, dtype=np.float64).reshape(4, 4)
        self.source_key = source_key
        self.target_voxelmap = target_voxelmap
        self.source = source
        self.enable_surface_validation = False
        self._linearized = None  # filled by NonlinearFactorSetGPU (store_linearized in the reference's batch protocol)
        self._own_set = None

    # -- reference API ------------------------------------------------------------------------------------------
    def set_enable_surface_validation(self, enable):
        self.enable_surface_validation = bool(enable)
        self._own_set = None

    def keys(self):
        return [self.target_key, self.source_key] if self.is_binary else [self.source_key]

    def dim(self):
        return 6

    def get_fixed_target_pose(self):
        return self.fixed_target_pose

    def memory_usage(self):
        return 976  # one glim_amd_linearized6 on the host

    def memory_usage_gpu(self):
        return self.source.memory_usage_gpu() + self.target_voxelmap.voxelmap_info()["bytes"]

    def clone(self):
        f = IntegratedVGICPFactorGPU(self.target_key if self.is_binary else self.fixed_target_pose, self.source_key,
                                     self.target_voxelmap, self.source)
        f.enable_surface_validation = self.enable_surface_validation
        return f

    def flags(self):
        return (FACTOR_BINARY if self.is_binary else 0) | (FACTOR_SURFACE_VALIDATION if self.enable_surface_validation else 0)

    def calc_delta(self, values):
        """T_target_source at `values` (dict key -> 4x4)."""
        Ts = np.asarray(values[self.source_key], dtype=np.float64)
        Tt = np.asarray(values[self.target_key], dtype=np.float64) if self.is_binary else self.fixed_target_pose
        return np.linalg.inv(Tt) @ Ts

    def _single_set(self):
        if self._own_set is None:
            self._own_set = NonlinearFactorSetGPU(self.source.ctx)
            self._own_set.add(self)
        return self._own_set

    def linearize(self, values):
        """HessianFactor ingredients.  Uses the batch result when a NonlinearFactorSetGPU linearised this factor at the
        same values; otherwise performs its own upload/launch/download (the reference's slow path)."""
        delta = self.calc_delta(values)
        if self._linearized is not None and np.array_equal(self._linearized[0], delta):
            return self._linearized[1]
        self._single_set().linearize(values)
        return self._linearized[1]

    def error(self, values):
        return self._single_set().error(values)[0]

    def inlier_fraction(self):
        if self._linearized is None:
            return 0.0
        return self._linearized[1]["num_inliers"] / max(1, self.source.size())

    def align(self, T_init, params=None):
        """The fine registration of this (unary) factor's pair from T_init (4 x 4 T_target_source): vgicp_align_batch with one problem."""
        if self.is_binary:
            raise GlimAmdError(-1, "IntegratedVGICPFactorGPU.align", "a binary factor: the fine registration keeps the target fixed")
        return vgicp_align_batch([self.target_voxelmap], [self.source], [T_init], self.flags(), params)[0]


class NonlinearFactorSetGPU:
    """gtsam_points::NonlinearFactorSetGPU: linearises every added GPU factor in one fused launch."""

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        check(lib().glim_amd_factor_set_create(self.ctx._h, C.byref(h)), "glim_amd_factor_set_create")
        self._h = h
        self.factors = []

    def add(self, factor):
        if not isinstance(factor, IntegratedVGICPFactorGPU):
            return False  # non-GPU factors are ignored, like the reference
        idx = C.c_int32()
        check(lib().glim_amd_factor_set_add(self._h, factor.target_voxelmap._h, factor.source._h, factor.flags(), C.byref(idx)),
              "glim_amd_factor_set_add")
        self.factors.append(factor)
        return True

    def clear(self):
        check(lib().glim_amd_factor_set_clear(self._h), "glim_amd_factor_set_clear")
        self.factors = []

    def size(self):
        n = C.c_int32()
        check(lib().glim_amd_factor_set_size(self._h, C.byref(n)), "glim_amd_factor_set_size")
        return n.value

    def _poses(self, values):
        return np.ascontiguousarray(np.stack([pose12(f.calc_delta(values)) for f in self.factors])) if self.factors else np.zeros((0, 12))

    def linearize(self, values):
        n = len(self.factors)
        if n == 0:
            return []
        T = self._poses(values)
        out = (Linearized6 * n)()
        check(lib().glim_amd_factor_set_linearize(self._h, _dp(T), out), "glim_amd_factor_set_linearize")
        res = []
        for f, L, t in zip(self.factors, out, T):
            d = _lin_to_dict(L)
            delta = np.eye(4)
            delta[:3, :4] = t.reshape(3, 4)
            f._linearized = (delta, d)
            res.append(d)
        return res

    def linearize_poses(self, T_target_source):
        """Same with explicit n x 12 poses (no Values indirection)."""
        n = len(self.factors)
        T = np.ascontiguousarray(np.asarray(T_target_source, dtype=np.float64).reshape(n, 12))
        out = (Linearized6 * n)()
        check(lib().glim_amd_factor_set_linearize(self._h, _dp(T), out), "glim_amd_factor_set_linearize")
        return [_lin_to_dict(L) for L in out]

    def error(self, values, values_lin=None):
        n = len(self.factors)
        if n == 0:
            return []
        Te = self._poses(values)
        Tl = self._poses(values_lin) if values_lin is not None else None
        err = np.zeros(n)
        inl = np.zeros(n, dtype=np.int64)
        check(lib().glim_amd_factor_set_error(self._h, _dp(Tl), _dp(Te), _dp(err), inl.ctypes.data_as(C.POINTER(C.c_int64))),
              "glim_amd_factor_set_error")
        self.last_error_inliers = inl
        return list(err)

    def _optimize(self, align, name, values, priors, betweens, params, dampings=()):
        if any(not f.is_binary for f in self.factors):
            raise GlimAmdError(-1, "NonlinearFactorSetGPU." + name, "a unary factor: the bundle is over binary factors")
        validation = {f.enable_surface_validation for f in self.factors}
        if len(validation) > 1:
            raise GlimAmdError(-1, "NonlinearFactorSetGPU." + name, "surface validation on some factors only")
        keys = sorted(values)
        at = {k: i for i, k in enumerate(keys)}
        res = align([(f.target_voxelmap, f.source, at[f.target_key], at[f.source_key]) for f in self.factors],
                    [(at[k], P, info) for k, P, info in priors], [(at[b[0]], at[b[1]]) + tuple(b[2:]) for b in betweens],
                    [values[k] for k in keys], FACTOR_SURFACE_VALIDATION if validation == {True} else 0, params, self.ctx,
                    dampings=[(at[k], d) for k, d in dampings])
        return {k: res.poses[i] for i, k in enumerate(keys)}, res

    def optimize(self, values, priors=(), betweens=(), params=None, dampings=()):
        """The sub-map bundle optimisation over this set's factors, which must all be binary (bundle_align; the loop of sub_mapping.cpp:430-452
        with its PriorFactor and BetweenFactor terms).  values: {key: 4 x 4}; priors: (key, P 4 x 4, information 6 x 6); betweens: (key_i, key_j,
        D 4 x 4, information 6 x 6[, Huber width]); dampings: (key, scale or 6 values), as bundle_align has them.  The poses are ordered by sorted
        key.  Returns ({key: 4 x 4}, BundleResult).  The set itself is untouched."""
        return self._optimize(bundle_align, "optimize", values, priors, betweens, params, dampings)

    def optimize_graph(self, values, priors=(), betweens=(), params=None, dampings=()):
        """optimize() through the global-graph optimisation (graph_align; global_mapping.cpp:430-484): the same arguments and returns, up to
        _lib.GRAPH_MAX_POSES poses and _lib.GRAPH_MAX_FACTORS factors."""
        return self._optimize(graph_align, "optimize_graph", values, priors, betweens, params, dampings)

    def optimize_nav_graph(self, values, kinds, priors=(), betweens=(), vector_priors=(), vector_betweens=(), imu_terms=(), params=None, dampings=()):
        """optimize_graph() over pose, velocity and bias variables (graph_align_nav; the graphs of sub_mapping.cpp:218-243 and
        global_mapping.cpp:168-216 with enable_imu = true).  values: {key: 4 x 4 pose, 6 bias values or 3 velocity values}; kinds: {key:
        NODE_POSE / NODE_BIAS / NODE_VELOCITY}; vector_priors: (key, value, information); vector_betweens: (key_i, key_j, measurement,
        information); imu_terms: ImuTerm whose five nodes are keys.  The nodes are ordered by sorted key.  Returns ({key: value},
        NavGraphResult)."""
        if any(not f.is_binary for f in self.factors):
            raise GlimAmdError(-1, "NonlinearFactorSetGPU.optimize_nav_graph", "a unary factor: the graph is over binary factors")
        validation = {f.enable_surface_validation for f in self.factors}
        if len(validation) > 1:
            raise GlimAmdError(-1, "NonlinearFactorSetGPU.optimize_nav_graph", "surface validation on some factors only")
        keys = sorted(values)
        at = {k: i for i, k in enumerate(keys)}
        terms = [ImuTerm(*[at[k] for k in t.nodes], t.dt, t.gravity, t.bias_hat, t.delta, t.H_bias, t.information, t.mode) for t in imu_terms]
        res = graph_align_nav([(f.target_voxelmap, f.source, at[f.target_key], at[f.source_key]) for f in self.factors], [(at[k], P, info) for k, P, info in priors],
                              [(at[b[0]], at[b[1]]) + tuple(b[2:]) for b in betweens], [values[k] for k in keys], [kinds[k] for k in keys],
                              [(at[k], v, info) for k, v, info in vector_priors], [(at[i], at[j], d, info) for i, j, d, info in vector_betweens], terms,
                              [(at[k], d) for k, d in dampings], FACTOR_SURFACE_VALIDATION if validation == {True} else 0, params, self.ctx)
        return {k: res.nodes[i] for i, k in enumerate(keys)}, res

    def correspondences(self, index, delta):
        n = self.factors[index].source.size()
        corr = np.zeros((n, 4), dtype=np.int32)
        T = pose12(delta)
        check(lib().glim_amd_factor_set_correspondences(self._h, int(index), _dp(T), _ip(corr)), "glim_amd_factor_set_correspondences")
        return corr

    def cull_stats(self, reset=False):
        """Always None: the pre-cull of the general-form factor kernel is retired (measured on the global-map workload the pre-pass cost more than the
        walk it saved: profiles/r06/probe/precull_ab_take1_thread_per_row.json, precull_ab_take2_lane_per_trip.json).  Kept because bench.py asks."""
        return None

    def linearize_device_async(self, T_target_source, out_device_ptr, row_offset=0):
        T = T_target_source
        if not (isinstance(T, np.ndarray) and T.dtype == np.float64 and T.flags.c_contiguous and T.size == 12 * len(self.factors)):
            T = np.ascontiguousarray(np.asarray(T_target_source, dtype=np.float64).reshape(len(self.factors), 12))
        # raw addresses: building ctypes pointer objects costs several microseconds per call, which matters in launch-rate loops
        rc = lib().glim_amd_factor_set_linearize_device_async(self._h, C.cast(T.ctypes.data, C.POINTER(C.c_double)), C.c_void_p(out_device_ptr),
                                                              int(row_offset))
        if rc != 0:
            check(rc, "glim_amd_factor_set_linearize_device_async")

    def profile(self, T_target_source, iters=20):
        """(ms per fused VGICP kernel launch, ms per device-resident linearise) measured with HIP events on the set's stream."""
        T = np.ascontiguousarray(np.asarray(T_target_source, dtype=np.float64).reshape(len(self.factors), 12))
        a, b = C.c_float(), C.c_float()
        check(lib().glim_amd_factor_set_profile(self._h, _dp(T), int(iters), C.byref(a), C.byref(b)), "glim_amd_factor_set_profile")
        return a.value, b.value

    def trip_stats(self, reset=False):
        """(skipped wavefront trips since the last reset, trips per evaluation) of the general factor kernel: glim_amd_factor_set_trip_stats."""
        a, b = C.c_uint64(), C.c_uint64()
        check(lib().glim_amd_factor_set_trip_stats(self._h, C.byref(a), C.byref(b), int(bool(reset))), "glim_amd_factor_set_trip_stats")
        return a.value, b.value

    def profile_sync(self, T_target_source, iters=200):
        """milliseconds per synchronous linearize() call measured inside the library (no binding overhead)."""
        T = np.ascontiguousarray(np.asarray(T_target_source, dtype=np.float64).reshape(len(self.factors), 12))
        a = C.c_float()
        check(lib().glim_amd_factor_set_profile_sync(self._h, _dp(T), int(iters), C.byref(a)), "glim_amd_factor_set_profile_sync")
        return a.value

    def linearize_repeat(self, pose_sets, iters):
        """EXACTLY `iters` synchronous linearize() calls issued from C (no binding overhead, no warm-up, no clock: the caller times it), call i at
        pose_sets[i % len(pose_sets)]; returns the last call's records (glim_amd_factor_set_linearize_repeat)."""
        nf = len(self.factors)
        T = np.ascontiguousarray(np.asarray(pose_sets, dtype=np.float64).reshape(-1, nf, 12))
        out = (Linearized6 * nf)()
        check(lib().glim_amd_factor_set_linearize_repeat(self._h, _dp(T), T.shape[0], int(iters), out), "glim_amd_factor_set_linearize_repeat")
        return [_lin_to_dict(L) for L in out]

    def profile_lm(self, T_target_source, iters=20):
        """(ms per synchronous linearize(), ms per synchronous error()) of the whole set, timed inside the library."""
        T = np.ascontiguousarray(np.asarray(T_target_source, dtype=np.float64).reshape(len(self.factors), 12))
        a, b = C.c_float(), C.c_float()
        check(lib().glim_amd_factor_set_profile_lm(self._h, _dp(T), int(iters), C.byref(a), C.byref(b)), "glim_amd_factor_set_profile_lm")
        return a.value, b.value

    def close(self):
        if self._h:
            lib().glim_amd_factor_set_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiDeviceCost:
    """Single-process, multi-device evaluation of a multi-scan VGICP cost (glim_amd_multi_*, include/glim_amd.h): clouds and voxel maps
    replicated on every device, the factor list sharded, one RCCL all-gather of the compact records per evaluation."""

    def __init__(self, devices=(0,), virtual=False):
        """virtual=True (tests / one-GPU boxes only, glim_amd_diag.h): a device ordinal may be listed several times -- every entry is a "virtual
        device" with its own context, host thread, shard and gathered array; the exchange is a same-device stand-in for ncclAllGather."""
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        h = C.c_void_p()
        if virtual:
            check(lib().glim_amd_debug_multi_create_virtual(_ip(dev), len(dev), C.byref(h)), "glim_amd_debug_multi_create_virtual")
        else:
            check(lib().glim_amd_multi_create(_ip(dev), len(dev), C.byref(h)), "glim_amd_multi_create")
        self._h = h
        self.factors = []

    def set_gather_mode(self, mode):
        """1 (default): the all-gather completes behind the call; 2: the call waits for it; 0: no exchange (glim_amd_multi_set_gather_mode)."""
        check(lib().glim_amd_multi_set_gather_mode(self._h, int(mode)), "glim_amd_multi_set_gather_mode")

    def wait_gather(self):
        check(lib().glim_amd_multi_wait_gather(self._h), "glim_amd_multi_wait_gather")

    def gathered_device(self, device=0):
        """(device pointer, rows) of the complete device-resident record array of one device (glim_amd_multi_gathered_device)."""
        ptr, rows = C.c_void_p(), C.c_int64()
        check(lib().glim_amd_multi_gathered_device(self._h, int(device), C.byref(ptr), C.byref(rows)), "glim_amd_multi_gathered_device")
        return ptr.value, rows.value

    def gathered_records(self, device=0, first=0, count=None):
        """What a device-side consumer on `device` reads after the exchange, copied back in factor order (glim_amd_debug_multi_gathered_download)."""
        count = self._n - first if count is None else count
        out = np.zeros((count, 29), dtype=np.float64)
        check(lib().glim_amd_debug_multi_gathered_download(self._h, int(device), int(first), int(count), _dp(out)), "glim_amd_debug_multi_gathered_download")
        return out

    def inject_failure(self, device, where):
        """One shot: the next evaluation fails on `device` before the barrier (where=1) / inside its exchange (where=2)."""
        check(lib().glim_amd_debug_multi_inject_failure(self._h, int(device), int(where)), "glim_amd_debug_multi_inject_failure")

    def set_diag(self, key_values):
        check(lib().glim_amd_debug_multi_set_diag(self._h, key_values.encode()), "glim_amd_debug_multi_set_diag")

    def info(self):
        nd, rc, nf = C.c_int32(), C.c_int32(), C.c_int64()
        check(lib().glim_amd_multi_info(self._h, C.byref(nd), C.byref(rc), C.byref(nf)), "glim_amd_multi_info")
        return {"num_devices": nd.value, "uses_rccl": bool(rc.value), "num_factors": nf.value}

    def add_cloud(self, points, covs=None, normals=None):
        points = np.asarray(points)
        n = points.shape[0]
        cid = C.c_int32()
        xyz = np.ascontiguousarray(points[:, :3], dtype=np.float32)
        c = None if covs is None else np.ascontiguousarray(np.asarray(covs, dtype=np.float32)[:, :3, :3]).reshape(n, 9)
        nr = None if normals is None else np.ascontiguousarray(np.asarray(normals, dtype=np.float32)[:, :3])
        check(lib().glim_amd_multi_add_cloud_f32(self._h, n, _fp(xyz), _fp(c), _fp(nr), C.byref(cid)), "glim_amd_multi_add_cloud_f32")
        return cid.value

    def estimate_covariances(self, cloud_id, k=10):
        check(lib().glim_amd_multi_cloud_estimate_covariances(self._h, int(cloud_id), int(k)), "glim_amd_multi_cloud_estimate_covariances")

    def add_voxelmap(self, cloud_id, resolution):
        mid = C.c_int32()
        check(lib().glim_amd_multi_add_voxelmap(self._h, int(cloud_id), float(resolution), C.byref(mid)), "glim_amd_multi_add_voxelmap")
        return mid.value

    def set_factors(self, target_map_ids, source_cloud_ids, flags=None):
        t = np.ascontiguousarray(target_map_ids, dtype=np.int32)
        s = np.ascontiguousarray(source_cloud_ids, dtype=np.int32)
        f = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint32)
        check(lib().glim_amd_multi_set_factors(self._h, len(t), _ip(t), _ip(s), None if f is None else f.ctypes.data_as(C.POINTER(C.c_uint32))),
              "glim_amd_multi_set_factors")
        self._n = len(t)

    def shard(self):
        b = np.zeros(self.info()["num_devices"] + 1, dtype=np.int64)
        check(lib().glim_amd_multi_shard(self._h, b.ctypes.data_as(C.POINTER(C.c_int64))), "glim_amd_multi_shard")
        return b

    def linearize(self, T_target_source):
        T = np.ascontiguousarray(np.asarray(T_target_source, dtype=np.float64).reshape(self._n, 12))
        out = (Linearized6 * self._n)()
        tot = C.c_double()
        check(lib().glim_amd_multi_linearize(self._h, _dp(T), out, C.byref(tot)), "glim_amd_multi_linearize")
        return [_lin_to_dict(L) for L in out], tot.value

    def profile(self, T_target_source, iters=10):
        T = np.ascontiguousarray(np.asarray(T_target_source, dtype=np.float64).reshape(self._n, 12))
        ms = C.c_float()
        check(lib().glim_amd_multi_profile(self._h, _dp(T), int(iters), C.byref(ms)), "glim_amd_multi_profile")
        return ms.value

    def last_timing(self):
        """Per device: HIP-event ms of the last evaluation's kernels and of its collective + copy-out."""
        nd = self.info()["num_devices"]
        k, g = np.zeros(nd, dtype=np.float32), np.zeros(nd, dtype=np.float32)
        check(lib().glim_amd_multi_last_timing(self._h, k.ctypes.data_as(C.POINTER(C.c_float)), g.ctypes.data_as(C.POINTER(C.c_float))), "glim_amd_multi_last_timing")
        return k.tolist(), g.tolist()

    BREAKDOWN_FIELDS = ("post", "wake", "pose_stage", "enqueue", "barrier", "collective", "wait", "join", "scan", "total", "library_calls",
                        "device_gather", "device_copy_out")

    def last_breakdown(self, device=0):
        """Host-side account of the last evaluation on one device's thread, microseconds (glim_amd_multi_last_breakdown)."""
        us = np.zeros(len(self.BREAKDOWN_FIELDS), dtype=np.float64)
        check(lib().glim_amd_multi_last_breakdown(self._h, int(device), _dp(us), len(us)), "glim_amd_multi_last_breakdown")
        return dict(zip(self.BREAKDOWN_FIELDS, us.tolist()))

    def set_split(self, mode):
        """-1: pieces of >= 2048 factors, at most 4 (default); 0 / 1: one piece; n: n pieces.  Applies to the next set_factors."""
        check(lib().glim_amd_multi_set_split(self._h, int(mode)), "glim_amd_multi_set_split")

    def set_host_records(self, mode):
        """1 (default): the finalising kernels store every record into the host array as well; 0: device-to-host copies behind each piece.
        Applies to the next set_factors."""
        check(lib().glim_amd_multi_set_host_records(self._h, int(mode)), "glim_amd_multi_set_host_records")

    def set_one_rank_collective(self, on):
        """One device: make the (no-op) ncclAllGather in every evaluation as well (measurement aid; default off)."""
        check(lib().glim_amd_multi_set_one_rank_collective(self._h, int(bool(on))), "glim_amd_multi_set_one_rank_collective")

    def evaluate(self, T_target_source):
        """One evaluation that leaves the records in the handle (records()) and returns the total error, summed by the devices."""
        T = np.ascontiguousarray(np.asarray(T_target_source, dtype=np.float64).reshape(self._n, 12))
        tot = C.c_double()
        check(lib().glim_amd_multi_linearize(self._h, _dp(T), None, C.byref(tot)), "glim_amd_multi_linearize")
        return tot.value

    def records(self, first=0, count=None):
        """Compact 29-double records of the last evaluation, factor order (glim_amd_multi_records)."""
        count = self._n - first if count is None else count
        out = np.zeros((count, 29), dtype=np.float64)
        check(lib().glim_amd_multi_records(self._h, int(first), int(count), _dp(out)), "glim_amd_multi_records")
        return out

    def close(self):
        if self._h:
            lib().glim_amd_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def resident_stats(ctx=None):
    """Debug: the device's resident session (glim_amd_debug_resident_stats): kernel launches, requests served, alive right now."""
    ctx = ctx or default_context()
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_int32()
    check(lib().glim_amd_debug_resident_stats(int(getattr(ctx, "device", 0)), C.byref(a), C.byref(b), C.byref(c)), "glim_amd_debug_resident_stats")
    return {"launches": a.value, "requests": b.value, "alive": bool(c.value)}


def resident_post_stats(ctx=None):
    """Debug: requests of the device's resident session by the way they were posted (glim_amd_debug_resident_post_stats, switch resident_post)."""
    ctx = ctx or default_context()
    a, b = C.c_uint64(), C.c_uint64()
    check(lib().glim_amd_debug_resident_post_stats(int(getattr(ctx, "device", 0)), C.byref(a), C.byref(b)), "glim_amd_debug_resident_post_stats")
    return {"direct": a.value, "lines": b.value}


def plan_stats(ctx=None):
    """Debug: factor plans built for new lists, how many of them in the buffers of an evicted plan, idle plans cached (glim_amd_debug_plan_stats)."""
    ctx = ctx or default_context()
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_int32()
    check(lib().glim_amd_debug_plan_stats(ctx._h, C.byref(a), C.byref(b), C.byref(c)), "glim_amd_debug_plan_stats")
    return {"built": a.value, "recycled": b.value, "cached": c.value}


def scratch_poke(ctx, word, value=0xFFFFFFFF):
    """Test hook (glim_amd_debug_scratch_poke): leave `value` in a word of the context's pinned scratch; the default stands for the sequence
    number the context's next polled voxel-map build waits for."""
    check(lib().glim_amd_debug_scratch_poke(ctx._h, int(word), int(value)), "glim_amd_debug_scratch_poke")


RESIDENT_TIMELINE_FIELDS = ("host_round_trip", "leader_published", "worker_pose_seen_min", "worker_pose_seen_median", "worker_pose_seen_max",
                            "worker_row_computed_min", "worker_row_computed_median", "worker_row_computed_max", "worker_row_published_min",
                            "worker_row_published_median", "worker_row_published_max", "finaliser_pose_seen", "finaliser_rows_summed",
                            "finaliser_record_stored", "workers_accounted", "device_span", "worker_loop_left_min", "worker_loop_left_median",
                            "worker_loop_left_max", "finaliser_group_sums_added", "finaliser_blocks_rotated", "shader_clock_mhz")


RESIDENT_TIMELINE_MAX_BLOCKS = 2048  # GLIM_AMD_RESIDENT_TIMELINE_MAX_BLOCKS
RESIDENT_TIMELINE_BLOCK_FIELDS = ("pose_seen", "row_computed", "row_published", "loop_left", "hw")  # GLIM_AMD_RESIDENT_TIMELINE_BLOCK_FIELDS each


def resident_timeline(device=0, enable=True, read=True, per_block=False):
    """glim_amd_debug_resident_timeline: ends the device's resident session; read=True returns the last request's timeline (microseconds relative to
    the leader seeing the request; None when no stamped session has run); the stamps stay on / off for the next sessions per `enable`.
    per_block=True adds the key "blocks": arrays with one entry per block of the launch, the workers first -- the four worker stamps (microseconds, -1
    where a block has none: a finalising block), `worker` (bool), and where the block runs: `hw_id`, `xcc_id` (the registers as read) and `cu`, one
    integer per compute unit (XCC_ID and the compute-unit, shader-array and shader-engine bits of HW_ID): equal `cu` = same compute unit."""
    nsum = len(RESIDENT_TIMELINE_FIELDS)
    nblk = len(RESIDENT_TIMELINE_BLOCK_FIELDS)
    us = np.zeros(nsum + (2 + nblk * RESIDENT_TIMELINE_MAX_BLOCKS if per_block else 0), dtype=np.float64)
    rc = lib().glim_amd_debug_resident_timeline(int(device), int(bool(enable)), _dp(us) if read else None, len(us) if read else 0)
    if rc == -5 and read:
        return None
    check(rc, "glim_amd_debug_resident_timeline")
    if not read:
        return None
    out = dict(zip(RESIDENT_TIMELINE_FIELDS, us[:nsum].tolist()))
    if per_block:
        blocks, workers = int(us[nsum]), int(us[nsum + 1])
        tab = us[nsum + 2 : nsum + 2 + nblk * blocks].reshape(blocks, nblk)
        hw = tab[:, 4].astype(np.uint64)
        hw_id, xcc_id = (hw & np.uint64(0xFFFFFFFF)).astype(np.int64), (hw >> np.uint64(32)).astype(np.int64)
        out["blocks"] = {name: tab[:, k].copy() for k, name in enumerate(RESIDENT_TIMELINE_BLOCK_FIELDS[:4])}
        out["blocks"].update(worker=np.arange(blocks) < workers, hw_id=hw_id, xcc_id=xcc_id, cu=((xcc_id & 0xF) << 8) | ((hw_id >> 8) & 0xFF))
    return out


def resident_stop(ctx=None):
    """Debug: end the device's resident session now (it would idle out by itself after `resident_idle_us`)."""
    ctx = ctx or default_context()
    check(lib().glim_amd_debug_resident_stop(int(getattr(ctx, "device", 0))), "glim_amd_debug_resident_stop")


def shard_bounds(costs, world):
    """glim_amd_shard_bounds: the C implementation of the sharding rule (host only; works without a device)."""
    c = np.ascontiguousarray(costs, dtype=np.float64)
    b = np.zeros(int(world) + 1, dtype=np.int64)
    check(lib().glim_amd_shard_bounds(_dp(c) if len(c) else None, len(c), int(world), b.ctypes.data_as(C.POINTER(C.c_int64))), "glim_amd_shard_bounds")
    return [int(x) for x in b]


def shard_layout(bounds, split_mode=-1):
    """glim_amd_shard_layout: (row of every factor in the gathered array, max_rows, pieces, piece_rows) -- host only, no device needed."""
    b = np.ascontiguousarray(bounds, dtype=np.int64)
    world = len(b) - 1
    rows = np.zeros(max(1, int(b[-1])), dtype=np.int64)
    mr, pc, pr = C.c_int64(), C.c_int32(), C.c_int64()
    lp = C.POINTER(C.c_int64)
    check(lib().glim_amd_shard_layout(b.ctypes.data_as(lp), world, int(split_mode), rows.ctypes.data_as(lp), C.byref(mr), C.byref(pc), C.byref(pr)), "glim_amd_shard_layout")
    return rows[: int(b[-1])], mr.value, pc.value, pr.value


def preprocess_params(**kw):
    """glim_amd_preprocess_params with the shipped defaults (config/config_preprocess.json), fields overridden by keyword."""
    p = PreprocessParams()
    check(lib().glim_amd_preprocess_default_params(C.byref(p)), "glim_amd_preprocess_default_params")
    for k, v in kw.items():
        if k in ("crop_bbox_min", "crop_bbox_max"):
            getattr(p, k)[:] = [float(x) for x in v]
        elif k == "T_imu_lidar":
            p.T_imu_lidar[:] = list(pose12(v))
        else:
            setattr(p, k, v)
    return p


class _GicpTarget:
    """What (target, target_tree) of a GICP-family factor resolve to: `ivox` (a borrowed IncrementalVoxelMap, or None), `tree` (what the factor
    shows as target_tree: the map, a borrowed search index, or an index created here) and `handle` (what the C calls take: the map's handle
    as it is at the call, None once the map is closed).  close() destroys the index only when it was created here."""

    def __init__(self, target, target_tree, max_correspondence_distance):
        self.ivox = next((t for t in (target_tree, target) if isinstance(t, IncrementalVoxelMap)), None)
        self.owned = target_tree is None and self.ivox is None
        if self.owned:
            target_tree = C.c_void_p()
            check(lib().glim_amd_nn_index_create(target._h, float(max_correspondence_distance), C.byref(target_tree)), "glim_amd_nn_index_create")
        self.tree = self.ivox if self.ivox is not None else target_tree

    @property
    def handle(self):
        return self.ivox._h if self.ivox is not None else self.tree

    def close(self):
        if self.owned and self.tree:
            lib().glim_amd_nn_index_destroy(self.tree)
            self.tree = None


class IntegratedGICPFactor:
    """gtsam_points::IntegratedGICPFactor on the device (sub_mapping.cpp:202, global_mapping.cpp:400, global_mapping_pose_graph.cpp:393).
    Unary form: IntegratedGICPFactor(fixed_target_pose, source_key, target, source); binary: (target_key, source_key, target, source).
    `target` / `source` are PointCloudGPU with covariances; the target's search index is built once here (or passed as `target_tree`).
    An IncrementalVoxelMap as `target_frame` (or `target_tree`) gives IntegratedGICPFactor_<iVox, PointCloud>: the map's own bounded search."""

    # the entry points of a target kind and the type of its correspondences (an index: original target index; a map: slot * max_points + place)
    _OVER_INDEX = ("glim_amd_gicp_linearize", "glim_amd_gicp_error", "glim_amd_gicp_correspondences", np.int32, C.c_int32)
    _OVER_IVOX = ("glim_amd_ivox_gicp_linearize", "glim_amd_ivox_gicp_error", "glim_amd_ivox_gicp_correspondences", np.int64, C.c_int64)

    def __init__(self, target, source_key, target_frame, source_frame, target_tree=None, max_correspondence_distance=1.0):
        self.binary = np.isscalar(target)
        self.target_key = int(target) if self.binary else None
        self.fixed_target_pose = None if self.binary else np.asarray(target, dtype=np.float64)
        self.source_key = int(source_key)
        self.target_frame, self.source_frame = target_frame, source_frame
        self.max_correspondence_distance = float(max_correspondence_distance)
        self._inliers = 0
        self._target = _GicpTarget(target_frame, target_tree, self.max_correspondence_distance)
        self.target_tree = self._target.tree
        kind = self._OVER_IVOX if self._target.ivox is not None else self._OVER_INDEX
        self._linearize, self._error, self._correspondences, self._corr_dtype, self._corr_ctype = kind

    def set_max_correspondence_distance(self, d):
        self.max_correspondence_distance = float(d)

    def calc_delta(self, values):
        Ts = np.asarray(values[self.source_key], dtype=np.float64)
        Tt = np.asarray(values[self.target_key], dtype=np.float64) if self.binary else self.fixed_target_pose
        return np.linalg.inv(Tt) @ Ts

    def linearize(self, values):
        L = Linearized6()
        T = pose12(self.calc_delta(values))
        self._call(self._linearize, T, FACTOR_BINARY if self.binary else 0, C.byref(L))
        out = _lin_to_dict(L)
        self._inliers = out["num_inliers"]
        return out

    def error(self, values):
        e, n = C.c_double(), C.c_int64()
        T = pose12(self.calc_delta(values))
        self._call(self._error, T, C.byref(e), C.byref(n))
        self._inliers = n.value
        return e.value

    def inlier_fraction(self):
        return self._inliers / max(1, self.source_frame.size())

    def correspondences(self, values):
        T = pose12(self.calc_delta(values))
        out = np.zeros(self.source_frame.size(), dtype=self._corr_dtype)
        self._call(self._correspondences, T, out.ctypes.data_as(C.POINTER(self._corr_ctype)))
        return out

    def _call(self, name, T, *out):
        check(getattr(lib(), name)(self._target.handle, self.source_frame._h, _dp(T), self.max_correspondence_distance, *out), name)

    def align(self, T_init, params=None):
        """The fine registration of this factor's pair from T_init (4 x 4 T_target_source): gicp_align_batch with one problem."""
        r = gicp_align_batch([self._target], [self.source_frame], [T_init], self.max_correspondence_distance, params)[0]
        self._inliers = r.num_inliers
        return r

    def close(self):
        self._target.close()
        self.target_tree = self._target.tree

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


ICP_POINT_TO_PLANE = 0x4  # GLIM_AMD_ICP_POINT_TO_PLANE


class IntegratedICPFactor(IntegratedGICPFactor):
    """gtsam_points::IntegratedICPFactor on the device (manual_loop_close_modal.cpp:485-490: the fine registration of clouds without
    covariances).  The constructor forms, the methods and the correspondences are IntegratedGICPFactor's -- the same search index, so
    `target_tree` may be shared with GICP factors -- over a PointCloudGPU target; neither cloud needs covariances.  use_point_to_plane:
    IntegratedPointToPlaneICPFactor, which needs the target's normals."""

    def __init__(self, target, source_key, target_frame, source_frame, max_correspondence_distance=1.0, use_point_to_plane=False, target_tree=None):
        if any(isinstance(t, IncrementalVoxelMap) for t in (target_frame, target_tree)):
            raise GlimAmdError(-1, "IntegratedICPFactor", "the ICP factors take a point-cloud target (a search index), not an iVox")
        super().__init__(target, source_key, target_frame, source_frame, target_tree=target_tree, max_correspondence_distance=max_correspondence_distance)
        self.use_point_to_plane = bool(use_point_to_plane)
        self._linearize, self._error = "glim_amd_icp_linearize", "glim_amd_icp_error"

    def flags(self):
        return (FACTOR_BINARY if self.binary else 0) | (ICP_POINT_TO_PLANE if self.use_point_to_plane else 0)

    def linearize(self, values):
        L = Linearized6()
        self._call(self._linearize, pose12(self.calc_delta(values)), self.flags(), C.byref(L))
        out = _lin_to_dict(L)
        self._inliers = out["num_inliers"]
        return out

    def error(self, values):
        e, n = C.c_double(), C.c_int64()
        self._call(self._error, pose12(self.calc_delta(values)), self.flags(), C.byref(e), C.byref(n))
        self._inliers = n.value
        return e.value

    def align(self, T_init, params=None):
        """The fine registration of this factor's pair from T_init (4 x 4 T_target_source): icp_align_batch with one problem."""
        r = icp_align_batch([self._target], [self.source_frame], [T_init], self.max_correspondence_distance,
                            ICP_POINT_TO_PLANE if self.use_point_to_plane else 0, params)[0]
        self._inliers = r.num_inliers
        return r


class IntegratedPointToPlaneICPFactor(IntegratedICPFactor):
    """gtsam_points::IntegratedPointToPlaneICPFactor: IntegratedICPFactor with use_point_to_plane."""

    def __init__(self, target, source_key, target_frame, source_frame, max_correspondence_distance=1.0, target_tree=None):
        super().__init__(target, source_key, target_frame, source_frame, max_correspondence_distance, True, target_tree)


class LMParams:
    """glim_amd_lm_params (include/glim_amd.h "GICP fine registration"): GTSAM's LevenbergMarquardtParams fields the fine registration reads.
    max_trials = 0: twice max_iterations."""

    def __init__(self, lambda_initial=1e-5, lambda_factor=10.0, lambda_upper_bound=1e5, lambda_lower_bound=0.0, relative_error_tol=1e-5,
                 absolute_error_tol=1e-5, max_iterations=10, max_trials=0, error_scale=1.0):
        self.lambda_initial = lambda_initial
        self.lambda_factor = lambda_factor
        self.lambda_upper_bound = lambda_upper_bound
        self.lambda_lower_bound = lambda_lower_bound
        self.relative_error_tol = relative_error_tol
        self.absolute_error_tol = absolute_error_tol
        self.max_iterations = max_iterations
        self.max_trials = max_trials
        self.error_scale = error_scale

    def resolved_max_trials(self):
        return int(self.max_trials) if self.max_trials else 2 * int(self.max_iterations)

    def _c(self):
        return _lib.LMParams(float(self.lambda_initial), float(self.lambda_factor), float(self.lambda_upper_bound), float(self.lambda_lower_bound),
                             float(self.relative_error_tol), float(self.absolute_error_tol), int(self.max_iterations), int(self.max_trials),
                             float(self.error_scale))


ALIGN_STATUS = {1: "CONVERGED", 2: "MAX_ITERATIONS", 3: "MAX_TRIALS", 4: "LAMBDA_BOUND", 5: "NO_CORRESPONDENCES", 6: "NUMERIC"}


class AlignResult:
    """glim_amd_align_result: the last kept pose (4 x 4), the factor's error and inliers there, the counts, the status (ALIGN_STATUS), the
    lambda after the last trial and the compact record at the pose (expand_compact gives the linearisation at the estimate)."""

    def __init__(self, c, source_size):
        T = np.eye(4)
        T[:3] = np.array(c.T_target_source[:]).reshape(3, 4)
        self.T_target_source = T
        self.error = c.error
        self.num_inliers = c.num_inliers
        self.inlier_fraction = c.num_inliers / max(1, source_size)
        self.iterations = c.iterations
        self.trials = c.trials
        self.status = c.status
        self.status_name = ALIGN_STATUS.get(c.status, "?")
        self.lam = c.lam
        self.compact = np.array(c.compact[:])

    def linearized(self, flags=0):
        return expand_compact(self.compact, self.T_target_source, flags)


def _align_args(targets, sources, T_init, max_correspondence_distance):
    """-> (resolved _GicpTarget per problem, is_ivox, the C arrays)"""
    n = len(sources)
    if len(targets) != n:
        raise ValueError("one target per source")
    dist = np.ascontiguousarray(np.broadcast_to(np.asarray(max_correspondence_distance, dtype=np.float64), (n,)))
    T = np.zeros((n, 12))
    for i, Ti in enumerate(T_init):
        T[i] = pose12(Ti)
    if len(T_init) != n:
        raise ValueError("one initial pose per source")
    resolved, owned = [], {}
    for t, d in zip(targets, dist):
        if isinstance(t, PointCloudGPU):  # an index of its own, one per distinct cloud of the batch
            if id(t) not in owned:
                owned[id(t)] = _GicpTarget(t, None, float(d))
            resolved.append(owned[id(t)])
        elif isinstance(t, _GicpTarget):
            resolved.append(t)
        else:
            resolved.append(_GicpTarget(None, t, float(d)))
    kinds = {r.ivox is not None for r in resolved}
    if len(kinds) > 1:
        for r in owned.values():
            r.close()
        raise GlimAmdError(-1, "gicp_align_batch", "search-index and iVox targets in one batch")
    th = (C.c_void_p * max(n, 1))(*[r.handle for r in resolved])
    sh = (C.c_void_p * max(n, 1))(*[s._h for s in sources])
    return list(owned.values()), (kinds == {True}), th, sh, T, dist


def gicp_align_batch(targets, sources, T_init, max_correspondence_distance, params=None):
    """GICP fine registration of len(sources) independent problems in one call and one host synchronisation: Levenberg-Marquardt over one unary
    IntegratedGICPFactor each (global_mapping_pose_graph.cpp:386-426, global_mapping.cpp:393-426, manual_loop_close_modal.cpp:470-520).
    targets[i]: a PointCloudGPU (its index is built here), a search-index handle (IntegratedGICPFactor.target_tree) or an IncrementalVoxelMap --
    one kind per batch; sources[i]: PointCloudGPU with covariances; T_init[i]: 4 x 4 T_target_source; max_correspondence_distance: a number or one
    per problem.  Returns one AlignResult per problem."""
    n = len(sources)
    owned, ivox, th, sh, T, dist = _align_args(targets, sources, T_init, max_correspondence_distance)
    try:
        prm = (params or LMParams())._c()
        out = (_lib.AlignResult * max(n, 1))()
        name = "glim_amd_gicp_align_batch_incremental" if ivox else "glim_amd_gicp_align_batch"
        check(getattr(lib(), name)(th, sh, _dp(T), _dp(dist), n, C.byref(prm), out), name)
    finally:
        for r in owned:
            r.close()
    return [AlignResult(out[i], sources[i].size()) for i in range(n)]


def gicp_align_debug_trace(targets, sources, T_init, max_correspondence_distance, params=None):
    """Test window (glim_amd_debug_gicp_align_trace): gicp_align_batch's results plus, per problem, one dict per round run -- round 0 is the
    initial pose -- with the pose evaluated (`T`, 4 x 4), the `lam` its step was solved with, the `compact` record there, `accepted` and the
    `status` after the round (0: still running)."""
    n = len(sources)
    params = params or LMParams()
    owned, ivox, th, sh, T, dist = _align_args(targets, sources, T_init, max_correspondence_distance)
    rounds = 1 + params.resolved_max_trials()
    try:
        prm = params._c()
        out = (_lib.AlignResult * max(n, 1))()
        trace = (_lib.AlignTraceEntry * max(n * rounds, 1))()
        check(lib().glim_amd_debug_gicp_align_trace(1 if ivox else 0, th, sh, _dp(T), _dp(dist), n, C.byref(prm), out, trace),
              "glim_amd_debug_gicp_align_trace")
    finally:
        for r in owned:
            r.close()
    results = [AlignResult(out[i], sources[i].size()) for i in range(n)]
    return results, [_trace_rows(trace, i, rounds, r.trials) for i, r in enumerate(results)]


def icp_align_params(**kw):
    """LMParams with the ICP fine registration's value (glim_amd_icp_align_default_params): max_iterations 200 (manual_loop_close_modal.cpp:490)."""
    p = dict(max_iterations=200)
    p.update(kw)
    return LMParams(**p)


def _icp_align_args(targets, sources, T_init, max_correspondence_distance):
    owned, ivox, th, sh, T, dist = _align_args(targets, sources, T_init, max_correspondence_distance)
    if ivox:
        raise GlimAmdError(-1, "icp_align_batch", "the ICP factors take point-cloud targets (search indices), not iVoxes")
    return owned, th, sh, T, dist


def icp_align_batch(targets, sources, T_init, max_correspondence_distance, flags=0, params=None):
    """ICP fine registration of len(sources) independent problems in one call: Levenberg-Marquardt over one unary IntegratedICPFactor each
    (manual_loop_close_modal.cpp:485-490, LM <= 200; params None: icp_align_params()).  targets[i]: a PointCloudGPU (its index is built here)
    or a search-index handle; sources[i]: PointCloudGPU; no covariances needed; flags: 0 or ICP_POINT_TO_PLANE, for every problem.  At most
    41 rounds are enqueued between two looks at the statuses.  Returns one AlignResult per problem."""
    n = len(sources)
    owned, th, sh, T, dist = _icp_align_args(targets, sources, T_init, max_correspondence_distance)
    try:
        prm = (params or icp_align_params())._c()
        out = (_lib.AlignResult * max(n, 1))()
        check(lib().glim_amd_icp_align_batch(th, sh, _dp(T), _dp(dist), int(flags), n, C.byref(prm), out), "glim_amd_icp_align_batch")
    finally:
        for r in owned:
            r.close()
    return [AlignResult(out[i], sources[i].size()) for i in range(n)]


def icp_align_debug_trace(targets, sources, T_init, max_correspondence_distance, flags=0, params=None, rounds_per_chunk=0):
    """Test window (glim_amd_debug_icp_align_trace): icp_align_batch's results plus, per problem, the rounds run, as gicp_align_debug_trace.
    rounds_per_chunk: rounds enqueued between two looks at the statuses (0: the call's own 41; "all": every round up front)."""
    n = len(sources)
    params = params or icp_align_params()
    owned, th, sh, T, dist = _icp_align_args(targets, sources, T_init, max_correspondence_distance)
    rounds = 1 + params.resolved_max_trials()
    chunk = rounds if rounds_per_chunk == "all" else int(rounds_per_chunk)
    try:
        prm = params._c()
        out = (_lib.AlignResult * max(n, 1))()
        trace = (_lib.AlignTraceEntry * max(n * rounds, 1))()
        check(lib().glim_amd_debug_icp_align_trace(th, sh, _dp(T), _dp(dist), int(flags), n, C.byref(prm), out, trace, chunk), "glim_amd_debug_icp_align_trace")
    finally:
        for r in owned:
            r.close()
    results = [AlignResult(out[i], sources[i].size()) for i in range(n)]
    return results, [_trace_rows(trace, i, rounds, r.trials) for i, r in enumerate(results)]


def _vgicp_align_args(targets, sources, T_init):
    n = len(sources)
    if len(targets) != n:
        raise ValueError("one target per source")
    if len(T_init) != n:
        raise ValueError("one initial pose per source")
    T = np.zeros((n, 12))
    for i, Ti in enumerate(T_init):
        T[i] = pose12(Ti)
    th = (C.c_void_p * max(n, 1))(*[t._h for t in targets])
    sh = (C.c_void_p * max(n, 1))(*[s._h for s in sources])
    return n, th, sh, T


def vgicp_align_batch(targets, sources, T_init, flags=0, params=None):
    """VGICP fine registration of len(sources) independent problems in one call and one host synchronisation: Levenberg-Marquardt over one unary
    IntegratedVGICPFactor each (global_mapping_pose_graph.cpp:405-417 with registration_type "VGICP").  targets[i]: GaussianVoxelMapGPU;
    sources[i]: PointCloudGPU with covariances; T_init[i]: 4 x 4 T_target_source; flags: 0 or FACTOR_SURFACE_VALIDATION, for every problem.
    Every trial record is what a NonlinearFactorSetGPU of the same pairs returns at the trial's poses.  Returns one AlignResult per problem."""
    n, th, sh, T = _vgicp_align_args(targets, sources, T_init)
    prm = (params or LMParams())._c()
    out = (_lib.AlignResult * max(n, 1))()
    check(lib().glim_amd_vgicp_align_batch(th, sh, _dp(T), int(flags), n, C.byref(prm), out), "glim_amd_vgicp_align_batch")
    return [AlignResult(out[i], sources[i].size()) for i in range(n)]


def vgicp_align_debug_trace(targets, sources, T_init, flags=0, params=None):
    """Test window (glim_amd_debug_vgicp_align_trace): vgicp_align_batch's results plus, per problem, the rounds run, as gicp_align_debug_trace."""
    params = params or LMParams()
    n, th, sh, T = _vgicp_align_args(targets, sources, T_init)
    rounds = 1 + params.resolved_max_trials()
    prm = params._c()
    out = (_lib.AlignResult * max(n, 1))()
    trace = (_lib.AlignTraceEntry * max(n * rounds, 1))()
    check(lib().glim_amd_debug_vgicp_align_trace(th, sh, _dp(T), int(flags), n, C.byref(prm), out, trace), "glim_amd_debug_vgicp_align_trace")
    results = [AlignResult(out[i], sources[i].size()) for i in range(n)]
    return results, [_trace_rows(trace, i, rounds, r.trials) for i, r in enumerate(results)]


def _trace_rows(trace, i, rounds, trials):
    rows = []
    for k in range(min(rounds, trials + 1)):
        e = trace[i * rounds + k]
        Tk = np.eye(4)
        Tk[:3] = np.array(e.T_candidate[:]).reshape(3, 4)
        rows.append({"T": Tk, "lam": e.lam, "compact": np.array(e.compact[:]), "accepted": bool(e.accepted), "status": e.status})
    return rows


KEYFRAME_ALIGN_MAX_TARGETS = 64  # GLIM_AMD_KEYFRAME_ALIGN_MAX_TARGETS
KEYFRAME_PRIOR_DOUBLES = 28  # a prior's traced contribution: 21 of J^T L J, 6 of J^T L r, r^T L r


def _keyframe_args(problems):
    """problems: (source, [(voxel map, T_world_target 4 x 4), ...], X_init 4 x 4[, prior]); prior: None or (P 4 x 4, information 6 x 6) -> the C
    arrays"""
    n = len(problems)
    first = np.zeros(n + 1, dtype=np.int32)
    maps, P, priors = [], [], []
    X = np.zeros((n, 12))
    for i, pr in enumerate(problems):
        source, targets, X_init = pr[0], pr[1], pr[2]
        for m, T in targets:
            maps.append(m)
            P.append(pose12(T))
        first[i + 1] = len(maps)
        X[i] = pose12(X_init)
        if len(pr) > 3 and pr[3] is not None:
            priors.append((i, pr[3][0], pr[3][1]))
    F = len(maps)
    P = np.ascontiguousarray(np.asarray(P, dtype=np.float64).reshape(F, 12))
    sh = (C.c_void_p * max(n, 1))(*[pr[0]._h for pr in problems])
    th = (C.c_void_p * max(F, 1))(*[m._h for m in maps])
    cp = (_lib.BundlePrior * max(len(priors), 1))()
    for c, (k, T, info) in zip(cp, priors):
        c.pose = int(k)
        c.T[:] = list(pose12(T))
        c.information[:] = list(np.asarray(info, dtype=np.float64).reshape(36))
    return n, F, first, (sh, _ip(first), th, _dp(P), _dp(X), cp if priors else None, len(priors)), (P, X)


def _keyframe_results(problems, out, first, compact):
    results = []
    for i, pr in enumerate(problems):
        r = AlignResult(out[i], pr[0].size() * len(pr[1]))  # the inliers are summed over the factors: the fraction is of M x size
        r.factor_compact = compact[first[i]:first[i + 1]].copy()  # every factor's record at the returned pose
        results.append(r)
    return results


def vgicp_align_keyframes(problems, flags=0, params=None):
    """Scan-to-keyframes VGICP registration of len(problems) independent problems in one call and one host synchronisation: Levenberg-Marquardt
    over ONE pose on the sum of one unary IntegratedVGICPFactorGPU per (keyframe, voxel-map level) with fixed target poses
    (odometry_estimation_gpu.cpp:150-165, 183-203).  A problem is (source, [(GaussianVoxelMapGPU, T_world_target 4 x 4), ...], X_init 4 x 4
    [, prior]) with at most KEYFRAME_ALIGN_MAX_TARGETS targets; X is T_world_source; prior: None or (P 4 x 4, information 6 x 6).  flags: 0 or
    FACTOR_SURFACE_VALIDATION.  Factor f is evaluated at P_f^-1 X; every trial record is what a NonlinearFactorSetGPU of all the batch's pairs
    returns at those poses.  Returns one AlignResult per problem -- T_target_source is X, error / num_inliers / compact are the summed record
    there -- with `factor_compact` (M x 29) attached."""
    n, F, first, args, keep = _keyframe_args(problems)
    prm = (params or LMParams())._c()
    out = (_lib.AlignResult * max(n, 1))()
    compact = np.zeros((F, _lib.COMPACT_DOUBLES))
    check(lib().glim_amd_keyframe_align_batch(*args, int(flags), n, C.byref(prm), out, _dp(compact)), "glim_amd_keyframe_align_batch")
    return _keyframe_results(problems, out, first, compact)


def vgicp_align_keyframes_debug_trace(problems, flags=0, params=None):
    """Test window (glim_amd_debug_keyframe_align_trace): vgicp_align_keyframes' results plus, per problem, one dict per round run -- round 0 is
    the initial pose -- as gicp_align_debug_trace gives them (`T`: the X evaluated, `compact`: the SUMMED record) with, in addition, `prior`
    (the prior's 28-double contribution), `Tf` (M x 12, the factor poses as the device computed them) and `factor_compact` (M x 29, the
    factors' records there)."""
    params = params or LMParams()
    n, F, first, args, keep = _keyframe_args(problems)
    rounds = 1 + params.resolved_max_trials()
    prm = params._c()
    out = (_lib.AlignResult * max(n, 1))()
    compact = np.zeros((F, _lib.COMPACT_DOUBLES))
    trace = (_lib.AlignTraceEntry * max(n * rounds, 1))()
    tprior, tTf = np.zeros((max(n, 1), rounds, KEYFRAME_PRIOR_DOUBLES)), np.zeros((rounds, max(F, 1), 12))
    trec = np.zeros((rounds, max(F, 1), _lib.COMPACT_DOUBLES))
    check(lib().glim_amd_debug_keyframe_align_trace(*args, int(flags), n, C.byref(prm), out, _dp(compact), trace, _dp(tprior), _dp(tTf), _dp(trec)),
          "glim_amd_debug_keyframe_align_trace")
    results = _keyframe_results(problems, out, first, compact)
    traces = []
    for i, r in enumerate(results):
        rows = _trace_rows(trace, i, rounds, r.trials)
        for k, row in enumerate(rows):
            row["prior"] = tprior[i, k].copy()
            row["Tf"] = tTf[k, first[i]:first[i + 1]].copy()
            row["factor_compact"] = trec[k, first[i]:first[i + 1]].copy()
        traces.append(rows)
    return results, traces


def bundle_align_params(**kw):
    """LMParams with the sub-mapping bundle's value (glim_amd_bundle_align_default_params): max_iterations 20 (sub_mapping.cpp:431)."""
    p = dict(max_iterations=20)
    p.update(kw)
    return LMParams(**p)


class BundleResult:
    """glim_amd_bundle_align's answer: the last kept poses (N x 4 x 4), the cost there and its three parts, the factors' inliers, the counts,
    the status (ALIGN_STATUS), the lambda after the last trial and the F compact records at the poses.  between_weights: the Q Huber weights of
    the evaluation at the poses (glim_amd_*_align_terms), or None from a call without damping terms and Huber widths."""

    def __init__(self, c, X, compact, between_weights=None):
        self.poses = X
        self.between_weights = between_weights
        self.cost, self.factor_cost, self.prior_cost, self.between_cost = c.cost, c.factor_cost, c.prior_cost, c.between_cost
        self.num_inliers = c.num_inliers
        self.iterations, self.trials, self.status = c.iterations, c.trials, c.status
        self.status_name = ALIGN_STATUS.get(c.status, "?")
        self.lam = c.lam
        self.compact = compact


def _poses44(X12):
    X = np.tile(np.eye(4), (len(X12), 1, 1))
    X[:, :3, :] = np.asarray(X12).reshape(-1, 3, 4)
    return X


def _bundle_args(factors, priors, betweens, X_init, ctx):
    """factors: (voxel map, cloud, target pose index, source pose index); priors: (pose index, P 4 x 4, information 6 x 6); betweens: (i, j,
    D 4 x 4, information 6 x 6) -> the C arrays"""
    F, P, Q, N = len(factors), len(priors), len(betweens), len(X_init)
    if ctx is None:
        ctx = factors[0][0].ctx if F else default_context()
    th = (C.c_void_p * max(F, 1))(*[f[0]._h for f in factors])
    sh = (C.c_void_p * max(F, 1))(*[f[1]._h for f in factors])
    ti = np.ascontiguousarray([f[2] for f in factors], dtype=np.int32).reshape(F)
    si = np.ascontiguousarray([f[3] for f in factors], dtype=np.int32).reshape(F)
    cp = (_lib.BundlePrior * max(P, 1))()
    for c, (k, T, info) in zip(cp, priors):
        c.pose = int(k)
        c.T[:] = list(pose12(T))
        c.information[:] = list(np.asarray(info, dtype=np.float64).reshape(36))
    cb = (_lib.BundleBetween * max(Q, 1))()
    for c, (i, j, T, info) in zip(cb, betweens):
        c.pose_i, c.pose_j = int(i), int(j)
        c.T[:] = list(pose12(T))
        c.information[:] = list(np.asarray(info, dtype=np.float64).reshape(36))
    X = np.zeros((N, 12))
    for k, Xk in enumerate(X_init):
        X[k] = pose12(Xk)
    return ctx, (ctx._h, th, sh, _ip(ti), _ip(si), F), (cp, P, cb, Q, _dp(X), N), (ti, si, X)


def _graph_terms(betweens, dampings):
    """The damping terms and the Huber widths (a between's fifth element) of a call -> (the betweens without widths, the arguments behind
    `result` of a glim_amd_*_align_terms entry, the weights' array, what must stay alive); all None but the betweens when the call has neither:
    the entry point without `_terms` is then called as it always was."""
    betweens, dampings = list(betweens), list(dampings)
    if not dampings and not any(len(b) > 4 for b in betweens):
        return betweens, None, None, None
    D, Q = len(dampings), len(betweens)
    cd = (_lib.GraphDamping * max(D, 1))()
    for c, (k, d) in zip(cd, dampings):
        c.pose = int(k)
        c.diagonal[:] = list(np.broadcast_to(np.asarray(d, dtype=np.float64).reshape(-1), (6,)))
    widths = np.array([float(b[4]) if len(b) > 4 else 0.0 for b in betweens], dtype=np.float64).reshape(Q)
    terms = _lib.GraphTerms(C.cast(cd, C.POINTER(_lib.GraphDamping)), D, 0, _dp(widths) if any(len(b) > 4 for b in betweens) else None)
    weights = np.zeros(Q)
    return [tuple(b[:4]) for b in betweens], (C.byref(terms), _dp(weights)), weights, (cd, widths, terms)


def _align_poses(entry, factors, priors, betweens, X_init, flags, params, ctx, dampings=()):
    """glim_amd_bundle_align or glim_amd_graph_align, or their `_terms` forms: the same arguments and results"""
    betweens, terms, weights, alive = _graph_terms(betweens, dampings)
    ctx, fa, ta, keep = _bundle_args(factors, priors, betweens, X_init, ctx)
    F, N = fa[-1], ta[-1]
    prm = (params or bundle_align_params())._c()
    X_out, compact, out = np.zeros((N, 12)), np.zeros((F, _lib.COMPACT_DOUBLES)), _lib.BundleResult()
    if terms:
        entry += "_terms"
    check(getattr(lib(), entry)(*fa, int(flags), *ta, C.byref(prm), _dp(X_out), _dp(compact), C.byref(out), *(terms or ())), entry)
    return BundleResult(out, _poses44(X_out), compact, weights)


def _align_poses_trace(entry, more, factors, priors, betweens, X_init, flags, params, ctx, one_thread, trace, dampings=()):
    """glim_amd_debug_bundle_align_trace or glim_amd_debug_graph_align_trace, or their `_terms` forms (`more`: the arguments behind the trace
    arrays)"""
    params = params or bundle_align_params()
    betweens, terms, weights, alive = _graph_terms(betweens, dampings)
    if terms:
        entry = entry.replace("_trace", "_terms_trace")
    ctx, fa, ta, keep = _bundle_args(factors, priors, betweens, X_init, ctx)
    F, N = fa[-1], ta[-1]
    rounds = 1 + params.resolved_max_trials()
    prm = params._c()
    X_out, compact, out = np.zeros((N, 12)), np.zeros((F, _lib.COMPACT_DOUBLES)), _lib.BundleResult()
    tX, tTf, trec = np.zeros((rounds, N, 12)), np.zeros((rounds, F, 12)), np.zeros((rounds, F, _lib.COMPACT_DOUBLES))
    tr = (_lib.BundleTraceRound * rounds)()
    targs = (_dp(tX), _dp(tTf), _dp(trec), tr) if trace else (None, None, None, None)
    check(getattr(lib(), entry)(*fa, int(flags), *ta, C.byref(prm), _dp(X_out), _dp(compact), C.byref(out), *(terms or ()), 1 if one_thread else 0, *targs,
                                *more), entry)
    res = BundleResult(out, _poses44(X_out), compact, weights)
    rows = []
    if trace and N:
        for k in range(min(rounds, res.trials + 1)):
            rows.append({"X": _poses44(tX[k]), "Tf": tTf[k].copy(), "compact": trec[k].copy(), "lam": tr[k].lam, "cost": tr[k].cost,
                         "accepted": bool(tr[k].accepted), "status": tr[k].status})
    return res, rows, (tX, tTf, trec, tr)


def bundle_align(factors, priors, betweens, X_init, flags=0, params=None, ctx=None, dampings=()):
    """The sub-map bundle optimisation in one call and one host synchronisation: Levenberg-Marquardt over len(X_init) poses on binary VGICP
    factors, prior and between terms (sub_mapping.cpp:183-216, 430-452).  factors: (GaussianVoxelMapGPU, PointCloudGPU, target pose index,
    source pose index), evaluated at X_t^-1 X_s; priors: (pose index, P 4 x 4, information 6 x 6); betweens: (i, j, D 4 x 4, information 6 x 6);
    flags: 0 or FACTOR_SURFACE_VALIDATION.  Every trial record is what a NonlinearFactorSetGPU of the same pairs returns at the trial's relative
    poses.  A between may carry a fifth element, its Huber width (0: Gaussian); dampings: (pose index, scale or 6 diagonal values), the
    LinearDampingFactor.  With either, glim_amd_bundle_align_terms is called and the result has between_weights.  Returns a BundleResult."""
    return _align_poses("glim_amd_bundle_align", factors, priors, betweens, X_init, flags, params, ctx, dampings)


def bundle_align_debug_trace(factors, priors, betweens, X_init, flags=0, params=None, ctx=None, one_thread=False, trace=True, dampings=()):
    """Test window (glim_amd_debug_bundle_align_trace): bundle_align's result plus one dict per round run -- round 0 is the initial poses -- with
    the candidate poses (`X`, N x 4 x 4), the relative poses as the device computed them (`Tf`, F x 12), the `compact` records there (F x 29), the
    `lam` the step was solved with, the `cost` the evaluation gave, `accepted` and the `status` after the round.  one_thread: the decide step is
    bundle_lm_step.hpp's step() in one device thread (the cross-check form).  trace=False: the result alone.  Returns (result, rows, the raw
    trace arrays of all 1 + max_trials rounds: X, Tf, compact, rounds)."""
    return _align_poses_trace("glim_amd_debug_bundle_align_trace", (), factors, priors, betweens, X_init, flags, params, ctx, one_thread, trace, dampings)


def graph_align_params(**kw):
    """LMParams with the global-graph optimisation's values (glim_amd_graph_align_default_params): the bundle's."""
    return bundle_align_params(**kw)


def graph_align(factors, priors, betweens, X_init, flags=0, params=None, ctx=None, dampings=()):
    """The global-graph optimisation (glim_amd_graph_align; global_mapping.cpp:430-484 and that file's between factors): bundle_align's
    arguments, rule and BundleResult at up to _lib.GRAPH_MAX_POSES poses and _lib.GRAPH_MAX_FACTORS factors.  The systems live in device
    memory and a round is a sequence of launches; within the bundle's caps the result is bundle_align's, bit for bit."""
    return _align_poses("glim_amd_graph_align", factors, priors, betweens, X_init, flags, params, ctx, dampings)


def graph_align_debug_trace(factors, priors, betweens, X_init, flags=0, params=None, ctx=None, one_thread=False, trace=True, rounds_per_chunk=0, dampings=()):
    """Test window (glim_amd_debug_graph_align_trace): bundle_align_debug_trace's returns for graph_align.  one_thread: every round is
    bundle_lm_step.hpp's step() in one device thread with its system in device memory (the cross-check form; seconds beyond a few dozen poses).
    rounds_per_chunk: rounds enqueued between two looks at the status (0: the default); it moves no bit."""
    return _align_poses_trace("glim_amd_debug_graph_align_trace", (int(rounds_per_chunk),), factors, priors, betweens, X_init, flags, params, ctx, one_thread, trace,
                              dampings)


NODE_POSE, NODE_BIAS, NODE_VELOCITY = _lib.NODE_POSE, _lib.NODE_BIAS, _lib.NODE_VELOCITY
IMU_TANGENT, IMU_MANIFOLD = _lib.IMU_TANGENT, _lib.IMU_MANIFOLD


class ImuTerm:
    """One gtsam::ImuFactor(X_i, V_i, X_j, V_j, B) of graph_align_nav (glim_amd_nav_imu_term): the five node indices, dt > 0, gravity (gtsam's
    n_gravity), bias_hat (acc, gyro), delta = (theta, dp, dv) the preintegrated measurement at bias_hat, H_bias (9 x 6) its derivative by
    (acc, gyro), information (9 x 9, (rot, pos, vel) order: the inverse of preintMeasCov) and the mode: IMU_TANGENT (gtsam's
    TangentPreintegration, the build default) or IMU_MANIFOLD."""

    def __init__(self, pose_i, velocity_i, pose_j, velocity_j, bias, dt, gravity, bias_hat, delta, H_bias, information, mode=IMU_TANGENT):
        self.nodes = (pose_i, velocity_i, pose_j, velocity_j, bias)  # (indices; keys in NonlinearFactorSetGPU.optimize_nav_graph)
        self.dt, self.mode = float(dt), int(mode)
        self.gravity = np.asarray(gravity, dtype=np.float64).reshape(3)
        self.bias_hat = np.asarray(bias_hat, dtype=np.float64).reshape(6)
        self.delta = np.asarray(delta, dtype=np.float64).reshape(9)
        self.H_bias = np.asarray(H_bias, dtype=np.float64).reshape(9, 6)
        self.information = np.asarray(information, dtype=np.float64).reshape(9, 9)

    def _fill(self, c):
        c.pose_i, c.velocity_i, c.pose_j, c.velocity_j, c.bias = [int(v) for v in self.nodes]
        c.mode, c.dt = self.mode, self.dt
        c.gravity[:], c.bias_hat[:], c.delta[:] = list(self.gravity), list(self.bias_hat), list(self.delta)
        c.H_bias[:], c.information[:] = list(self.H_bias.reshape(-1)), list(self.information.reshape(-1))


class NavGraphResult(BundleResult):
    """glim_amd_graph_align_nav's answer: BundleResult's fields (`poses` is None), `nodes` (per node a 4 x 4 pose, 6 bias values or 3 velocity
    values), `values12` (the raw N x 12 rows) and the three further parts of the cost."""

    def __init__(self, c, X12, kinds, compact, between_weights=None):
        BundleResult.__init__(self, c, None, compact, between_weights)
        self.values12 = X12
        self.nodes = [_poses44(x[None])[0] if k == NODE_POSE else x[:6].copy() if k == NODE_BIAS else x[:3].copy() for x, k in zip(X12, kinds)]
        self.vector_prior_cost, self.vector_between_cost, self.imu_cost = c.vector_prior_cost, c.vector_between_cost, c.imu_cost


def _padded(v, info, dim):
    """a vector term's value and information (3 or 6 wide) in the 6-wide form of the C structs"""
    value, L = np.zeros(6), np.zeros((6, 6))
    v, info = np.asarray(v, dtype=np.float64).reshape(-1), np.asarray(info, dtype=np.float64)
    d = len(v)
    if d not in (dim, 6) or info.shape not in ((d, d), (6, 6)):
        raise GlimAmdError(-1, "graph_align_nav", "a vector term's value and information must be %d or 6 wide" % dim)
    value[:d] = v
    L[:info.shape[0], :info.shape[0]] = info
    return list(value), list(L.reshape(-1))


def _nav_args(nodes_init, kinds, vector_priors, vector_betweens, imu_terms):
    """-> (the node rows N x 12, glim_amd_nav_terms, what must stay alive)"""
    kinds = np.ascontiguousarray(kinds, dtype=np.int32).reshape(len(nodes_init))
    X = np.zeros((len(nodes_init), 12))
    for k, (x, kind) in enumerate(zip(nodes_init, kinds)):
        x = np.asarray(x, dtype=np.float64)
        if kind == NODE_POSE:
            X[k] = pose12(x)
        else:
            X[k, :x.size] = x.reshape(-1)  # (a row that is too long or has entries where none belong is the entry point's to refuse)
    dim = lambda node: 3 if 0 <= node < len(kinds) and kinds[node] == NODE_VELOCITY else 6
    VP, VB, I = len(vector_priors), len(vector_betweens), len(imu_terms)
    cp, cb, ci = (_lib.NavVectorPrior * max(VP, 1))(), (_lib.NavVectorBetween * max(VB, 1))(), (_lib.NavImuTerm * max(I, 1))()
    for c, (k, v, info) in zip(cp, vector_priors):
        c.node = int(k)
        c.value[:], c.information[:] = _padded(v, info, dim(int(k)))
    for c, (i, j, d, info) in zip(cb, vector_betweens):
        c.node_i, c.node_j = int(i), int(j)
        c.measurement[:], c.information[:] = _padded(d, info, dim(int(i)))
    for c, term in zip(ci, imu_terms):
        term._fill(c)
    nav = _lib.NavTerms(_ip(kinds), C.cast(cp, C.POINTER(_lib.NavVectorPrior)), C.cast(cb, C.POINTER(_lib.NavVectorBetween)), C.cast(ci, C.POINTER(_lib.NavImuTerm)),
                        VP, VB, I, 0)
    return X, kinds, nav, (cp, cb, ci)


def _graph_align_nav(entry, tail, factors, priors, betweens, nodes_init, kinds, vector_priors, vector_betweens, imu_terms, dampings, flags, params, ctx, rounds=0):
    params = params or bundle_align_params()
    X, kinds, nav, alive = _nav_args(nodes_init, kinds, list(vector_priors), list(vector_betweens), list(imu_terms))
    betweens, terms, weights, alive2 = _graph_terms(betweens, dampings)
    ctx, fa, ta, keep = _bundle_args(factors, priors, betweens, [np.eye(4)] * len(X), ctx)
    F, N = fa[-1], ta[-1]
    prm = params._c()
    X_out, compact, out = np.zeros((N, 12)), np.zeros((F, _lib.COMPACT_DOUBLES)), _lib.NavResult()
    tX, tTf, trec = np.zeros((rounds, N, 12)), np.zeros((rounds, F, 12)), np.zeros((rounds, F, _lib.COMPACT_DOUBLES))
    tr = (_lib.BundleTraceRound * max(rounds, 1))()
    targs = (_dp(tX), _dp(tTf), _dp(trec), tr) if rounds else (None, None, None, None)
    more = tail(targs) if tail else ()
    check(getattr(lib(), entry)(*fa, int(flags), *ta[:4], _dp(X), N, C.byref(prm), _dp(X_out), _dp(compact), C.byref(out), *(terms or (None, None)), C.byref(nav),
                                *more), entry)
    res = NavGraphResult(out, X_out, kinds, compact, weights)
    rows = []
    for k in range(min(rounds, res.trials + 1) if N else 0):
        rows.append({"X": tX[k].copy(), "Tf": tTf[k].copy(), "compact": trec[k].copy(), "lam": tr[k].lam, "cost": tr[k].cost, "accepted": bool(tr[k].accepted),
                     "status": tr[k].status})
    return res, rows, (tX, tTf, trec, tr)


def graph_align_nav(factors, priors, betweens, nodes_init, kinds, vector_priors=(), vector_betweens=(), imu_terms=(), dampings=(), flags=0, params=None, ctx=None):
    """The global-graph optimisation over pose, velocity and bias nodes (glim_amd_graph_align_nav): the graphs GLIM builds with enable_imu = true
    (sub_mapping.cpp:218-243, global_mapping.cpp:168-216).  factors, priors, betweens, dampings, flags, params: graph_align's, with node
    indices; factors, priors and betweens must name POSE nodes, a damping may name any node.  nodes_init: per node a 4 x 4 pose, 6 bias values
    (acc, gyro) or 3 velocity values; kinds: NODE_POSE / NODE_BIAS / NODE_VELOCITY per node.  vector_priors: (node, value, information);
    vector_betweens: (i, j, measurement of x_j - x_i, information), 3 wide for velocities and 6 wide for biases; imu_terms: ImuTerm.  Returns a
    NavGraphResult."""
    return _graph_align_nav("glim_amd_graph_align_nav", None, factors, priors, betweens, nodes_init, kinds, vector_priors, vector_betweens, imu_terms, dampings, flags,
                            params, ctx)[0]


def graph_align_nav_debug_trace(factors, priors, betweens, nodes_init, kinds, vector_priors=(), vector_betweens=(), imu_terms=(), dampings=(), flags=0, params=None,
                                ctx=None, one_thread=False, trace=True, rounds_per_chunk=0):
    """Test window (glim_amd_debug_graph_align_nav_trace): graph_align_debug_trace's returns for graph_align_nav; a row's `X` is the N x 12 node
    values of the round's candidate.  one_thread: every round is bundle_lm_step.hpp's step() in one device thread."""
    params = params or bundle_align_params()
    tail = lambda targs: (1 if one_thread else 0, *targs, int(rounds_per_chunk))
    return _graph_align_nav("glim_amd_debug_graph_align_nav_trace", tail, factors, priors, betweens, nodes_init, kinds, vector_priors, vector_betweens, imu_terms,
                            dampings, flags, params, ctx, rounds=1 + params.resolved_max_trials() if trace else 0)


def graph_solve_debug(S, n, lam, ctx=None):
    """Test window (glim_amd_debug_graph_solve): the device's blocked solve of (H + lam I) delta = -b on a packed system S (the lower triangle of
    H by rows, then b).  Returns (ok, delta)."""
    ctx = ctx or default_context()
    S = np.ascontiguousarray(S, dtype=np.float64)
    assert S.size == n * (n + 1) // 2 + n
    delta, ok = np.full(n, np.nan), C.c_int32(-1)
    check(lib().glim_amd_debug_graph_solve(ctx._h, _dp(S), int(n), float(lam), _dp(delta), C.byref(ok)), "glim_amd_debug_graph_solve")
    return bool(ok.value), delta


SE3_DEBUG_OPS = {"exp": (0, 6, 12), "log": (1, 12, 6), "jr": (2, 6, 36), "jr_inv": (3, 6, 36), "ad": (4, 12, 36), "prior": (5, 24, 42), "between": (6, 36, 78),
                 "ct": (7, 25, 84)}  # name -> op, doubles in, doubles out (include/glim_amd_diag.h)


def se3_debug_eval(op, x, ctx=None):
    """Test window (glim_amd_debug_se3_eval): one routine of csrc/ct_se3.hpp on the device, one thread per row of x (cases x IN doubles).
    op: a name of SE3_DEBUG_OPS.  Returns cases x OUT doubles."""
    ctx = ctx or default_context()
    code, n_in, n_out = SE3_DEBUG_OPS[op]
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, n_in)
    out = np.full((len(x), n_out), np.nan)
    check(lib().glim_amd_debug_se3_eval(ctx._h, code, len(x), _dp(x), _dp(out)), "glim_amd_debug_se3_eval")
    return out


def ct_align_params(**kw):
    """LMParams with GLIM's continuous-time odometry values (glim_amd_ct_align_default_params): lambda_initial 1e-10, absolute_error_tol 1e-2,
    max_iterations 8 (odometry_estimation_ct.cpp:176-183)."""
    p = dict(lambda_initial=1e-10, absolute_error_tol=1e-2, max_iterations=8)
    p.update(kw)
    return LMParams(**p)


def _ct_record(c):
    """a glim_amd_ct_linearized as IntegratedCT_GICPFactor.linearize returns it"""
    a = np.frombuffer(c, dtype=np.float64, count=122).copy()
    return {"num_inliers": int(c.num_inliers), "error": float(a[1]), "H_00": a[2:38].reshape(6, 6), "H_01": a[38:74].reshape(6, 6),
            "H_11": a[74:110].reshape(6, 6), "b_0": a[110:116], "b_1": a[116:122]}


class CtAlignResult:
    """glim_amd_ct_align_result: the last kept pair X, Y (4 x 4), the factor's record at it (`linearized`, as IntegratedCT_GICPFactor.linearize
    returns it), the total cost and the two terms' costs, the counts, the status (ALIGN_STATUS) and the lambda after the last trial.  `raw` holds
    the bytes of the C structure."""

    def __init__(self, c):
        self.raw = bytes(c)
        self.X, self.Y = np.eye(4), np.eye(4)
        self.X[:3] = np.array(c.X[:]).reshape(3, 4)
        self.Y[:3] = np.array(c.Y[:]).reshape(3, 4)
        self.linearized = _ct_record(c.linearized)
        self.error = self.linearized["error"]
        self.num_inliers = self.linearized["num_inliers"]
        self.cost = c.cost
        self.location_cost = c.location_cost
        self.between_cost = c.between_cost
        self.iterations = c.iterations
        self.trials = c.trials
        self.status = c.status
        self.status_name = ALIGN_STATUS.get(c.status, "?")
        self.lam = c.lam


def _ct_align_args(factor, values, location_prior, between, params):
    X, Y = factor._xy(values)
    terms = _lib.CtAlignTerms()
    none = True
    for term, pose, prec in ((location_prior, "T_location", "location_precision"), (between, "T_between", "between_precision")):
        if term is not None:
            T, k = term
            getattr(terms, pose)[:] = list(pose12(T))
            setattr(terms, prec, float(k))
            none = False
    prm = (params or ct_align_params())
    return X, Y, (None if none else C.byref(terms)), prm


def ct_align_debug_trace(factor, values, location_prior=None, between=None, params=None):
    """Test window (glim_amd_debug_ct_align_trace): IntegratedCT_GICPFactor.align's result plus one dict per round run -- round 0 is the initial
    pair -- with the pair evaluated (`X`, `Y`, 4 x 4), the `lam` its step was solved with, the factor's `record` there (92 doubles), the total
    `cost`, `accepted` and the `status` after the round (0: still running)."""
    X, Y, terms, prm = _ct_align_args(factor, values, location_prior, between, params)
    rounds = 1 + prm.resolved_max_trials()
    out = _lib.CtAlignResult()
    trace = (_lib.CtAlignTraceEntry * rounds)()
    pc = prm._c()
    check(lib().glim_amd_debug_ct_align_trace(factor._h, _dp(X), _dp(Y), terms, C.byref(pc), C.byref(out), trace), "glim_amd_debug_ct_align_trace")
    r = CtAlignResult(out)
    rows = []
    for k in range(min(rounds, r.trials + 1)):
        e = trace[k]
        Xk, Yk = np.eye(4), np.eye(4)
        Xk[:3] = np.array(e.X[:]).reshape(3, 4)
        Yk[:3] = np.array(e.Y[:]).reshape(3, 4)
        rows.append({"X": Xk, "Y": Yk, "lam": e.lam, "record": np.array(e.record[:]), "cost": e.cost, "accepted": bool(e.accepted), "status": e.status})
    return r, rows


class IntegratedCT_GICPFactor:
    """gtsam_points::IntegratedCT_GICPFactor (point-cloud target, KdTree) on the device: GLIM's continuous-time odometry cost
    (odometry_estimation_ct.cpp:158-183).  One scan between key0 (X, the pose at scan begin) and key1 (Y, at scan end); every point moves
    with the pose of its time bucket, T_k = X Exp(t_k Log(X^-1 Y)).  `target` / `source`: PointCloudGPU with covariances; the source also
    needs per-point times (`times`, or the ones its preprocessing kept).  linearize() returns the HessianFactor ingredients
    {num_inliers, error, H_00, H_01, H_11, b_0, b_1}; error() reuses the correspondences and M of the last linearize().
    An IncrementalVoxelMap as `target` (or `target_tree`) gives the frame-to-model form of :158-162: the factor reads the map as it is at
    each call, correspondences() returns slot * max_points + place, and the map cannot be closed before the factor."""

    def __init__(self, key0, key1, target, source, target_tree=None, max_correspondence_distance=1.0, times=None):
        self.keys = (int(key0), int(key1))
        self.target, self.source = target, source
        self._h = None
        self._target = _GicpTarget(target, target_tree, max_correspondence_distance)
        self.target_tree = self._target.tree
        t = None if times is None else np.ascontiguousarray(times, dtype=np.float64).reshape(source.size())
        h = C.c_void_p()
        create = "glim_amd_ivox_ct_factor_create" if self._target.ivox is not None else "glim_amd_ct_gicp_create"
        check(getattr(lib(), create)(self._target.handle, source._h, _dp(t), C.byref(h)), create)
        self._h = h
        self.set_max_correspondence_distance(max_correspondence_distance)

    def set_max_correspondence_distance(self, d):
        check(lib().glim_amd_ct_gicp_set_max_correspondence_distance(self._h, float(d)), "glim_amd_ct_gicp_set_max_correspondence_distance")
        self.max_correspondence_distance = float(d)

    def set_num_threads(self, n):
        """no-op: the device decides its own parallelism (kept for call-site compatibility)."""

    def _xy(self, values):
        return pose12(values[self.keys[0]]), pose12(values[self.keys[1]])

    def linearize(self, values):
        X, Y = self._xy(values)
        L = CtLinearized()
        check(lib().glim_amd_ct_gicp_linearize(self._h, _dp(X), _dp(Y), C.byref(L)), "glim_amd_ct_gicp_linearize")
        return _ct_record(L)

    def error(self, values, with_inliers=False):
        X, Y = self._xy(values)
        e, n = C.c_double(), C.c_int64()
        check(lib().glim_amd_ct_gicp_error(self._h, _dp(X), _dp(Y), C.byref(e), C.byref(n)), "glim_amd_ct_gicp_error")
        return (e.value, n.value) if with_inliers else e.value

    def align(self, values, location_prior=None, between=None, params=None):
        """The whole frame optimisation of odometry_estimation_ct.cpp:158-195 on the device, one host synchronisation (glim_amd_ct_align):
        Levenberg-Marquardt over values[key0], values[key1] on this factor plus the optional terms location_prior = (T, precision) on X and
        between = (T, precision) on X^-1 Y.  params: LMParams, default ct_align_params().  Returns a CtAlignResult; the state error() reuses
        is left as it was."""
        X, Y, terms, prm = _ct_align_args(self, values, location_prior, between, params)
        out = _lib.CtAlignResult()
        pc = prm._c()
        check(lib().glim_amd_ct_align(self._h, _dp(X), _dp(Y), terms, C.byref(pc), C.byref(out)), "glim_amd_ct_align")
        return CtAlignResult(out)

    def debug_align_poses(self, values):
        """(T_k n x 4 x 4, D0_k, D1_k n x 6 x 6) as the pose table kernel of align() computes them at `values`."""
        X, Y = self._xy(values)
        nb = C.c_int32()
        check(lib().glim_amd_debug_ct_align_poses(self._h, _dp(X), _dp(Y), C.byref(nb), 0, None, None, None), "glim_amd_debug_ct_align_poses")
        m = nb.value
        T, D0, D1 = np.zeros((m, 12)), np.zeros((m, 36)), np.zeros((m, 36))
        check(lib().glim_amd_debug_ct_align_poses(self._h, _dp(X), _dp(Y), C.byref(nb), m, _dp(T), _dp(D0), _dp(D1)), "glim_amd_debug_ct_align_poses")
        T44 = np.tile(np.eye(4), (m, 1, 1))
        T44[:, :3, :] = T.reshape(m, 3, 4)
        return T44, D0.reshape(m, 6, 6), D1.reshape(m, 6, 6)

    def correspondences(self, values):
        X, Y = self._xy(values)
        out = np.zeros(self.source.size(), dtype=np.int32)
        check(lib().glim_amd_ct_gicp_correspondences(self._h, _dp(X), _dp(Y), _ip(out)), "glim_amd_ct_gicp_correspondences")
        return out

    def deskewed_source_points(self, values, local=False):
        """T_k p_i per point (N x 3, FP64); local: in the frame of the first bucket's pose (odometry_estimation_ct.cpp:191)."""
        X, Y = self._xy(values)
        p4 = np.zeros((self.source.size(), 4))
        check(lib().glim_amd_ct_gicp_deskewed_points(self._h, _dp(X), _dp(Y), int(bool(local)), _dp(p4)), "glim_amd_ct_gicp_deskewed_points")
        return p4[:, :3].copy()

    def deskewed_cloud(self, values, local=False):
        """The deskewed points as a new PointCloudGPU carrying the source's neighbour lists (estimate_covariances runs on it, :194-195)."""
        X, Y = self._xy(values)
        h = C.c_void_p()
        check(lib().glim_amd_ct_gicp_deskewed_cloud(self._h, _dp(X), _dp(Y), int(bool(local)), C.byref(h)), "glim_amd_ct_gicp_deskewed_cloud")
        g = PointCloudGPU(h, self.source.ctx)
        g._k = getattr(self.source, "_k", 0)
        return g

    def debug_poses(self, values):
        """(time table, T_k n x 4 x 4, D0_k, D1_k n x 6 x 6, time_index) as the library evaluates them at `values`."""
        X, Y = self._xy(values)
        nb = C.c_int32()
        check(lib().glim_amd_debug_ct_gicp_poses(self._h, _dp(X), _dp(Y), C.byref(nb), 0, None, None, None, None, None), "glim_amd_debug_ct_gicp_poses")
        m = nb.value
        tab, T, D0, D1 = np.zeros(m), np.zeros((m, 12)), np.zeros((m, 36)), np.zeros((m, 36))
        idx = np.zeros(self.source.size(), dtype=np.int32)
        check(lib().glim_amd_debug_ct_gicp_poses(self._h, _dp(X), _dp(Y), C.byref(nb), m, _dp(tab), _dp(T), _dp(D0), _dp(D1), _ip(idx)),
              "glim_amd_debug_ct_gicp_poses")
        T44 = np.tile(np.eye(4), (m, 1, 1))
        T44[:, :3, :] = T.reshape(m, 3, 4)
        return tab, T44, D0.reshape(m, 6, 6), D1.reshape(m, 6, 6), idx

    def close(self):
        if self._h:
            lib().glim_amd_ct_gicp_destroy(self._h)
            self._h = None
        self._target.close()
        self.target_tree = self._target.tree

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def median_distance(points, max_scan_count=256):
    """gtsam_points::median_distance (odometry_estimation_gpu.cpp:91, global_mapping.cpp:239): host side, as in the reference."""
    p = np.asarray(points, dtype=np.float64)[:, :3]
    n = len(p)
    if n == 0:
        return 0.0
    step = 1 if n < max_scan_count else n // max_scan_count
    d = np.sort(np.sqrt((p[::step] ** 2).sum(1)))
    return float(d[len(d) // 2])


def adaptive_voxel_resolution(dist_median, voxel_resolution, voxel_resolution_max, voxel_resolution_dmin, voxel_resolution_dmax):
    """base_resolution of odometry_estimation_gpu.cpp:92-93 / global_mapping.cpp:240-241."""
    p = max(0.0, min(1.0, (dist_median - voxel_resolution_dmin) / (voxel_resolution_dmax - voxel_resolution_dmin)))
    return voxel_resolution + p * (voxel_resolution_max - voxel_resolution)


def _pack_frames(poses, frames_points, frames_covs):
    """Host layouts of the reference for a list of frames: poses n x 12, Vector4d points, column-major Matrix4d covariances."""
    nf = len(poses)
    P12 = np.ascontiguousarray(np.stack([pose12(T) for T in poses])) if nf else np.zeros((1, 12))
    p4s, c16s = [], []
    for p, c in zip(frames_points, frames_covs):
        p = np.asarray(p, dtype=np.float64).reshape(-1, np.shape(p)[-1] if np.ndim(p) == 2 else 3)
        n = p.shape[0]
        p4 = np.ones((n, 4))
        p4[:, : p.shape[1]] = p
        c = np.asarray(c, dtype=np.float64)
        c16 = np.zeros((n, 4, 4))
        if c.size == n * 9:
            c16[:, :3, :3] = np.transpose(c.reshape(n, 3, 3), (0, 2, 1))
        else:
            c16[:] = c.reshape(n, 4, 4)
        p4s.append(p4)
        c16s.append(np.ascontiguousarray(c16.reshape(n, 16)))
    sizes = np.array([len(p) for p in p4s], dtype=np.int64)
    dp = C.POINTER(C.c_double)
    pp = (dp * max(nf, 1))(*[_dp(p) for p in p4s])
    cp = (dp * max(nf, 1))(*[_dp(c) for c in c16s])
    return dict(nf=nf, P12=P12, p4s=p4s, c16s=c16s, sizes=sizes, pp=pp, cp=cp)


def merge_frames(poses, frames_points, frames_covs, downsample_resolution, target_num_points=-1, seed=0, block_size=1024, ctx=None, packed=None):
    """gtsam_points::merge_frames (sub_mapping.cpp:480-497) on the device.  poses[f]: T_origin_frame; frames_points[f]: N_f x 3 / x 4;
    frames_covs[f]: N_f x 3 x 3 / 4 x 4.  Returns the merged PointCloudGPU (points + covariances)."""
    ctx = ctx or default_context()
    k = packed if packed is not None else _pack_frames(poses, frames_points, frames_covs)
    h = C.c_void_p()
    check(lib().glim_amd_merge_frames(ctx._h, k["nf"], _dp(k["P12"]), k["pp"], k["cp"], k["sizes"].ctypes.data_as(C.POINTER(C.c_int64)),
                                      float(downsample_resolution), int(target_num_points), int(block_size), int(seed), C.byref(h)), "glim_amd_merge_frames")
    return PointCloudGPU(h, ctx)


def debug_sort_pairs(keys, vals=None, bits=64, ctx=None):
    """The stable device radix sort behind the preprocessing (parity / debug)."""
    ctx = ctx or default_context()
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    v = None if vals is None else np.ascontiguousarray(vals, dtype=np.uint32)
    ko, vo = np.zeros_like(k), np.zeros(len(k), dtype=np.uint32)
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    check(lib().glim_amd_debug_sort_pairs(ctx._h, len(k), int(bits), k.ctypes.data_as(u64p), None if v is None else v.ctypes.data_as(u32p),
                                          ko.ctypes.data_as(u64p), vo.ctypes.data_as(u32p)), "glim_amd_debug_sort_pairs")
    return ko, vo


def debug_exclusive_scan(values, ctx=None):
    """The device's exclusive prefix sum of int32 values (csrc/scan.hpp) behind every stable compaction (parity / debug)."""
    ctx = ctx or default_context()
    v = np.ascontiguousarray(values, dtype=np.int32).reshape(-1)
    out = np.zeros_like(v)
    check(lib().glim_amd_debug_exclusive_scan(ctx._h, len(v), _ip(v) if len(v) else None, _ip(out) if len(v) else None), "glim_amd_debug_exclusive_scan")
    return out


def debug_select_smallest(keys, m, ctx=None):
    """The selection stage of PointCloudGPU.random_sampling on caller-supplied 32-bit keys: keep[i] = 1 iff (keys[i], i) is among the m
    smallest pairs (parity / debug)."""
    ctx = ctx or default_context()
    k = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1)
    keep = np.zeros(len(k), dtype=np.int32)
    check(lib().glim_amd_debug_select_smallest(ctx._h, len(k), k.ctypes.data_as(C.POINTER(C.c_uint32)) if len(k) else None, int(m),
                                               _ip(keep) if len(k) else None), "glim_amd_debug_select_smallest")
    return keep


def expand_compact(compact, T_target_source, flags):
    c = np.ascontiguousarray(compact, dtype=np.float64).reshape(_lib.COMPACT_DOUBLES)
    T = pose12(T_target_source)
    L = Linearized6()
    check(lib().glim_amd_expand_compact(_dp(c), _dp(T), int(flags), C.byref(L)), "glim_amd_expand_compact")
    return _lin_to_dict(L)


def overlap_gpu(target_voxelmaps, source, deltas, ctx=None):
    """gtsam_points::overlap_gpu: single (voxelmap, source, delta) or multi-target (voxelmaps[], source, deltas[])."""
    if isinstance(target_voxelmaps, GaussianVoxelMapGPU):
        target_voxelmaps, deltas = [target_voxelmaps], [deltas]
    ctx = ctx or source.ctx
    hs = (C.c_void_p * len(target_voxelmaps))(*[m._h.value for m in target_voxelmaps])
    T = np.ascontiguousarray(np.stack([pose12(d) for d in deltas]))
    out = C.c_double()
    check(lib().glim_amd_overlap(ctx._h, len(target_voxelmaps), hs, _dp(T), source._h, C.byref(out)), "glim_amd_overlap")
    return out.value


overlap_auto = overlap_gpu


def _overlap_args(queries):
    nt = np.array([len(q[0]) for q in queries], dtype=np.int32)
    maps = [m._h.value for q in queries for m in q[0]]
    hs = (C.c_void_p * len(maps))(*maps)
    srcs = (C.c_void_p * len(queries))(*[q[1]._h.value for q in queries])
    T = np.ascontiguousarray(np.stack([pose12(d) for q in queries for d in q[2]]))
    return nt, hs, srcs, T


def overlap_profile(queries, iters=200, ctx=None):
    """microseconds per glim_amd_overlap_batch call answering `queries` ([(voxelmaps[], source, deltas[]), ...]), timed inside the library."""
    ctx = ctx or queries[0][1].ctx
    nt, hs, srcs, T = _overlap_args(queries)
    us = C.c_float()
    check(lib().glim_amd_overlap_profile(ctx._h, len(queries), _ip(nt), hs, _dp(T), srcs, int(iters), C.byref(us)), "glim_amd_overlap_profile")
    return us.value


def profile_fresh_sets(factors, T_target_source, iters=200, ctx=None):
    """GLIM's live pattern -- a fresh NonlinearFactorSetGPU per linearisation: create, add every factor, linearize, destroy -- timed inside
    the library; microseconds per iteration.  factors: IntegratedVGICPFactorGPU objects; T_target_source: n x 12."""
    ctx = ctx or factors[0].source.ctx
    n = len(factors)
    maps = (C.c_void_p * n)(*[f.target_voxelmap._h.value for f in factors])
    srcs = (C.c_void_p * n)(*[f.source._h.value for f in factors])
    flags = (C.c_uint32 * n)(*[f.flags() for f in factors])
    T = np.ascontiguousarray(T_target_source, dtype=np.float64)
    us = C.c_float()
    check(lib().glim_amd_factor_set_profile_fresh(ctx._h, n, maps, srcs, flags, _dp(T), int(iters), C.byref(us)), "glim_amd_factor_set_profile_fresh")
    return us.value


def profile_fresh_sets_samples(factors, T_target_source, iters=200, gap_us=0.0, ctx=None):
    """profile_fresh_sets with every iteration timed on its own: microseconds per iteration (array of `iters`); `gap_us` of host work between
    two iterations."""
    ctx = ctx or factors[0].source.ctx
    n = len(factors)
    maps = (C.c_void_p * n)(*[f.target_voxelmap._h.value for f in factors])
    srcs = (C.c_void_p * n)(*[f.source._h.value for f in factors])
    flags = (C.c_uint32 * n)(*[f.flags() for f in factors])
    T = np.ascontiguousarray(T_target_source, dtype=np.float64)
    out = np.zeros(int(iters), dtype=np.float32)
    check(lib().glim_amd_factor_set_profile_fresh_samples(ctx._h, n, maps, srcs, flags, _dp(T), int(iters), float(gap_us), out.ctypes.data_as(C.POINTER(C.c_float))),
          "glim_amd_factor_set_profile_fresh_samples")
    return out


def overlap_gpu_batch(queries, ctx=None):
    """Many overlap_gpu calls in ONE launch (the keyframe-selection loops of odometry_estimation_gpu.cpp:262-281 issue K of them back to
    back): queries = [(target_voxelmaps[], source, deltas[]), ...] -> list of overlaps."""
    if not queries:
        return []
    ctx = ctx or queries[0][1].ctx
    nt, hs, srcs, T = _overlap_args(queries)
    out = np.zeros(len(queries), dtype=np.float64)
    check(lib().glim_amd_overlap_batch(ctx._h, len(queries), _ip(nt), hs, _dp(T), srcs, _dp(out)), "glim_amd_overlap_batch")
    return out.tolist()


# ---- plane / edge bundle-adjustment factors and ball selection (include/glim_amd.h) ----
def clone_exact(points, ctx=None):
    """A cloud that keeps its points in FP64 (glim_amd_cloud_create_exact): what the ball selection reads without the rounding of clone()."""
    ctx = ctx or default_context()
    points = np.asarray(points, dtype=np.float64).reshape(len(points), -1) if len(points) else np.zeros((0, 3))
    p4 = np.ones((len(points), 4), dtype=np.float64)
    p4[:, :3] = points[:, :3]
    h = C.c_void_p()
    check(lib().glim_amd_cloud_create_exact(ctx._h, len(p4), _dp(p4), C.byref(h)), "glim_amd_cloud_create_exact")
    return PointCloudGPU(h, ctx)


class BundleAdjustmentParams:
    """The radius search's limits (bundle_adjustment_modal.cpp:21-25)."""

    def __init__(self, min_radius=0.1, max_radius=5.0, plane_eps=0.01):
        self.min_radius, self.max_radius, self.plane_eps = float(min_radius), float(max_radius), float(plane_eps)

    def _c(self):
        return _lib.BaParams(self.min_radius, self.max_radius, self.plane_eps)


def _ball_args(clouds, poses, center):
    S = len(clouds)
    if len(poses) != S:
        raise ValueError("one pose per cloud")
    T = np.zeros((max(S, 1), 12))
    for i, Ti in enumerate(poses):
        T[i] = pose12(Ti)
    c = np.ascontiguousarray(np.asarray(center, dtype=np.float64).reshape(3))
    hs = (C.c_void_p * max(S, 1))(*[cl._h for cl in clouds])
    return hs, S, T, c


def ba_ball_select(clouds, poses, center, radius, capacity=None):
    """extract_points (bundle_adjustment_modal.cpp:143-161) over device clouds: -> (pairs, count).  pairs: min(count, capacity) x 2 int32
    (sub-map index, point index), ascending; count: how many points the ball holds, whatever the capacity (default: every point)."""
    hs, S, T, c = _ball_args(clouds, poses, center)
    if capacity is None:
        capacity = sum(cl.size() for cl in clouds)
    pairs = np.zeros((max(int(capacity), 1), 2), dtype=np.int32)
    n = C.c_int64()
    check(lib().glim_amd_ba_ball_select(hs, S, _dp(T), _dp(c), float(radius), int(capacity), _ip(pairs), C.byref(n)), "glim_amd_ba_ball_select")
    return pairs[: min(n.value, int(capacity))].copy(), n.value


def ba_ball_stats(clouds, poses, center, radius):
    """calc_eigenvalues (:163-184) of the ball's points: {num_points, sum (3), sum_cross (3 x 3), eigenvalues (3, ascending)}."""
    hs, S, T, c = _ball_args(clouds, poses, center)
    out = _lib.BaStats()
    check(lib().glim_amd_ba_ball_stats(hs, S, _dp(T), _dp(c), float(radius), C.byref(out)), "glim_amd_ba_ball_stats")
    s6 = np.array(out.sum_cross[:])
    return {"num_points": out.num_points, "sum": np.array(out.sum[:]), "eigenvalues": np.array(out.eigenvalues[:]),
            "sum_cross": np.array([[s6[0], s6[1], s6[2]], [s6[1], s6[3], s6[4]], [s6[2], s6[4], s6[5]]])}


BA_STOP = {0: "trials", 1: "range", 2: "few_points", 3: "plane_eps"}
BA_DECISION = {0: "initial", 1: "taken", 2: "range", 3: "few_points", 4: "plane_eps"}


def ba_auto_radius(clouds, poses, center, radius, params=None, trace=False):
    """auto_radius (:186-227) in one call and one host synchronisation: {radius, num_points, eigenvalues, trials, stop}; with trace=True
    also "trace": one {radius, count, eigenvalues, decision} per evaluation (the window of include/glim_amd_diag.h)."""
    hs, S, T, c = _ball_args(clouds, poses, center)
    prm = (params or BundleAdjustmentParams())._c()
    out = _lib.BaRadiusResult()
    if trace:
        ent = (_lib.BaTraceEntry * (_lib.BA_MAX_TRIALS + 1))()
        ne = C.c_int32()
        check(lib().glim_amd_debug_ba_auto_radius_trace(hs, S, _dp(T), _dp(c), float(radius), C.byref(prm), C.byref(out), ent, C.byref(ne)),
              "glim_amd_debug_ba_auto_radius_trace")
    else:
        check(lib().glim_amd_ba_auto_radius(hs, S, _dp(T), _dp(c), float(radius), C.byref(prm), C.byref(out)), "glim_amd_ba_auto_radius")
    res = {"radius": out.radius, "num_points": out.num_points, "eigenvalues": np.array(out.eigenvalues[:]), "trials": out.trials,
           "stop": BA_STOP.get(out.stop, out.stop)}
    if trace:
        res["trace"] = [{"radius": e.radius, "count": e.count, "eigenvalues": np.array(e.eigenvalues[:]), "decision": BA_DECISION.get(e.decision, e.decision)}
                        for e in ent[: ne.value]]
    return res


def ba_debug_eigen3(matrices, ctx=None):
    """csrc/eig3_direct.hpp on the device, one thread per 3 x 3 symmetric matrix: -> (eigenvalues n x 3 ascending, eigenvectors n x 3 x 3 with
    [i, k] the k-th eigenvector)."""
    ctx = ctx or default_context()
    m = np.ascontiguousarray(np.asarray(matrices, dtype=np.float64).reshape(-1, 9))
    lam, U = np.zeros((len(m), 3)), np.zeros((len(m), 9))
    check(lib().glim_amd_debug_ba_eigen3(ctx._h, len(m), _dp(m), _dp(lam), _dp(U)), "glim_amd_debug_ba_eigen3")
    return lam, U.reshape(-1, 3, 3)


class PlaneEVMFactor:
    """gtsam_points::PlaneEVMFactor on the device: the cost is the smallest eigenvalue of the covariance of the points of K frames moved by
    their poses.  The points are reduced to per-frame moments once, at creation; error() and linearize() read the moments only."""

    KIND = 0

    def __init__(self, handle, ctx):
        self._h, self.ctx = handle, ctx
        K, N = C.c_int32(), C.c_int64()
        check(lib().glim_amd_ba_factor_info(self._h, C.byref(K), C.byref(N), None, None, None), "glim_amd_ba_factor_info")
        self._K, self._N = K.value, N.value

    @classmethod
    def from_ball(cls, clouds, poses, center, radius):
        """The factor create_factor builds (:229-245): the ball's points, frame by frame, without leaving the device.  frames() are the
        indices of the clouds that had a point in the ball."""
        hs, S, T, c = _ball_args(clouds, poses, center)
        h = C.c_void_p()
        check(lib().glim_amd_ba_factor_create_from_ball(hs, S, _dp(T), _dp(c), float(radius), cls.KIND, C.byref(h)), "glim_amd_ba_factor_create_from_ball")
        return cls(h, clouds[0].ctx)

    @classmethod
    def from_points(cls, points, frame_index, num_frames=None, ctx=None):
        """points: n x 3, frame-local; frame_index: n entries in [0, num_frames).  What add(point, key) collects."""
        ctx = ctx or default_context()
        p = np.ascontiguousarray(np.asarray(points, dtype=np.float64)[:, :3])
        fi = np.ascontiguousarray(np.asarray(frame_index, dtype=np.int32))
        if len(fi) != len(p):
            raise ValueError("one frame index per point")
        if num_frames is None:
            num_frames = int(fi.max()) + 1 if len(fi) else 0
        h = C.c_void_p()
        check(lib().glim_amd_ba_factor_create(ctx._h, cls.KIND, len(p), _dp(p), _ip(fi), int(num_frames), C.byref(h)), "glim_amd_ba_factor_create")
        return cls(h, ctx)

    def num_points(self):
        return self._N

    def num_frames(self):
        return self._K

    def frames(self):
        kept = np.zeros(self._K, dtype=np.int32)
        check(lib().glim_amd_ba_factor_info(self._h, None, None, None, _ip(kept), None), "glim_amd_ba_factor_info")
        return kept

    def moments(self):
        """K x 13: n | c_f | v_f | P_f (00 01 02 11 12 22)"""
        m = np.zeros((self._K, _lib.BA_MOMENT_DOUBLES))
        check(lib().glim_amd_ba_factor_info(self._h, None, None, None, None, _dp(m)), "glim_amd_ba_factor_info")
        return m

    def _poses(self, poses):
        if len(poses) != self._K:
            raise ValueError(f"{self._K} poses expected")
        T = np.zeros((self._K, 12))
        for i, Ti in enumerate(poses):
            T[i] = pose12(Ti)
        return T

    def error(self, poses, with_status=False):
        T = self._poses(poses)
        cost, st = C.c_double(), C.c_uint32()
        check(lib().glim_amd_ba_factor_error(self._h, _dp(T), C.byref(cost), C.byref(st)), "glim_amd_ba_factor_error")
        return (cost.value, st.value) if with_status else cost.value

    def linearize(self, poses):
        """{cost, g (6 K), H (6 K x 6 K), status}; tangent order [rotation, translation] per frame, perturbation T Exp(xi).  The
        HessianFactor of it is (G = H, g = -g, f = 2 cost)."""
        T = self._poses(poses)
        n = 6 * self._K
        cost, st = C.c_double(), C.c_uint32()
        g, H = np.zeros(n), np.zeros((n, n))
        check(lib().glim_amd_ba_factor_linearize(self._h, _dp(T), C.byref(cost), _dp(g), _dp(H), C.byref(st)), "glim_amd_ba_factor_linearize")
        return {"cost": cost.value, "g": g, "H": H, "status": st.value}

    def close(self):
        if self._h:
            check(lib().glim_amd_ba_factor_destroy(self._h), "glim_amd_ba_factor_destroy")
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EdgeEVMFactor(PlaneEVMFactor):
    """gtsam_points::EdgeEVMFactor: the cost is the sum of the two smallest eigenvalues."""

    KIND = 1


# ---- map editing: point selection, region growing, removal (include/glim_amd.h "Map editing") ----
EDIT_BOX, EDIT_SPHERE, EDIT_WINDOW, EDIT_WINDOW_BALL = _lib.EDIT_BOX, _lib.EDIT_SPHERE, _lib.EDIT_WINDOW, _lib.EDIT_WINDOW_BALL
EDIT_ROUNDS_PER_LOOK = _lib.EDIT_ROUNDS_PER_LOOK
EDIT_OK, EDIT_EMPTY, EDIT_FEW_POINTS, EDIT_NO_SEED, EDIT_ROUND_LIMIT = _lib.EDIT_OK, _lib.EDIT_EMPTY, _lib.EDIT_FEW_POINTS, _lib.EDIT_NO_SEED, _lib.EDIT_ROUND_LIMIT
EDIT_CAP_SCALE, EDIT_MIN_CUT_MAX_ROUNDS = _lib.EDIT_CAP_SCALE, _lib.EDIT_MIN_CUT_MAX_ROUNDS
EDIT_STATUS = {_lib.EDIT_OK: "ok", _lib.EDIT_EMPTY: "empty", _lib.EDIT_FEW_POINTS: "few_points", _lib.EDIT_NO_SEED: "no_seed",
               _lib.EDIT_ROUND_LIMIT: "round_limit"}


class RegionGrowingParams:
    """Region growing over the candidates of the window.  The three thresholds' defaults are a recollection of
    gtsam_points::RegionGrowingParams, which is not in the reference tree.  angle_threshold is in radians; its cosine is taken once, here."""

    def __init__(self, distance_threshold=0.5, angle_threshold=np.deg2rad(10.0), dilation_radius=0.5, use_normals=False, max_hops=0):
        self.distance_threshold, self.angle_threshold, self.dilation_radius = float(distance_threshold), float(angle_threshold), float(dilation_radius)
        self.use_normals, self.max_hops = bool(use_normals), int(max_hops)

    def cos_angle_threshold(self):
        return float(np.cos(self.angle_threshold))

    def _c(self):
        return _lib.EditRegionGrowingParams(self.distance_threshold, self.cos_angle_threshold(), self.dilation_radius, int(self.use_normals), self.max_hops)


def _edit_matrices(clouds, matrices):
    S = len(clouds)
    if len(matrices) != S:
        raise ValueError("one matrix per cloud")
    M = np.zeros((max(S, 1), 12))
    for i, Mi in enumerate(matrices):
        M[i] = pose12(Mi)
    hs = (C.c_void_p * max(S, 1))(*[cl._h for cl in clouds])
    return hs, S, M


def _edit_window(center, resolution, window):
    c = np.asarray(center, dtype=np.float64).reshape(3)
    return _lib.EditWindow((C.c_double * 3)(*c), float(resolution), int(window), 0)


def edit_local_matrices(model_matrix, poses):
    """T_local_submap = inv(model matrix) T_world_submap per sub-map (points_selector.cpp:630, :637), FP64 on the host: S matrices 3 x 4."""
    inv = np.linalg.inv(np.asarray(model_matrix, dtype=np.float64).reshape(4, 4))
    out = []
    for T in poses:
        T4 = np.eye(4)
        T4[:3, :4] = np.asarray(T, dtype=np.float64)[:3, :4]
        out.append((inv @ T4)[:3, :4].copy())
    return out


def edit_select(clouds, poses, mode, model_matrix=None, center=None, radius=0.0, resolution=2.0, window=5, capacity=None):
    """The editor's selections over device clouds -> (pairs, count).  mode EDIT_BOX / EDIT_SPHERE: the unit box / sphere of the gizmo's
    model matrix (select_points_tool, :623-674); EDIT_WINDOW: the cells around `center` (collect_neighbor_point_ids, :85-112);
    EDIT_WINDOW_BALL: those within `radius` of it (select_points_radius, :677-700).  pairs: min(count, capacity) x 2 int32 (sub-map, point),
    ascending."""
    if mode in (EDIT_BOX, EDIT_SPHERE):
        hs, S, M = _edit_matrices(clouds, edit_local_matrices(model_matrix, poses))
        win = None
    else:
        hs, S, M = _edit_matrices(clouds, poses)
        win = C.byref(_edit_window(center, resolution, window))
    if capacity is None:
        capacity = sum(cl.size() for cl in clouds)
    pairs = np.zeros((max(int(capacity), 1), 2), dtype=np.int32)
    n = C.c_int64()
    check(lib().glim_amd_edit_select(hs, S, _dp(M), int(mode), win, float(radius), int(capacity), _ip(pairs), C.byref(n)), "glim_amd_edit_select")
    return pairs[: min(n.value, int(capacity))].copy(), n.value


def edit_select_outliers(clouds, poses, center, radius, radius_offset=1.0, num_neighbors=10, stddev_thresh=2.0, resolution=2.0, window=5, capacity=None):
    """select_outlier_points_radius (:703-759) -> (pairs, count, status): the points within `radius` of `center` whose mean distance to
    their k nearest neighbours -- among the points within radius + radius_offset -- is not below mean + stddev_thresh * std.
    status "few_points": fewer candidates than k, nothing selected."""
    hs, S, M = _edit_matrices(clouds, poses)
    win = _edit_window(center, resolution, window)
    prm = _lib.EditOutlierParams(float(radius_offset), float(stddev_thresh), int(num_neighbors), 0)
    if capacity is None:
        capacity = sum(cl.size() for cl in clouds)
    pairs = np.zeros((max(int(capacity), 1), 2), dtype=np.int32)
    n, st = C.c_int64(), C.c_int32()
    check(lib().glim_amd_edit_select_outliers(hs, S, _dp(M), C.byref(win), float(radius), C.byref(prm), int(capacity), _ip(pairs), C.byref(n), C.byref(st)),
          "glim_amd_edit_select_outliers")
    return pairs[: min(n.value, int(capacity))].copy(), n.value, EDIT_STATUS.get(st.value, st.value)


def edit_region_grow(clouds, poses, center, params=None, resolution=2.0, window=5, capacity=None):
    """select_points_segmentation, region growing (:798-810) -> {pairs, levels, count, num_candidates, seed, seed_qq, rounds, status}.
    pairs ascending; levels[i] = hops of pairs[i] from the seed (dilated points: last level + 1)."""
    hs, S, M = _edit_matrices(clouds, poses)
    win = _edit_window(center, resolution, window)
    prm = (params or RegionGrowingParams())._c()
    if capacity is None:
        capacity = sum(cl.size() for cl in clouds)
    pairs = np.zeros((max(int(capacity), 1), 2), dtype=np.int32)
    levels = np.zeros(max(int(capacity), 1), dtype=np.int32)
    out = _lib.EditRegionResult()
    check(lib().glim_amd_edit_region_grow(hs, S, _dp(M), C.byref(win), C.byref(prm), int(capacity), _ip(pairs), _ip(levels), C.byref(out)),
          "glim_amd_edit_region_grow")
    wr = min(out.count, int(capacity))
    return {"pairs": pairs[:wr].copy(), "levels": levels[:wr].copy(), "count": out.count, "num_candidates": out.num_candidates,
            "seed": (out.seed[0], out.seed[1]), "seed_qq": out.seed_qq, "rounds": out.rounds, "status": EDIT_STATUS.get(out.status, out.status)}


class MinCutParams:
    """Min-cut segmentation around the picked point (include/glim_amd.h "Map editing", min-cut).  The sigmas and k are a recollection of
    gtsam_points::MinCutParams, which is not in the reference tree; the radii and the weight are the editor's (points_selector.cpp:42-44).
    angle_sigma is in radians.  background_weight 0: the foreground weight.  max_rounds 0: EDIT_MIN_CUT_MAX_ROUNDS."""

    def __init__(self, distance_sigma=0.25, angle_sigma=np.deg2rad(10.0), foreground_mask_radius=0.5, background_mask_radius=5.0, foreground_weight=10.0,
                 background_weight=0.0, k_neighbors=20, use_normals=False, max_rounds=0):
        self.distance_sigma, self.angle_sigma = float(distance_sigma), float(angle_sigma)
        self.foreground_mask_radius, self.background_mask_radius = float(foreground_mask_radius), float(background_mask_radius)
        self.foreground_weight, self.background_weight = float(foreground_weight), float(background_weight)
        self.k_neighbors, self.use_normals, self.max_rounds = int(k_neighbors), bool(use_normals), int(max_rounds)

    def _c(self):
        return _lib.EditMinCutParams(self.distance_sigma, self.angle_sigma, self.foreground_mask_radius, self.background_mask_radius, self.foreground_weight,
                                     self.background_weight, self.k_neighbors, int(self.use_normals), self.max_rounds, 0)


def _min_cut_counts(out):
    return {"count": out.count, "num_candidates": out.num_candidates, "num_edges": out.num_edges, "num_foreground": out.num_foreground,
            "num_background": out.num_background, "flow": out.flow, "rounds": out.rounds, "looks": out.looks, "status": EDIT_STATUS.get(out.status, out.status)}


def edit_min_cut(clouds, poses, center, params=None, resolution=2.0, window=5, capacity=None):
    """select_points_segmentation, min-cut (:774-797) -> {pairs, count, num_candidates, num_edges, num_foreground, num_background, flow,
    rounds, looks, status}.  pairs ascending: the points on the source side of the minimal minimum cut between the points within the
    foreground radius of `center` and those beyond the background radius, over the k-nearest-neighbour graph of the candidates."""
    hs, S, M = _edit_matrices(clouds, poses)
    win = _edit_window(center, resolution, window)
    prm = (params or MinCutParams())._c()
    if capacity is None:
        capacity = sum(cl.size() for cl in clouds)
    pairs = np.zeros((max(int(capacity), 1), 2), dtype=np.int32)
    out = _lib.EditMinCutResult()
    check(lib().glim_amd_edit_min_cut(hs, S, _dp(M), C.byref(win), C.byref(prm), int(capacity), _ip(pairs), C.byref(out)), "glim_amd_edit_min_cut")
    res = _min_cut_counts(out)
    res["pairs"] = pairs[: min(out.count, int(capacity))].copy()
    return res


def diag_edit_min_cut_graph(clouds, poses, center, params=None, resolution=2.0, window=5):
    """glim_amd_diag_edit_min_cut_graph: the graph edit_min_cut builds -> {candidates, source_cap, sink_cap, edges, edge_cap, + the counts}"""
    hs, S, M = _edit_matrices(clouds, poses)
    win = _edit_window(center, resolution, window)
    prm = (params or MinCutParams())._c()
    out = _lib.EditMinCutResult()
    none = None
    check(lib().glim_amd_diag_edit_min_cut_graph(hs, S, _dp(M), C.byref(win), C.byref(prm), 0, none, none, none, 0, none, none, C.byref(out)),
          "glim_amd_diag_edit_min_cut_graph")
    m, E = max(out.num_candidates, 1), max(out.num_edges, 1)
    pairs, src, snk = np.zeros((m, 2), dtype=np.int32), np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32)
    edges, cap = np.zeros((E, 2), dtype=np.int32), np.zeros(E, dtype=np.int32)
    check(lib().glim_amd_diag_edit_min_cut_graph(hs, S, _dp(M), C.byref(win), C.byref(prm), m, _ip(pairs), _ip(src), _ip(snk), E, _ip(edges), _ip(cap),
                                                 C.byref(out)), "glim_amd_diag_edit_min_cut_graph")
    res = _min_cut_counts(out)
    m, E = out.num_candidates, out.num_edges
    res.update(candidates=pairs[:m].copy(), source_cap=src[:m].copy(), sink_cap=snk[:m].copy(), edges=edges[:E].copy(), edge_cap=cap[:E].copy())
    return res


def diag_max_flow(ctx, n, edges, edge_cap, source_cap, sink_cap, max_rounds=0):
    """glim_amd_diag_max_flow: the min-cut solver alone on a caller's undirected graph -> {member, flow, rounds, looks, status}"""
    edges = np.ascontiguousarray(np.asarray(edges, dtype=np.int32).reshape(-1, 2))
    cap = np.ascontiguousarray(np.asarray(edge_cap, dtype=np.int32).reshape(-1))
    src = np.ascontiguousarray(np.asarray(source_cap, dtype=np.int32).reshape(-1))
    snk = np.ascontiguousarray(np.asarray(sink_cap, dtype=np.int32).reshape(-1))
    if len(cap) != len(edges) or len(src) != n or len(snk) != n:
        raise ValueError("one capacity per edge, one source and one sink capacity per node")
    member = np.zeros(max(int(n), 1), dtype=np.int32)
    flow, rounds, looks, status = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
    ptr = lambda a: _ip(a) if len(a) else None  # noqa: E731
    check(lib().glim_amd_diag_max_flow(ctx._h, int(n), len(edges), ptr(edges), ptr(cap), ptr(src), ptr(snk), int(max_rounds), _ip(member), C.byref(flow),
                                       C.byref(rounds), C.byref(looks), C.byref(status)), "glim_amd_diag_max_flow")
    return {"member": member[: int(n)].copy(), "flow": flow.value, "rounds": rounds.value, "looks": looks.value,
            "status": EDIT_STATUS.get(status.value, status.value)}


def edit_remove_points(cloud, indices):
    """A NEW cloud without the listed points (any order, duplicates allowed), the others in their original order with every per-point array
    the cloud holds; the input cloud is untouched (gtsam_points::sample with the surviving indices, :537-562).  Neighbours are dropped."""
    idx = np.ascontiguousarray(np.asarray(indices, dtype=np.int32).reshape(-1))
    h = C.c_void_p()
    check(lib().glim_amd_edit_remove_points(cloud._h, len(idx), _ip(idx) if len(idx) else None, C.byref(h)), "glim_amd_edit_remove_points")
    g = PointCloudGPU(h, cloud.ctx)
    g._k = 0
    g._has_intensities = getattr(cloud, "_has_intensities", False)
    return g


def edit_remove_selected(clouds, pairs):
    """remove_selected_points (:513-562): the sorted pairs are partitioned by sub-map, and every sub-map that is touched gets a new cloud.
    -> a list like `clouds` in which the untouched sub-maps are the very objects passed in."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    ids = np.sort((pairs[:, 0].astype(np.uint64) << np.uint64(32)) | pairs[:, 1].astype(np.uint64))
    sub = (ids >> np.uint64(32)).astype(np.int64)
    out = list(clouds)
    for s in np.unique(sub):
        out[int(s)] = edit_remove_points(clouds[int(s)], (ids[sub == s] & np.uint64(0xFFFFFFFF)).astype(np.int32))
    return out
