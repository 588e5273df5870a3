/*
 * glim_amd.h -- C ABI of the MI355X-native (gfx950) VGICP scan-matching hot path for GLIM.
 * gtsam_points' matching-cost family as the reference calls it is all here: the VGICP, GICP, continuous-time GICP and ICP factors, and the
 * fine registrations over them (GICP, ICP, VGICP, CT frame alignment, sub-map bundle), each one loop on the device.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch/Eigen types.  Each entry
 * point names the reference interface it replaces.  The reference (koide3/glim v1.2.2) reaches this path through
 * koide3/gtsam_points (un-vendored, CMakeLists.txt:28); the file:line citations are GLIM's call sites of those
 * gtsam_points symbols, relative to /root/reference.
 *
 * Conventions
 *   - return value: 0 = GLIM_AMD_OK, < 0 = error code (glim_amd_error_string).  Never throws, never aborts.
 *   - poses: 12 doubles, row-major 3x4 [R | t]  (Eigen::Isometry3d::matrix().topRows<3>()).
 *     T_target_source = T_target^-1 * T_source for binary factors, fixed_target_pose^-1 * T_source for unary ones.
 *   - tangent order [omega(3); v(3)] (gtsam::Pose3), right perturbation T (+) xi = T * Exp(xi).
 *   - host point layouts are the reference's: Eigen::Vector4d points / normals (stride 4 doubles), Eigen::Matrix4d
 *     covariances (16 doubles, column-major, zero last row/col)   include/glim/preprocess/preprocessed_frame.hpp:31,
 *     src/glim/common/cloud_covariance_estimation.cpp:96.  Host arrays are borrowed only for the duration of a call.
 *   - all device work of a context runs on its HIP stream(s); calls are synchronous unless named *_async.
 *   - handles are owned by the caller; destroy children (clouds, voxel maps, iVox maps, factor sets, search indices) before their context:
 *     glim_amd_ctx_destroy refuses (GLIM_AMD_ERR_STATE) while any child is alive.
 */
#ifndef GLIM_AMD_H
#define GLIM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLIM_AMD_VERSION 100 /* 0.1.0 */

enum {
  GLIM_AMD_OK = 0,
  GLIM_AMD_ERR_INVALID = -1,     /* bad argument */
  GLIM_AMD_ERR_HIP = -2,         /* HIP runtime failure (glim_amd_last_hip_error) */
  GLIM_AMD_ERR_NO_DEVICE = -3,   /* no gfx950 device visible */
  GLIM_AMD_ERR_RANGE = -4,       /* voxel coordinate outside the +-2^20 key range */
  GLIM_AMD_ERR_STATE = -5,       /* call not valid in this state (e.g. covariances requested before kNN) */
  GLIM_AMD_ERR_UNSUPPORTED = -6, /* not implemented in this build */
  GLIM_AMD_ERR_NOMEM = -7
};

typedef struct glim_amd_ctx glim_amd_ctx;                 /* device + stream pool (CUDAStream / StreamTempBufferRoundRobin) */
typedef struct glim_amd_cloud glim_amd_cloud;             /* gtsam_points::PointCloudGPU */
typedef struct glim_amd_voxelmap glim_amd_voxelmap;       /* gtsam_points::GaussianVoxelMapGPU */
typedef struct glim_amd_factor_set glim_amd_factor_set;   /* gtsam_points::NonlinearFactorSetGPU of IntegratedVGICPFactorGPU */

/* Result of one factor linearisation -- the FP64 image of gtsam_points' LinearizedSystem6.
 * H_* row-major 6x6.  gtsam::HessianFactor(k_t, k_s, H_tt, H_ts, -b_t, H_ss, -b_s, error)  (unary: k_s, H_ss, -b_s, error). */
typedef struct {
  int64_t num_inliers;
  double error;
  double H_tt[36];
  double H_ss[36];
  double H_ts[36];
  double b_t[6];
  double b_s[6];
} glim_amd_linearized6;

/* factor flags */
#define GLIM_AMD_FACTOR_BINARY 0x1             /* fill H_tt, H_ts, b_t (otherwise they are zero: unary factor) */
#define GLIM_AMD_FACTOR_SURFACE_VALIDATION 0x2 /* IntegratedVGICPFactorGPU::set_enable_surface_validation(true) */
#define GLIM_AMD_ICP_POINT_TO_PLANE 0x4        /* the ICP factors ("ICP factors" below): IntegratedPointToPlaneICPFactor; otherwise point-to-point */

/* ---- library / context --------------------------------------------------------------------------------------- */
int glim_amd_version(void);
const char* glim_amd_error_string(int code);
/* last HIP error text seen by this thread's failing call ("" if none). */
const char* glim_amd_last_hip_error(void);
/* number of visible HIP devices (0 on a CPU-only box; never fails). */
int glim_amd_device_count(void);

/* Replaces gtsam_points::CUDAStream + StreamTempBufferRoundRobin(num_streams)
 * (src/glim/odometry/odometry_estimation_gpu.cpp:76-77, src/glim/mapping/sub_mapping.cpp:86-87, global_mapping.cpp:110).
 * external_stream: a hipStream_t to run on (e.g. torch's current stream) or NULL to create `num_streams` streams.  The null stream is
 * named explicitly: pass hipStreamLegacy ((hipStream_t)1) or hipStreamPerThread ((hipStream_t)2), never 0. */
int glim_amd_ctx_create(int device, int num_streams, void* external_stream, glim_amd_ctx** out);
/* The same with a scheduling priority for the context's own streams: 0 = default, 1 = the device's greatest stream priority, -1 = its least.
 * GLIM runs three modules in three threads on one device, each with its own stream pool (async_odometry_estimation.cpp:15 /
 * odometry_estimation_gpu.cpp:76-77, async_sub_mapping.cpp:8 / sub_mapping.cpp:86-87, async_global_mapping.cpp:24 / global_mapping.cpp:110):
 * one context per module, the odometry's with priority 1, keeps a 25 us odometry linearisation from queueing behind a sub-mapping merge on
 * the host (a context's calls serialise on ITS mutex only) and behind a 10 ms global-mapping kernel on the device.
 * Clouds, voxel maps and search indices may be used by calls and factor sets of ANY context of the same device (the modules hand frames and
 * maps to one another); an object is destroyed through, and counted by, the context that created it. */
int glim_amd_ctx_create_ex(int device, int num_streams, void* external_stream, int priority, glim_amd_ctx** out);
/* GLIM_AMD_ERR_STATE (and the context stays valid) while clouds, voxel maps, factor sets or search indices created from it are alive. */
int glim_amd_ctx_destroy(glim_amd_ctx* ctx);
int glim_amd_ctx_synchronize(glim_amd_ctx* ctx);
/* gtsam_points::cuda_device_names / cuda_mem_get_info (src/glim/util/debug.cpp:84, viewer/memory_monitor.cpp:39). */
int glim_amd_device_info(glim_amd_ctx* ctx, char* name, size_t name_len, size_t* free_bytes, size_t* total_bytes, int* num_cus);

/* ---- point clouds: PointCloudGPU::clone (odometry_estimation_gpu.cpp:96, sub_mapping.cpp:168,393, global_mapping.cpp:253,260,743) */
/* points4: n x 4 doubles (required).  covs16: n x 16 doubles or NULL.  normals4: n x 4 doubles or NULL.
 * Device layout: FP32 SoA -- float4 xyz1, symmetric covariance as float4 (c00 c01 c02 c11) + float2 (c12 c22), float4 normals. */
int glim_amd_cloud_create(glim_amd_ctx* ctx, int64_t n, const double* points4, const double* covs16, const double* normals4,
                          glim_amd_cloud** out);
/* same from compact FP32 arrays: xyz n x 3, cov33 n x 9 (row-major, symmetric) or NULL, normals3 n x 3 or NULL. */
int glim_amd_cloud_create_f32(glim_amd_ctx* ctx, int64_t n, const float* xyz, const float* cov33, const float* normals3,
                              glim_amd_cloud** out);
int glim_amd_cloud_destroy(glim_amd_cloud* cloud);
int glim_amd_cloud_size(const glim_amd_cloud* cloud, int64_t* n);
/* device bytes held (IntegratedVGICPFactorGPU::memory_usage_gpu accounting, viewer/standard_viewer_mem.cpp:52-56). */
int glim_amd_cloud_memory_usage(const glim_amd_cloud* cloud, size_t* bytes);
/* copy back (parity / debug): any pointer may be NULL.  xyz n x 3, cov33 n x 9, normals3 n x 3, neighbors n x k. */
int glim_amd_cloud_download(const glim_amd_cloud* cloud, float* xyz, float* cov33, float* normals3, int32_t* neighbors);

/* gtsam_points::PointCloud::save_compact(dir) / PointCloudCPU::load(dir) + clone, as SubMap::save / SubMap::load use them for a
 * submap's merged cloud (src/glim/mapping/sub_map.cpp:62, :142): FP32 files points_compact.bin (n x xyz), covs_compact.bin
 * (n x c00 c01 c02 c11 c12 c22), normals_compact.bin, times_compact.bin, intensities_compact.bin inside `dir` (which must exist).
 * load also accepts the full-precision points.bin / covs.bin / normals.bin (Vector4d / Matrix4d) when no compact files exist. */
int glim_amd_cloud_save_compact(const glim_amd_cloud* cloud, const char* dir);
int glim_amd_cloud_load_compact(glim_amd_ctx* ctx, const char* dir, glim_amd_cloud** out);

/* CloudDeskewing::deskew fused with the upload: src/glim/common/cloud_deskewing.cpp:11-53 (constant
 * velocity: n_imu == 0, linear_vel3 / angular_vel3, NULL = zero) and :55-133 (IMU poses: imu_times[n_imu], imu_poses12[n_imu x 12]
 * = T_world_imu row-major 3x4, `stamp` = scan start time), as called at src/glim/odometry/odometry_estimation_imu.cpp:313-316.
 * points4: n x Vector4d, times: n per-point offsets from the scan start (as the preprocessor leaves them: ascending), T_imu_lidar12:
 * extrinsic.
 * to_imu_frame != 0 fuses the step BOTH reference callers take next: every deskewed point is moved into the IMU frame,
 * `pt = T_imu_lidar * pt` (odometry_estimation_imu.cpp:314-316; sub_mapping.cpp:368-370 with T_lidar_imu.inverse()), as a second FP64
 * product with its own roundings, BEFORE the covariances are estimated (:320 / :374) -- so normals face the IMU-frame origin
 * (cloud_covariance_estimation.cpp:98-101) and every voxel map / factor built from the cloud lives in the IMU frame, as in GLIM.
 * to_imu_frame == 0 returns exactly CloudDeskewing::deskew's value (LiDAR frame).
 * The result is a device cloud of the deskewed points -- the exact FP64 values (what glim_amd_cloud_estimate_covariances reads and
 * glim_amd_cloud_download_frame returns) and their FP32 image for the factor path; no covariances yet. */
/* PointCloudGPU::clone of points only that KEEPS the exact FP64 values beside their FP32 image (what a preprocessed / deskewed cloud does): for
 * points that are not FP32-representable -- deskewed, IMU-frame points handed to CloudCovarianceEstimation::estimate by a caller that holds them on
 * the host (src/glim/odometry/odometry_estimation_imu.cpp:320; adapters/glim/cloud_covariance_estimation_hip.cpp) -- so that
 * glim_amd_cloud_estimate_covariances reads what the reference reads (the 1e-5 covariance gate is then met on every point). */
int glim_amd_cloud_create_exact(glim_amd_ctx* ctx, int64_t n, const double* points4, glim_amd_cloud** out);
int glim_amd_cloud_create_deskewed(glim_amd_ctx* ctx, int64_t n, const double* points4, const double* times, const double* T_imu_lidar12,
                                   int32_t n_imu, const double* imu_times, const double* imu_poses12, double stamp, const double* linear_vel3,
                                   const double* angular_vel3, int32_t to_imu_frame, glim_amd_cloud** out);

/* ---- scan preprocessing on device: CloudPreprocessor::preprocess_impl,
 * src/glim/preprocess/cloud_preprocessor.cpp:92-188 -- downsampling (gtsam_points::randomgrid_sampling / voxelgrid_sampling,
 * :104-109), range filter (:117-128), sort by time (:134-136), global shutter (:138-140), cropbox (:143-160), statistical outlier
 * removal (:162-164) and the kNN for the covariances (:183-184), without a host round trip between the stages. */
typedef struct glim_amd_preprocess_params { /* CloudPreprocessorParams, cloud_preprocessor.cpp:20-61; config/config_preprocess.json */
  double distance_near_thresh, distance_far_thresh;
  int32_t use_random_grid_downsampling;
  int32_t downsample_target; /* random_downsample_target: > 0 -> rate = target / n (:105) */
  double downsample_resolution, downsample_rate;
  int32_t global_shutter; /* config_sensors global_shutter_lidar (:24) */
  int32_t enable_outlier_removal, outlier_removal_k;
  double outlier_std_mul_factor;
  int32_t enable_cropbox_filter, crop_bbox_frame_imu; /* crop_bbox_frame == "imu" */
  double crop_bbox_min[3], crop_bbox_max[3];
  double T_imu_lidar[12]; /* row-major 3x4, used by the "imu" cropbox only */
  int32_t k_correspondences;
  int32_t voxelgrid_block_size; /* gtsam_points averages voxels inside blocks of 1024 sorted points; 0 = never split a voxel */
  uint64_t seed;                /* the reference draws from a std::mt19937 (:67); here: seed of the counter-based sampler */
} glim_amd_preprocess_params;
/* shipped defaults (config/config_preprocess.json) */
int glim_amd_preprocess_default_params(glim_amd_preprocess_params* params);
/* points4: n x Vector4d (RawPoints::points), times: n (RawPoints::times), intensities: n or NULL.  The result is a device
 * cloud holding the surviving points (FP32 for the factor path + the exact FP64 values), their times, intensities and -- when
 * k_correspondences > 0 -- their k nearest neighbours: everything PreprocessedFrame carries
 * (include/glim/preprocess/preprocessed_frame.hpp:26-39). */
int glim_amd_preprocess(glim_amd_ctx* ctx, int64_t n, const double* points4, const double* times, const double* intensities,
                        const glim_amd_preprocess_params* params, glim_amd_cloud** out);
/* PreprocessedFrame fields of a preprocessed cloud back on the host; any pointer may be NULL.  points4 n x 4 (w = 1), times n,
 * intensities n (GLIM_AMD_ERR_STATE if the scan had none), neighbors n x k. */
int glim_amd_cloud_download_frame(const glim_amd_cloud* cloud, double* points4, double* times, double* intensities, int32_t* neighbors);
/* CloudDeskewing::deskew (+ the IMU-frame step when to_imu_frame != 0) applied to a preprocessed cloud that is already on the device
 * (same arguments as glim_amd_cloud_create_deskewed).  The new cloud shares nothing with `pre`; the neighbour lists found on the raw scan
 * are carried over, as the reference does (odometry_estimation_imu.cpp:313-320: deskew, IMU frame, then covariances from raw_frame->neighbors). */
int glim_amd_cloud_deskew(const glim_amd_cloud* pre, const double* T_imu_lidar12, int32_t n_imu, const double* imu_times,
                          const double* imu_poses12, double stamp, const double* linear_vel3, const double* angular_vel3, int32_t to_imu_frame,
                          glim_amd_cloud** out);
/* ---- GICP factor on device: gtsam_points::IntegratedGICPFactor -- nearest-neighbour correspondences instead
 * of a voxel lookup -- as constructed at src/glim/mapping/sub_mapping.cpp:202 (between factors, one linearize, :203),
 * src/glim/mapping/global_mapping.cpp:400-402 (set_max_correspondence_distance(0.5), 10 LM iterations) and
 * src/glim/mapping/global_mapping_pose_graph.cpp:393-394 (loop validation; passes the target's pre-built tree). */
typedef struct glim_amd_nn_index glim_amd_nn_index; /* the target's search structure (gtsam_points::KdTree at global_mapping_pose_graph.cpp:393) */
/* Built once per target cloud (which needs covariances for the factor calls and must outlive the index), reused by every
 * linearisation.  max_correspondence_distance_hint sizes the grid cells: their edge h is chosen from the target's density between hint/3
 * and hint.  The ring walk is bounded at 64 cells: the calls below accept any distance up to 64 x 0.999999 x h -- every distance up to
 * 21 x hint for any target, up to just under 64 x hint for a sparse one -- and return GLIM_AMD_ERR_UNSUPPORTED beyond that (rebuild with
 * a larger hint).  The grid spans 2^20 cells either side of the origin on each axis: a target point outside it (a tiny hint, a far
 * point), like a non-finite one, is kept out of the index and is never a correspondence, and a transformed source point outside it has
 * none; every other answer is what it would be without those points. */
int glim_amd_nn_index_create(const glim_amd_cloud* target, double max_correspondence_distance_hint, glim_amd_nn_index** out);
int glim_amd_nn_index_destroy(glim_amd_nn_index* index);
/* IntegratedGICPFactor::linearize at T_target_source (flags: GLIM_AMD_FACTOR_BINARY fills the target-side blocks). */
int glim_amd_gicp_linearize(const glim_amd_nn_index* target, const glim_amd_cloud* source, const double* T_target_source12,
                            double max_correspondence_distance, uint32_t flags, glim_amd_linearized6* out);
/* IntegratedGICPFactor::error and ::inlier_fraction (num_inliers / source size) -- global_mapping_pose_graph.cpp:404-405. */
int glim_amd_gicp_error(const glim_amd_nn_index* target, const glim_amd_cloud* source, const double* T_target_source12,
                        double max_correspondence_distance, double* error, int64_t* num_inliers);
/* parity / debug: matched target index per source point, or -1.  The correspondences are the search's alone: clouds without covariances
 * (the ICP factors' case, below) are answered too. */
int glim_amd_gicp_correspondences(const glim_amd_nn_index* target, const glim_amd_cloud* source, const double* T_target_source12,
                                  double max_correspondence_distance, int32_t* correspondences);

/* ---- ICP factors on device: gtsam_points::IntegratedICPFactor (point-to-point) and IntegratedPointToPlaneICPFactor, the factor GLIM's manual
 * loop closing refines with when a cloud carries no covariances (src/glim/viewer/interactive/manual_loop_close_modal.cpp:485-490: LM capped at
 * 200 iterations; with covariances it takes the GICP factor, :476-483).  gtsam_points is not in the reference tree: the rule is upstream RECALL.
 *   p_i        the source cloud's FP32 coordinates;  q = T p_i in FP64, the GICP factor's own transform
 *   j          the exact nearest target point within max_correspondence_distance: the GICP factor's search over glim_amd_nn_index -- the same
 *              index, tie rule (the smaller index) and ring bound, so glim_amd_gicp_correspondences returns these correspondences
 *   r          b_j - q
 *   point-to-point   e = sum r^T r,  J_s = [R hat(p) | -R],  H_ss = sum J_s^T J_s,  b_s = sum J_s^T r
 *   point-to-plane   (GLIM_AMD_ICP_POINT_TO_PLANE) residual and Jacobian weighted ELEMENTWISE by the target normal n_j: r' = n_j o r,
 *              J' = diag(n_j) J_s, i.e. the metric diag(n_x^2, n_y^2, n_z^2) in the target frame (not n n^T): e = sum r'^T r',
 *              H_ss = sum J'^T J', b_s = sum J'^T r'.  GLIM itself calls only point-to-point.
 *   error      carries no 1/2, as the GICP factor's: with frozen correspondences d e / d xi = 2 b_s
 *   inliers    the matched points
 *   record     the 29-double compact record of the VGICP / GICP factors; glim_amd_expand_compact gives the binary blocks from it unchanged
 *   inputs     neither cloud needs covariances.  Point-to-plane needs the TARGET cloud's normals (read through the index, from the cloud the
 *              index was built over): GLIM_AMD_ERR_STATE without them.
 * flags: GLIM_AMD_FACTOR_BINARY and / or GLIM_AMD_ICP_POINT_TO_PLANE; any other bit: GLIM_AMD_ERR_INVALID.  Other errors as glim_amd_gicp_linearize
 * (GLIM_AMD_ERR_UNSUPPORTED: a distance beyond the index's ring walk).  An empty source or target gives the zero record. */
int glim_amd_icp_linearize(const glim_amd_nn_index* target, const glim_amd_cloud* source, const double* T_target_source12,
                           double max_correspondence_distance, uint32_t flags, glim_amd_linearized6* out);
/* IntegratedICPFactor::error and the inlier count at T_target_source (flags as above; GLIM_AMD_FACTOR_BINARY changes nothing here) */
int glim_amd_icp_error(const glim_amd_nn_index* target, const glim_amd_cloud* source, const double* T_target_source12,
                       double max_correspondence_distance, uint32_t flags, double* error, int64_t* num_inliers);

/* ---- continuous-time GICP factor on device: gtsam_points::IntegratedCT_GICPFactor_<PointCloud, PointCloud> (KdTree target), the whole
 * per-frame cost of GLIM's LiDAR-only CT odometry (src/glim/odometry/odometry_estimation_ct.cpp:158-183, config_odometry_ct.json).
 * One scan, two keys: X = the pose at scan begin, Y = at scan end.  Semantics (upstream recall, gicp.hip states them in full):
 *   time table, built once: source times in index order, a new bucket when t - table.back() > 1e-3, every entry / max(1e-9, table.back());
 *   bucket k: T_k = X * Exp(t_k * Log(X^-1 Y)), D0_k / D1_k = d T_k / d X, d T_k / d Y (right perturbations, FP64 on the host);
 *   point i of bucket k: q = T_k p_i, exact nearest target point within max_correspondence_distance (glim_amd_gicp_*'s search),
 *   M = (C_B + R_k C_A R_k^T)^-1, r = q - b, J = [-R_k hat(p) | R_k]: e += r^T M r, H_00 += (J D0)^T M (J D0), ... b_1 += (J D1)^T M r.
 * gtsam::HessianFactor(X, Y, H_00, H_01, -b_0, H_11, -b_1, error).  All H_* row-major 6x6, tangent [omega; v]. */
typedef struct glim_amd_ct_gicp_factor glim_amd_ct_gicp_factor; /* child of the target index's context */
typedef struct {
  int64_t num_inliers;
  double error;
  double H_00[36]; /* X-X */
  double H_01[36]; /* X-Y */
  double H_11[36]; /* Y-Y */
  double b_0[6];
  double b_1[6];
} glim_amd_ct_linearized;
/* IntegratedCT_GICPFactor(X, Y, target, source, target_tree) -- odometry_estimation_ct.cpp:158-160.  `target` needs covariances (checked
 * per call, as glim_amd_gicp_*); `source` needs covariances and per-point times: `times` (n, host, copied) or NULL = the times its
 * preprocessing kept (glim_amd_preprocess).  GLIM_AMD_ERR_STATE when either is missing.  Both the index and the source must outlive the
 * factor; max_correspondence_distance starts at 1.0. */
int glim_amd_ct_gicp_create(const glim_amd_nn_index* target, const glim_amd_cloud* source, const double* times, glim_amd_ct_gicp_factor** out);
int glim_amd_ct_gicp_destroy(glim_amd_ct_gicp_factor* factor);
/* set_max_correspondence_distance (config_odometry_ct.json max_correspondence_distance); GLIM_AMD_ERR_UNSUPPORTED beyond what the index was
 * sized for (the rule of glim_amd_gicp_*), the distance is then left unchanged. */
int glim_amd_ct_gicp_set_max_correspondence_distance(glim_amd_ct_gicp_factor* factor, double max_correspondence_distance);
/* linearize(values) -- called by LM at odometry_estimation_ct.cpp:176-183: correspondences and M are recomputed at (X, Y) and kept on the
 * device for error(). */
int glim_amd_ct_gicp_linearize(glim_amd_ct_gicp_factor* factor, const double* X12, const double* Y12, glim_amd_ct_linearized* out);
/* error(values) -- LM's cost evaluations (same call site): the correspondences and M kept by the last linearize (computed first at (X, Y)
 * when there was none).  num_inliers may be NULL. */
int glim_amd_ct_gicp_error(glim_amd_ct_gicp_factor* factor, const double* X12, const double* Y12, double* error, int64_t* num_inliers);
/* parity / debug: matched target index per source point at (X, Y), or -1 (the kept state is not touched). */
int glim_amd_ct_gicp_correspondences(glim_amd_ct_gicp_factor* factor, const double* X12, const double* Y12, int32_t* correspondences);
/* deskewed_source_points(values, local) -- odometry_estimation_ct.cpp:191: T_k p_i (n x Vector4d, w = 1), FP64 from the source's exact
 * points where it keeps them; local != 0: in the frame of T_0 (T_0^-1 T_k p_i). */
int glim_amd_ct_gicp_deskewed_points(glim_amd_ct_gicp_factor* factor, const double* X12, const double* Y12, int32_t local, double* points4);
/* the same points as a new device cloud (FP64 kept beside the FP32 image) carrying the source's neighbour lists: what :194-195 hands to
 * CloudCovarianceEstimation::estimate -- glim_amd_cloud_estimate_covariances runs on it directly. */
int glim_amd_ct_gicp_deskewed_cloud(glim_amd_ct_gicp_factor* factor, const double* X12, const double* Y12, int32_t local, glim_amd_cloud** out);

/* ---- device iVox: gtsam_points::IncrementalVoxelMap<FlatContainer> (gtsam_points::iVox), the incremental target model of the LiDAR-only
 * continuous-time odometry (src/glim/odometry/odometry_estimation_ct.cpp:56-63 creates it, :158-162 builds the frame's factor on it, :229-235
 * inserts every finished frame); also the target of the "GICP" branch of odometry_estimation_cpu.cpp, of loose_initial_state_estimation.cpp and
 * of the manual loop-close tool.  gtsam_points is not under the reference tree: the semantics below are upstream recall (DESIGN.md lists the
 * guesses).
 *   voxel of a point: floor(p * (1 / leaf)) per axis, FP64, on the STORED point.
 *   insert(cloud): points in input order.  A point whose voxel does not exist creates it (new voxels are appended in first-seen order); the
 *     voxel's lru becomes the current counter; FlatContainer::add drops the point when the cell already holds max_points_in_cell points, or
 *     when a point already in the cell -- one accepted earlier in the same call included -- is closer than min_dist_in_cell (squared distance
 *     < min_dist^2, strict; FP64 (dx^2 + dy^2) + dz^2 with separate roundings); otherwise the point is appended with its covariance.  After
 *     all points: if (++lru_counter % lru_clear_cycle == 0) every voxel with lru + lru_horizon < lru_counter is removed, survivors keep
 *     their order.
 *   nearest neighbour of q: from the voxel c of q visit c + offset for the offsets of the neighbour mode -- 1: {0}; 7: the centre, then +x -x
 *     +y -y +z -z; 19: those, then the twelve edges (+-1,+-1,0), (+-1,0,+-1), (0,+-1,+-1), first sign slower; 27: the full cube, z outermost
 *     and x innermost -- and keep the smallest FP64 squared distance (same form); a later candidate replaces the best only when strictly
 *     smaller; valid iff d^2 <= max_correspondence_distance^2.  NOT an exact search: points outside the visited voxels are never seen.
 *   defaults: min_dist_in_cell 0.1, max_points_in_cell 20, lru_horizon 10, lru_clear_cycle 10, neighbour mode 7.
 * Storage (this library's choice): FP32 points and six-float covariances, like every device cloud.  Insert with a pose computes
 * x' = ((R00 x + R01 y) + R02 z) + tx in FP64 with separate roundings (likewise y', z'), rounds to FP32, and C' = R C R^T in FP32; the voxel
 * and the min_dist test use the stored value.  Normals are not stored.  Non-finite points and points outside the +-2^20-voxel key range are
 * skipped.  Every call returns with the map's work finished: `num_voxels` / `num_points` are on the host and any later reader sees the map.
 * The map is a child of its context; a map with a live continuous-time factor on it refuses to be destroyed (GLIM_AMD_ERR_STATE). */
typedef struct glim_amd_ivox glim_amd_ivox;
int glim_amd_ivox_create(glim_amd_ctx* ctx, double leaf_size, glim_amd_ivox** out);
int glim_amd_ivox_destroy(glim_amd_ivox* ivox);
/* voxel_insertion_setting(): max_points_in_cell in 1..64 (a cell never holds more than one wavefront's lanes).  GLIM_AMD_ERR_STATE once the
 * map has been inserted into. */
int glim_amd_ivox_set_insertion(glim_amd_ivox* ivox, double min_dist_in_cell, int32_t max_points_in_cell);
/* set_lru_horizon / set_lru_clear_cycle (horizon >= 0, clear_cycle >= 1) */
int glim_amd_ivox_set_lru(glim_amd_ivox* ivox, int32_t horizon, int32_t clear_cycle);
/* set_neighbor_voxel_mode: 1 | 7 | 19 | 27 */
int glim_amd_ivox_set_neighbor_voxel_mode(glim_amd_ivox* ivox, int32_t mode);
/* insert(*frame) with the host transform loop of odometry_estimation_ct.cpp:230-234 fused in: T_world_cloud12 moves points and covariances
 * (NULL = identity: values are stored as they are).  The cloud needs covariances (GLIM_AMD_ERR_STATE). */
int glim_amd_ivox_insert(glim_amd_ivox* ivox, const glim_amd_cloud* cloud, const double* T_world_cloud12);
int glim_amd_ivox_info(const glim_amd_ivox* ivox, int32_t* num_voxels, int64_t* num_points, int32_t* lru_counter, double* leaf_size);
/* copy back in slot (= upstream's voxel) order; cap = max_points_in_cell.  coords V x 3, counts V, points V x cap x 3, covs V x cap x 9
 * (places beyond a voxel's count are zero).  Any may be NULL. */
int glim_amd_ivox_download(const glim_amd_ivox* ivox, int32_t* coords, int32_t* counts, float* points, float* covs);
/* voxel_points() (odometry_estimation_ct.cpp:302): num_points x Vector4d, voxels in slot order, points in cell order. */
int glim_amd_ivox_voxel_points(const glim_amd_ivox* ivox, double* points4);
/* IntegratedGICPFactor_<iVox, PointCloud>: the glim_amd_gicp_* trio over the map.  Any finite max_correspondence_distance is accepted (the
 * search is bounded by the neighbour mode, not by the radius).  correspondences: slot * max_points_in_cell + place in the cell, or -1. */
int glim_amd_ivox_gicp_linearize(const glim_amd_ivox* target, const glim_amd_cloud* source, const double* T_target_source12,
                                 double max_correspondence_distance, uint32_t flags, glim_amd_linearized6* out);
int glim_amd_ivox_gicp_error(const glim_amd_ivox* target, const glim_amd_cloud* source, const double* T_target_source12,
                             double max_correspondence_distance, double* error, int64_t* num_inliers);
int glim_amd_ivox_gicp_correspondences(const glim_amd_ivox* target, const glim_amd_cloud* source, const double* T_target_source12,
                                       double max_correspondence_distance, int64_t* correspondences);
/* IntegratedCT_GICPFactor_<iVox, PointCloud>(X, Y, target_ivox, frame, target_ivox) -- odometry_estimation_ct.cpp:158-162.  The handle is the
 * continuous-time factor's: linearize, error, set_max_correspondence_distance (any distance), deskewed_points, deskewed_cloud and destroy
 * above work on it unchanged, and its correspondences call writes slot * max_points_in_cell + place (always below 2^31: the map refuses to
 * grow beyond that) or -1.  The factor reads the map as it is at each call; an insert after linearize invalidates the kept correspondences
 * and M (error then recomputes them first).  The map must outlive the factor: glim_amd_ivox_destroy refuses while the factor lives. */
int glim_amd_ivox_ct_factor_create(glim_amd_ivox* target, const glim_amd_cloud* source, const double* times, glim_amd_ct_gicp_factor** out);

/* ---- submap merge on device: gtsam_points::merge_frames(poses, frames, downsample_resolution, target_num_points)
 * as called at src/glim/mapping/sub_mapping.cpp:480-497 (the reference's own GPU variant, merge_frames_gpu, is commented out at :491).
 * Frame f (sizes[f] points: points4[f] n x Vector4d, covs16[f] n x column-major Matrix4d) is moved by poses12[f] (row-major 3x4
 * T_origin_frame): p' = T p, C' = R C R^T; the concatenation is voxel-grid averaged (points and covariances) at
 * `downsample_resolution`; when target_num_points > 0 and more points remain, a uniform random sample of that size is kept
 * (same meaning as sub_mapping_passthrough.cpp:149-151).  The result is a device cloud with covariances, ready for
 * GaussianVoxelMapGPU::insert / the factors (global_mapping.cpp:253-266); voxelgrid_block_size: see glim_amd_preprocess_params. */
int glim_amd_merge_frames(glim_amd_ctx* ctx, int32_t num_frames, const double* poses12, const double* const* points4, const double* const* covs16,
                          const int64_t* sizes, double downsample_resolution, int32_t target_num_points, int32_t voxelgrid_block_size, uint64_t seed,
                          glim_amd_cloud** out);
/* the merged submap back on the host as gtsam_points::PointCloudCPU holds it: points4 n x Vector4d, covs16 n x Matrix4d (exact FP64). */
int glim_amd_cloud_download_merged(const glim_amd_cloud* cloud, double* points4, double* covs16);

/* kNN on device: CloudPreprocessor::find_neighbors (src/glim/preprocess/cloud_preprocessor.cpp:190-221).
 * k nearest among all points including the query itself, ascending (distance, index); fewer than k points -> the tail is 0 (what the
 * reference's zero-initialised result vector holds there, cloud_preprocessor.cpp:193, :200).
 * Result stays on the device inside the cloud (and is copied to neighbors_out, n x k, when not NULL). */
int glim_amd_cloud_find_neighbors(glim_amd_cloud* cloud, int k, int32_t* neighbors_out);
/* upload caller-provided neighbours (n x k) instead; GLIM_AMD_ERR_INVALID if any index is outside [0, n). */
int glim_amd_cloud_set_neighbors(glim_amd_cloud* cloud, int k, const int32_t* neighbors);
/* CloudCovarianceEstimation::estimate (src/glim/common/cloud_covariance_estimation.cpp:43-122, PLANE regularisation :181-196):
 * fills the cloud's covariances and sensor-facing normals from the first k_neighbors stored neighbours. */
int glim_amd_cloud_estimate_covariances(glim_amd_cloud* cloud, int k_neighbors);

/* ---- Gaussian voxel maps: GaussianVoxelMapGPU(resolution, ...) + insert(frame)
 *      (odometry_estimation_gpu.cpp:103-104, sub_mapping.cpp:398-399, global_mapping.cpp:265-266,747-748) ------------ */
/* The reference's init_num_buckets / max_bucket_scan_count / target_points_drop_rate are accepted for signature
 * compatibility and ignored: this build is lossless (every point is inserted).
 *
 * Points that do not fit.  A voxel coordinate is fast_floor(x / resolution) and lives in [-2^20, 2^20) per axis (the 21-bit key fields).  A
 * point DOES NOT FIT when a coordinate is NaN, +-Inf, or a finite value whose voxel coordinate lies outside that range -- decided on the FP64
 * product before anything is converted to an integer.  One rule, two sides:
 *   target side (every way of putting points into a voxel map: glim_amd_voxelmap_insert into an empty or a populated map, with or without an
 *     LRU horizon, and glim_amd_frame_create): a point that does not fit makes the call return GLIM_AMD_ERR_RANGE; the map is left as it was
 *     (glim_amd_frame_create creates nothing);
 *   source side (every evaluation that transforms a cloud's points into a map: the factor-set calls, glim_amd_overlap*, the alignment loops
 *     over voxel-map targets): a point whose IMAGE under the pose does not fit -- because the point itself is NaN, +-Inf or huge, or because
 *     the pose carries it out of range -- has no correspondence: it is an outlier, it is not counted, and it contributes exactly nothing to
 *     any sum (a record equals, bit for bit, that of the same cloud with a far-away finite point in its place).
 * Non-finite covariances or normals of a finite point are outside this rule: the caller keeps them finite. */
int glim_amd_voxelmap_create(glim_amd_ctx* ctx, double resolution, int init_num_buckets, int max_bucket_scan_count,
                             double target_points_drop_rate, glim_amd_voxelmap** out);
/* build from a cloud that has covariances.  Voxel = mean of member means, mean of member covariances.  A second insert into the same map
 * adds its points to the voxels already there (GaussianVoxelMapCPU semantics: odometry_estimation_cpu.cpp:66-67,189); the map is rebuilt, so
 * GLIM's GPU callers, which insert once per map, pay nothing for it.
 * DEVIATION (unverified, gtsam_points is not under the reference tree): upstream's GaussianVoxelMapGPU::insert is believed to REBUILD the table
 * from the new frame only.  Every GPU call site of the reference inserts exactly once per map (odometry_estimation_gpu.cpp:103-104,
 * sub_mapping.cpp:398-399, global_mapping.cpp:265-266,747-748), so both semantics give the same map there; a port that re-inserts into a GPU map
 * and wants upstream's behaviour creates a new map per frame instead.  The re-opened voxels pass through their FP32 records (mean * n,
 * cov * n), i.e. each further insert adds a rounding of 1 FP32 ulp to the old voxels' statistics
 * (tests/test_gpu_parity.py::test_voxelmap_incremental_insert_matches_oracle bounds it against the FP64 oracle's merged map). */
int glim_amd_voxelmap_insert(glim_amd_voxelmap* vmap, const glim_amd_cloud* cloud);
/* create_frame of the GPU odometry as ONE submission (src/glim/odometry/odometry_estimation_gpu.cpp:86-107): PointCloudGPU::clone of a frame that
 * arrives with CPU covariances (+ normals) and GaussianVoxelMapGPU(resolutions[lv]).insert(frame) for lv < num_levels (<= 8; voxelmap_levels, 2 in the
 * shipped configuration) are enqueued back to back and the host synchronises once.  Same arguments as glim_amd_cloud_create; the results are what the
 * separate calls return (same bits), *cloud and maps[lv] are owned by the caller.  On failure nothing is created. */
int glim_amd_frame_create(glim_amd_ctx* ctx, int64_t n, const double* points4, const double* covs16, const double* normals4, int32_t num_levels,
                          const double* resolutions, glim_amd_cloud** cloud, glim_amd_voxelmap** maps);
int glim_amd_voxelmap_destroy(glim_amd_voxelmap* vmap);
/* GaussianVoxelMapCPU::set_lru_horizon of the CPU odometry's incremental target map (src/glim/odometry/odometry_estimation_cpu.cpp:63-68,
 * update_target :177-191; config_odometry_cpu.json "lru_thresh": 100): every insert carries a counter; every `lru_clear_cycle` inserts (<= 0: 10,
 * gtsam_points' default) the voxels that no insert has touched for more than `lru_horizon` inserts are dropped.  lru_horizon <= 0 (the default):
 * no eviction -- the GPU callers of the reference never set one.  Applies to the inserts that follow. */
int glim_amd_voxelmap_set_lru_horizon(glim_amd_voxelmap* vmap, int32_t lru_horizon, int32_t lru_clear_cycle);
/* VoxelMapInfo (standard_viewer_mem.cpp:76-77): num_voxels, num_buckets, resolution, device bytes. */
int glim_amd_voxelmap_info(const glim_amd_voxelmap* vmap, int32_t* num_voxels, int32_t* num_buckets, double* resolution,
                           size_t* bytes);
/* copy back all voxels (unspecified order): coords V x 3, counts V, means V x 3, cov33 V x 9.  Any may be NULL. */
int glim_amd_voxelmap_download(const glim_amd_voxelmap* vmap, int32_t* coords, int32_t* counts, float* means, float* cov33);

/* ---- factor sets: NonlinearFactorSetGPU of IntegratedVGICPFactorGPU
 *      (odometry_estimation_gpu.cpp:144,161,383-386; sub_mapping.cpp:307; global_mapping.cpp:335,466,860) ------------- */
int glim_amd_factor_set_create(glim_amd_ctx* ctx, glim_amd_factor_set** out);
int glim_amd_factor_set_destroy(glim_amd_factor_set* set);
/* add IntegratedVGICPFactorGPU(target voxel map, source cloud).  The set borrows both handles; keep them alive.  A source point whose image
 * does not fit the key range (NaN, +-Inf, beyond 2^20 voxels: "Points that do not fit" above) is an outlier in every call below. */
int glim_amd_factor_set_add(glim_amd_factor_set* set, const glim_amd_voxelmap* target, const glim_amd_cloud* source, uint32_t flags,
                            int32_t* factor_index);
int glim_amd_factor_set_clear(glim_amd_factor_set* set);
int glim_amd_factor_set_size(const glim_amd_factor_set* set, int32_t* n);
/* NonlinearFactorSetGPU::linearize: one fused launch over every factor (+ a tiny FP64 finalise), one upload of the
 * poses, one download of the results.  T_target_source: n x 12.  out: n records. */
int glim_amd_factor_set_linearize(glim_amd_factor_set* set, const double* T_target_source, glim_amd_linearized6* out);
/* NonlinearFactorSetGPU::error.  T_lin == NULL: correspondences recomputed at T_eval (CPU-factor semantics, the parity
 * default); otherwise correspondences and Mahalanobis matrices frozen at T_lin (GPU-factor semantics).  errors: n; inliers: n or NULL. */
int glim_amd_factor_set_error(glim_amd_factor_set* set, const double* T_lin, const double* T_eval, double* errors, int64_t* inliers);
/* correspondences of one factor at a pose (parity/debug): corr n_points x 4 int32 = {cx, cy, cz, hit ? 1 : -1}; a point whose image does
 * not fit the key range has no voxel coordinate: {INT32_MIN, INT32_MIN, INT32_MIN, -1}. */
int glim_amd_factor_set_correspondences(glim_amd_factor_set* set, int32_t factor_index, const double* T_target_source, int32_t* corr);

/* Device-resident variant for multi-GPU cost evaluation and benchmarking: results are left on the device in
 * `out_device` (n x GLIM_AMD_COMPACT_DOUBLES doubles, caller-owned device memory, e.g. a torch tensor) without a host
 * round trip; the launch is asynchronous on the context stream.  Compact record: [num_inliers, error, 21 upper-triangular
 * entries of H_ss (row-major), 6 of b_s]; glim_amd_expand_compact turns records into glim_amd_linearized6 on the host. */
#define GLIM_AMD_COMPACT_DOUBLES 29
int glim_amd_factor_set_linearize_device_async(glim_amd_factor_set* set, const double* T_target_source_host, double* out_device,
                                               int64_t out_row_offset);
int glim_amd_expand_compact(const double* compact, const double* T_target_source, uint32_t flags, glim_amd_linearized6* out);

/* ---- multi-device cost evaluation (BASELINE.json configs[3]; no counterpart in the reference, which is single-device:
 *      src/glim/mapping/global_mapping.cpp:110 one StreamTempBufferRoundRobin(64), :430-484 create_matching_cost_factors) -------------
 * One process, N devices: a context + a host thread + an RCCL communicator (ncclCommInitAll; librccl is dlopen'ed on first use) per
 * device (device 0 is driven by the CALLING thread).  Clouds and voxel maps are replicated on every device, the factor list is sharded into
 * contiguous cost-balanced chunks, every device linearises its chunk -- in a few pieces, so that the ncclAllGather of one piece's 29-double
 * compact records travels over xGMI (and this device's own rows to the host over its own PCIe link) while the next piece's kernels run --
 * and the records are expanded on the host in the original factor order.  One hand-over to the devices' threads per evaluation.  All
 * calls are synchronous and must come from one host thread at a time.
 * Who reads what: the HOST optimiser (GLIM's ISAM2 / LM, global_mapping.cpp:501) gets every record through a second store of the finalising
 * kernels into one pinned host array, so a call returns when the kernels are done; the all-gather completes the DEVICE-resident copy of the
 * record array on every device for device-side consumers (glim_amd_multi_gathered_device) and finishes behind the call
 * (glim_amd_multi_set_gather_mode). */
typedef struct glim_amd_multi glim_amd_multi;
/* devices: distinct HIP device ordinals.  A multi-device handle without a working RCCL is refused (GLIM_AMD_ERR_HIP) rather than
 * silently gathering over PCIe; a single device works either way (GLIM_AMD_DIAG="multi_rccl=0" skips the collective there).  (Test boxes with one
 * GPU run the N > 1 path over "virtual devices" -- one ordinal listed several times -- only when GLIM_AMD_DIAG holds multi_virtual=1:
 * glim_amd_diag.h.) */
int glim_amd_multi_create(const int32_t* devices, int32_t num_devices, glim_amd_multi** out);
int glim_amd_multi_destroy(glim_amd_multi* multi);
int glim_amd_multi_info(const glim_amd_multi* multi, int32_t* num_devices, int32_t* uses_rccl, int64_t* num_factors);
/* replicated PointCloudGPU::clone (same arguments as glim_amd_cloud_create / _f32); cloud_id indexes the replicas */
int glim_amd_multi_add_cloud(glim_amd_multi* multi, int64_t n, const double* points4, const double* covs16, const double* normals4, int32_t* cloud_id);
int glim_amd_multi_add_cloud_f32(glim_amd_multi* multi, int64_t n, const float* xyz, const float* cov33, const float* normals3, int32_t* cloud_id);
/* kNN (k) + CloudCovarianceEstimation on every replica (deterministic kernels: the replicas stay bit-identical) */
int glim_amd_multi_cloud_estimate_covariances(glim_amd_multi* multi, int32_t cloud_id, int k);
/* replicated GaussianVoxelMapGPU(resolution).insert(cloud) */
int glim_amd_multi_add_voxelmap(glim_amd_multi* multi, int32_t cloud_id, double resolution, int32_t* map_id);
/* the factor list: factor f = IntegratedVGICPFactorGPU(maps[target_map_ids[f]], clouds[source_cloud_ids[f]]), flags[f] (NULL = unary);
 * replaces the previous list and shards it over the devices (cost of a factor = its source points). */
int glim_amd_multi_set_factors(glim_amd_multi* multi, int64_t num_factors, const int32_t* target_map_ids, const int32_t* source_cloud_ids,
                               const uint32_t* flags);
/* device d owns factors [bounds[d], bounds[d + 1]); bounds has num_devices + 1 entries */
int glim_amd_multi_shard(const glim_amd_multi* multi, int64_t* bounds);
/* H / b / error of every factor at T_target_source (n x 12); out (n records) and total_error may be NULL.  With out == NULL the compact
 * records stay in the handle's pinned host array (glim_amd_multi_records) and total_error is summed by the devices. */
int glim_amd_multi_linearize(glim_amd_multi* multi, const double* T_target_source, glim_amd_linearized6* out, double* total_error);
/* the last evaluation's compact 29-double records [num_inliers, error, 21 upper-triangular H_ss entries, 6 b_s] of factors
 * [first, first + count), in factor order (expand one with glim_amd_expand_compact) */
int glim_amd_multi_records(const glim_amd_multi* multi, int64_t first, int64_t count, double* compact29);
/* The exchange of an evaluation: 1 (default) = enqueued behind every piece, NOT waited for by glim_amd_multi_linearize (the next evaluation's
 * kernels wait for it on the device before they overwrite their send slots; glim_amd_multi_gathered_device / _wait_gather wait on the host);
 * 2 = the call returns only when every device holds every record (the form of versions <= 0.1.0 r5); 0 = no exchange at all (host records only). */
int glim_amd_multi_set_gather_mode(glim_amd_multi* multi, int32_t mode);
/* host wait for the last evaluation's exchange on every device (no-op when none is pending) */
int glim_amd_multi_wait_gather(glim_amd_multi* multi);
/* The consumer side of the all-gather: the device-resident record array of device `device` (an index into the handle's device list), complete on
 * return -- *gathered points at num_devices x max_rows records of GLIM_AMD_COMPACT_DOUBLES doubles in DEVICE memory (valid until the next
 * glim_amd_multi_set_factors / destroy; overwritten by the next evaluation), *rows (may be NULL) = num_devices x max_rows; factor f of the list sits at
 * the row glim_amd_shard_layout gives for it.  An on-device consumer (cost, gradient or a whole optimiser step built from every factor's blocks)
 * reads it from any stream of that device without a host trip. */
int glim_amd_multi_gathered_device(glim_amd_multi* multi, int32_t device, const double** gathered, int64_t* rows);
/* the sharding rule as a pure host function (no device needed): contiguous chunks whose cumulative cost is nearest to r / world of the total */
int glim_amd_shard_bounds(const double* costs, int64_t n, int32_t world, int64_t* bounds);
/* where every factor's 29-double record sits in the gathered [world x max_rows] array of an evaluation, as a pure host function (the rule
 * glim_amd_multi_linearize, its collectives and glim_amd_multi_records use): bounds from glim_amd_shard_bounds (world + 1 entries),
 * split_mode as glim_amd_multi_set_split; rows (bounds[world] entries, may be NULL) receives each factor's row, the other outputs (may be
 * NULL) the padded shard length, the number of pieces a shard is cut into and the rows of a full piece.  Piece p of every shard forms one
 * contiguous region of world equal slots -- one in-place ncclAllGather each. */
int glim_amd_shard_layout(const int64_t* bounds, int32_t world, int32_t split_mode, int64_t* rows, int64_t* max_rows, int32_t* pieces, int64_t* piece_rows);

/* ---- overlap: overlap_gpu / overlap_auto (odometry_estimation_gpu.cpp:231,248,265,279,326; sub_mapping.cpp:252-253;
 *      global_mapping.cpp:322,448).  Fraction of source points that hit an occupied voxel of ANY target under its delta; a point whose
 *      image does not fit the key range ("Points that do not fit", voxel maps) hits none and stays in the denominator. */
int glim_amd_overlap(glim_amd_ctx* ctx, int32_t num_targets, const glim_amd_voxelmap* const* targets, const double* T_target_source,
                     const glim_amd_cloud* source, double* overlap);
/* num_queries overlap_gpu calls answered by ONE launch -- the keyframe loops of odometry_estimation_gpu.cpp:262-281 issue up to
 * max_num_keyframes of them back to back.  Query q: num_targets[q] (map, delta) pairs, stored consecutively in `targets` /
 * `T_target_source` (12 doubles each) in query order, against sources[q]; overlaps[q] receives the fraction.  At most 1024 queries. */
int glim_amd_overlap_batch(glim_amd_ctx* ctx, int32_t num_queries, const int32_t* num_targets, const glim_amd_voxelmap* const* targets,
                           const double* T_target_source, const glim_amd_cloud* const* sources, double* overlaps);

/* ---- FPFH: gtsam_points::estimate_fpfh and the nearest-descriptor queries of global registration
 *      (viewer/interactive/manual_loop_close_modal.cpp:376-463: estimate_fpfh on both clouds, KdTreeX<FPFH_DIM> over the 33-D descriptors,
 *      RANSAC / GNC on nearest-descriptor correspondences).  RANSAC and GNC are the two sections after this one; both consume the
 *      correspondence list glim_amd_fpfh_match returns, on the device.
 * The descriptor follows PCL's FPFHEstimation, which gtsam_points follows as far as recalled; the gtsam_points source is not in the
 * reference tree, so the points below that PCL leaves open are guesses (listed as such in DESIGN.md 4.7):
 *   neighbours   N(i) = { j : 0 < d2_ij <= r^2 }, d2 = (dx^2 + dy^2) + dz^2 in FP64 from the cloud's FP32 coordinates (zero-distance pairs,
 *                the point itself among them, are skipped; no cap on the neighbour count).  k = |N(i)|.
 *   pair (i, j)  FP64 throughout.  dp = p_j - p_i, f4 = |dp|, a1 = n_i.dp / f4, a2 = n_j.dp / f4.  If |a1| < |a2| the roles swap:
 *                n1 = n_j, n2 = n_i, dp = -dp, f3 = -a2; otherwise n1 = n_i, n2 = n_j, f3 = a1.  v = dp x n1; a pair with |v| = 0 is skipped
 *                (it still counts in k, as in PCL); v /= |v|, w = n1 x v, f2 = v.n2, f1 = atan2(w.n2, n1.n2).
 *                bins b1 = floor(11 (f1 + pi) / (2 pi)), b2 = floor(11 (f2 + 1) / 2), b3 = floor(11 (f3 + 1) / 2), each clamped to 0..10.
 *   SPFH         S_i = 33 counts over N(i) (bins 0..10 by b1, 11..21 by b2, 22..32 by b3), each count * 100 / k; all zero when k = 0.
 *   FPFH         F_i = sum over j in N(i) of S_j * (1 / d2_ij), accumulated in FP64 (the query's own SPFH is not added); each 11-bin block is
 *                then rescaled to sum 100 unless its sum is 0; ONE rounding to FP32.
 * A point with a non-finite coordinate has no neighbours and is nobody's neighbour: its row is all zero.
 * Deterministic: two calls on the same cloud return the same bits (fixed candidate order, fixed reduction tree, no floating-point atomics). */
typedef struct glim_amd_fpfh glim_amd_fpfh; /* n x 33 FP32 descriptors on the device; a child of the cloud's context */
/* GLIM_AMD_ERR_STATE: the cloud has no normals.  GLIM_AMD_ERR_INVALID: search_radius is NaN, infinite or <= 0. */
int glim_amd_fpfh_estimate(const glim_amd_cloud* cloud, double search_radius, glim_amd_fpfh** out);
int glim_amd_fpfh_destroy(glim_amd_fpfh* fpfh);
int glim_amd_fpfh_size(const glim_amd_fpfh* fpfh, int64_t* n);
/* descriptors33: n x 33 floats, row i = point i of the cloud */
int glim_amd_fpfh_download(const glim_amd_fpfh* fpfh, float* descriptors33);
/* Nearest target descriptor of every source descriptor (the KdTreeX<FPFH_DIM> knn_search(k = 1) loop).  nearest[i] (source size, may be NULL)
 * = index of the target descriptor with the smallest squared L2 distance, ties to the smaller index; sqdist[i] (may be NULL) = that distance.
 * FP32 arithmetic: d = (|a|^2 + |b|^2) - 2 a.b, clamped at 0, every sum one FMA chain over the 33 bins in order; error bound
 * 36 * 2^-24 * (|a|^2 + |b|^2).  GLIM_AMD_FPFH_RECIPROCAL: nearest[i] becomes -1 unless source i is also the nearest source descriptor of
 * target nearest[i] (same rule, same arithmetic -- GNC's reciprocal_check); sqdist[i] stays the forward distance.  An empty target gives
 * nearest = -1 and sqdist = +infinity.  Both handles must belong to one context (GLIM_AMD_ERR_INVALID otherwise). */
#define GLIM_AMD_FPFH_RECIPROCAL 0x1
int glim_amd_fpfh_match(const glim_amd_fpfh* target, const glim_amd_fpfh* source, uint32_t flags, int32_t* nearest, float* sqdist);

/* Descriptors that are already on the host (n x 33 floats, row i = point i) as a device object of context `ctx`; the row's squared norm the
 * matcher reads is filled in exactly as glim_amd_fpfh_estimate fills it (the same FP32 FMA chain), so matching an uploaded set and matching the
 * set it was downloaded from give the same bits. */
int glim_amd_fpfh_create(glim_amd_ctx* ctx, int64_t n, const float* descriptors33, glim_amd_fpfh** out);

/* ---- RANSAC: gtsam_points::estimate_pose_ransac, the global registration of viewer/interactive/manual_loop_close_modal.cpp:431-443
 *      (target, source, their FPFH descriptors, two search trees, RANSACParams{max_iterations 5000, early_stop_inlier_rate 0.9,
 *      inlier_voxel_resolution 1.0, dof 4 | 6, seed}).  The other estimator of that switch, GNC, is the section after this one.
 * The gtsam_points source is not in the reference tree: what follows is a restatement from recall plus decisions (listed in DESIGN.md 4.7a).
 *   inputs       target and source device clouds (points only), nearest[i] = matched target point of source point i or -1, the parameters.
 *   occupancy    the set of voxel coordinates fast_floor(p * (1 / res)) of every target point: FP64 product of the FP32 coordinate, 21 bits per
 *                axis, range [-2^20, 2^20).  A target point outside the range or not finite is simply absent.
 *   hypothesis   `it` (0-based), independent of every other:
 *     draw       s_k = splitmix64(seed, 3 it + k) mod N_source, k = 0 1 2 (the counter-based generator of glim_amd_preprocess, in place of the
 *                reference's sequential std::mt19937); t_k = nearest[s_k].
 *     status     the first that applies; only 0 is scored:
 *                1  some t_k < 0
 *                2  two equal s_k or two equal t_k
 *                3  edge lengths: for the edges (0,1), (1,2), (2,0), d_s = |s_a - s_b| and d_t = |t_a - t_b| in FP64, (dx^2 + dy^2) + dz^2 under
 *                   the root; rejected unless min(d_s, d_t) >= (1 - poly_error_thresh) * max(d_s, d_t).  The rule is stated for finite
 *                   lengths: a sample with a non-finite coordinate has status 4, not 3.
 *                4  a sampled point is not finite, or the centred source triangle is collinear: sigma_1 = 0 or sigma_2 < 1e-6 sigma_1.
 *     pose       least-squares rigid transform of the three pairs in FP64.  dof 6: Horn's quaternion form, the eigenvector of the largest
 *                eigenvalue of the 4 x 4 symmetric matrix by cyclic Jacobi with a fixed sweep count.  dof 4: the rotation about z by
 *                yaw = atan2(sum(x_s y_t - y_s x_t), sum(x_s x_t + y_s y_t)) over the centred pairs (formed as (cos, sin) = (C, S) / |(C, S)|),
 *                translation from the centroids, z included.  One function for host and device: glim_amd/csrc/ransac_pose.hpp.
 *     score      inliers(it) = number of finite source points p whose q = R p + t, in FP64 as nine FMAs,
 *                  q_r = fma(T[4r], p_x, fma(T[4r+1], p_y, fma(T[4r+2], p_z, T[4r+3]))),     r = 0 1 2
 *                has fast_floor(q * (1 / res)) in the occupancy set; a q outside the key range is no inlier.
 *   result       the sequential loop's, whatever the batching on the device: stop = the smallest `it` of status 0 with
 *                inliers(it) >= early_stop_inlier_rate * N_source; if there is one, that hypothesis, iterations_run = stop + 1; otherwise the
 *                status-0 hypothesis with the largest count over all max_iterations, the smallest `it` among equals, iterations_run =
 *                max_iterations.  No status-0 hypothesis: the identity, inlier_rate 0, best_iteration -1.  inlier_rate = inliers / N_source.
 * Deterministic: the same inputs and seed return the same bits in any context (integer counts, integer atomics only). */
typedef struct {
  int32_t max_iterations;
  double early_stop_inlier_rate;
  double poly_error_thresh;
  double inlier_voxel_resolution;
  int32_t dof; /* 4 or 6 */
  uint64_t seed;
} glim_amd_ransac_params;
typedef struct {
  double T_target_source[12];
  double inlier_rate;
  int64_t num_inliers;
  int32_t best_iteration; /* -1: no hypothesis passed the checks */
  int32_t iterations_run;
} glim_amd_registration_result;
/* the modal's defaults: 5000, 0.9, poly_error_thresh 0.5, 1.0, dof 6, seed 0 */
int glim_amd_ransac_default_params(glim_amd_ransac_params* params);
/* nearest: host array, one entry per source point.  GLIM_AMD_ERR_INVALID: a NULL argument, clouds of two contexts, dof not 4 or 6,
 * max_iterations <= 0, inlier_voxel_resolution not finite or <= 0, a NaN early_stop_inlier_rate or poly_error_thresh, a nearest value < -1 or
 * >= the target size.  A source of fewer than 3 points or an empty target is no error: the "no status-0 hypothesis" result. */
int glim_amd_ransac_align(const glim_amd_cloud* target, const glim_amd_cloud* source, const int32_t* nearest, const glim_amd_ransac_params* params,
                          glim_amd_registration_result* result);
/* The same with the correspondences of glim_amd_fpfh_match(target_fpfh, source_fpfh, match_flags) found on the device: `nearest` never visits
 * the host.  match_flags: 0 or GLIM_AMD_FPFH_RECIPROCAL.  GLIM_AMD_ERR_INVALID also when a descriptor set is not the size of its cloud or
 * belongs to another context. */
int glim_amd_ransac_align_fpfh(const glim_amd_cloud* target, const glim_amd_cloud* source, const glim_amd_fpfh* target_fpfh,
                               const glim_amd_fpfh* source_fpfh, uint32_t match_flags, const glim_amd_ransac_params* params,
                               glim_amd_registration_result* result);

/* ---- GNC: gtsam_points::estimate_pose_gnc, the second global registration of viewer/interactive/manual_loop_close_modal.cpp:445-458
 *      (GNCParams{max_init_samples, reciprocal_check = true, tuple_check = false, max_num_tuples 5000, dof 4 | 6, seed}).
 * The gtsam_points source is not in the reference tree: what follows is a restatement from recall plus decisions (listed in DESIGN.md 4.7b).  The
 * algorithm is Fast Global Registration (Zhou, Park, Koltun 2016): optional tuple test, Geman-McClure weights, graduated mu.  FP64 throughout,
 * contraction off, fma where written.
 *   inputs       target and source device clouds (points only), nearest[i] = matched target point of source point i or -1, the parameters.
 *                reciprocal_check is not a parameter: it is the match_flags argument of the *_fpfh entry.
 *   1 selection  max_init_samples >= N_source: every source point is a candidate; otherwise the candidates are the SET
 *                { splitmix64(seed, j) mod N_source : 0 <= j < max_init_samples } (RANSAC's generator; draws with replacement, so the set may be
 *                smaller).  The list L holds the candidates i with nearest[i] >= 0 and both points finite, ascending in i; C = |L|.
 *   2 tuples     only when tuple_check: trials j = 0 .. min(100 C, 2^22) - 1 draw c_k = splitmix64(seed + 1 (mod 2^64), 3 j + k) mod C, k = 0 1 2.
 *                A trial passes when the three entries are distinct and every edge (0,1), (1,2), (2,0) has max(d_s, d_t) > 0 and
 *                min(d_s, d_t) >= tuple_thresh * max(d_s, d_t), d = sqrt((dx^2 + dy^2) + dz^2).  The list becomes the three correspondences of
 *                each of the first max_num_tuples passing trials, in trial order; duplicates are kept (a correspondence in several tuples weighs
 *                more, as in FGR).
 *   3 none       fewer than 3 list entries after 1 and 2: the identity, inlier_rate 0, best_iteration -1, iterations_run 0.  Not an error.
 *   4 frame      c_s, c_t = unweighted centroids of the listed source / target points (sum in the tree of 5, divided by the list length);
 *                p = s - c_s, q = t - c_t.  D^2 = the larger of the squared bounding-box diagonals (dx^2 + dy^2) + dz^2 of the listed source and
 *                of the listed target points.  mu_0 = D^2; mu_min = max_corr_dist^2, or (0.025 sqrt(D^2))^2 when max_corr_dist <= 0.
 *   5 loop       k = 0 .. max_iterations - 1, no data-dependent exit but the one below; the pose starts at the identity.  Per list entry:
 *                  x = R s + t as RANSAC's nine FMAs, d = t_i - x, r^2 = (d_x^2 + d_y^2) + d_z^2, w = (mu / (mu + r^2))^2
 *                seventeen sums over the list, each an FMA chain per lane: W = sum w, a = sum w p, b = sum w q, M = sum (w p) q^T,
 *                cost = sum w r^2.  Tree: lane l of 512 takes the entries l, l + 512, .. in ascending order; the 64 lanes of a wavefront are
 *                added by an xor-butterfly (offsets 32, 16, .. 1); the 8 wavefront sums are added in wavefront order.
 *                Pose: H = M - a b^T / W; R from H as RANSAC derives it from its H (dof 6: Horn's 4 x 4 matrix by 8 cyclic Jacobi sweeps; dof 4:
 *                (C, S) / |(C, S)|, S = H_01 - H_10, C = H_00 + H_11); t = (c_t + b / W) - R (c_s + a / W).  One function for host and device:
 *                glim_amd/csrc/gnc_pose.hpp.  This is the closed-form minimiser for fixed weights, in place of FGR's one Gauss-Newton step.
 *                If W or an entry of the new pose is not finite, the previous pose is kept and the loop ends: iterations_run = k.
 *                After iteration k with k mod 4 = 3 and mu > mu_min: mu <- max(mu / div_factor, mu_min).
 *   6 result     T_target_source = the last pose; num_inliers and inlier_rate by RANSAC's rule exactly: ALL finite source points under that pose
 *                against the occupancy table at inlier_voxel_resolution, inlier_rate = num_inliers / N_source; best_iteration =
 *                iterations_run - 1.  If not one iteration completed (iterations_run = 0) the result is that of 3.
 * Deterministic: the same inputs and seed return the same bits in any context (integer selection, one fixed reduction tree, no floating-point
 * atomics). */
typedef struct {
  int32_t max_init_samples;
  int32_t tuple_check; /* 0 or 1 */
  double tuple_thresh;
  int32_t max_num_tuples;
  double div_factor;
  int32_t max_iterations;
  double max_corr_dist; /* <= 0: 0.025 D */
  double inlier_voxel_resolution;
  int32_t dof; /* 4 or 6 */
  uint64_t seed;
} glim_amd_gnc_params;
typedef struct {
  int64_t num_correspondences; /* C after step 1 */
  int64_t num_tuples;          /* passing trials kept (0 without tuple_check) */
  int64_t list_length;         /* entries the loop ran over */
  double mu_final;             /* the mu of the last completed iteration */
  double weight_sum;           /* its W */
  double cost;                 /* its sum w r^2 */
} glim_amd_gnc_info;
/* 5000, 0, 0.9, 1000, 1.4, 64, 0, 1.0, dof 6, seed 0 */
int glim_amd_gnc_default_params(glim_amd_gnc_params* params);
/* nearest: host array, one entry per source point.  info may be NULL.  GLIM_AMD_ERR_INVALID: a NULL required argument, clouds of two contexts,
 * dof not 4 or 6, max_iterations <= 0, max_init_samples <= 0, max_num_tuples <= 0 with tuple_check, div_factor not finite or <= 1, a NaN
 * tuple_thresh, inlier_voxel_resolution not finite or <= 0, max_corr_dist NaN or infinite, a nearest value < -1 or >= the target size. */
int glim_amd_gnc_align(const glim_amd_cloud* target, const glim_amd_cloud* source, const int32_t* nearest, const glim_amd_gnc_params* params,
                       glim_amd_registration_result* result, glim_amd_gnc_info* info);
/* The same with the correspondences of glim_amd_fpfh_match(target_fpfh, source_fpfh, match_flags) found on the device: `nearest` never visits
 * the host.  match_flags: 0 or GLIM_AMD_FPFH_RECIPROCAL (GNCParams::reciprocal_check).  GLIM_AMD_ERR_INVALID also when a descriptor set is not
 * the size of its cloud or belongs to another context. */
int glim_amd_gnc_align_fpfh(const glim_amd_cloud* target, const glim_amd_cloud* source, const glim_amd_fpfh* target_fpfh,
                            const glim_amd_fpfh* source_fpfh, uint32_t match_flags, const glim_amd_gnc_params* params,
                            glim_amd_registration_result* result, glim_amd_gnc_info* info);

/* ---- GICP fine registration: "a few Levenberg-Marquardt iterations over one unary IntegratedGICPFactor", the loop GLIM runs at
 *      src/glim/mapping/global_mapping_pose_graph.cpp:386-426 (loop-candidate validation, LM <= 10, many candidates in parallel :429-438),
 *      src/glim/mapping/global_mapping.cpp:393-426 (between-submap registration, LM <= 10, then the Hessian at the estimate :423-424),
 *      src/glim/viewer/interactive/manual_loop_close_modal.cpp:470-520 ("run fine registration", LM <= 20, behind RANSAC / GNC) and
 *      src/glim/odometry/loose_initial_state_estimation.cpp (iVox target) -- as a batch of B independent problems (target, source, initial
 *      T_target_source, max_correspondence_distance) in one call with ONE host synchronisation.  The target is fixed.
 * GTSAM's optimiser is not in the reference tree: the rule below is upstream RECALL of LevenbergMarquardtOptimizer in fixed-lambda-factor mode
 * (diagonalDamping off), which gtsam_points' LevenbergMarquardtOptimizerExt follows.  FP64, contraction off; one function for host and device:
 * glim_amd/csrc/lm_step.hpp.
 *   record     "the error at a pose" is the `error` field of glim_amd_gicp_linearize (glim_amd_ivox_gicp_linearize) at that pose: a trial is one
 *              linearising evaluation, which gives the candidate's error and, if it is accepted, the system of the next iteration.  Every trial
 *              record is bit for bit what that entry point returns at the trial's pose.
 *   solve      (H_ss + lambda I) delta = -b_s by 6 x 6 Cholesky; a pivot that is not > 0 is a failed solve (the trial is rejected).
 *   retract    T' = T Exp(delta), omega first (series coefficients below 0.02 rad).  The rotation is re-orthonormalised never: the pose travels as
 *              12 doubles.
 *   round 0    linearise at the initial pose: always kept, neither an iteration nor a trial.  Zero inliers: NO_CORRESPONDENCES, the initial pose
 *              is returned.
 *   a trial    trials += 1.  Accept iff the solve succeeded, the candidate has >= 1 inlier and e_new < e_cur.
 *     accept   T <- T', keep the record, lambda <- max(lambda / lambda_factor, lambda_lower_bound), iterations += 1; CONVERGED if
 *              e_cur - e_new <= absolute_error_tol / error_scale or (e_cur - e_new) / e_cur <= relative_error_tol.
 *     reject   lambda <- lambda * lambda_factor; LAMBDA_BOUND if lambda > lambda_upper_bound; pose and record unchanged, the next candidate is
 *              solved from the kept record with the new lambda.
 *   budgets    then MAX_ITERATIONS at iterations == max_iterations, then MAX_TRIALS at trials == max_trials.
 *   non-finite a non-finite record or pose: NUMERIC, the last kept pose is returned.
 * Deterministic: the same inputs return the same bits, in any batch, in any context of the same device model. */
typedef struct {
  double lambda_initial;     /* 1e-5 (global_mapping.cpp:414 sets 1e-12) */
  double lambda_factor;      /* 10 */
  double lambda_upper_bound; /* 1e5 */
  double lambda_lower_bound; /* 0 */
  double relative_error_tol; /* 1e-5 */
  double absolute_error_tol; /* 1e-5 */
  int32_t max_iterations;    /* 10 (setMaxIterations(10) at global_mapping.cpp:413, global_mapping_pose_graph.cpp:399; 20 in the modal) */
  int32_t max_trials;        /* 0 = 2 x max_iterations; at most 4096 */
  double error_scale;        /* 1.0: the twin of GLIM_AMD_VGICP_ERROR_SCALE; enters the absolute tolerance only */
} glim_amd_lm_params;
#define GLIM_AMD_ALIGN_CONVERGED 1
#define GLIM_AMD_ALIGN_MAX_ITERATIONS 2
#define GLIM_AMD_ALIGN_MAX_TRIALS 3
#define GLIM_AMD_ALIGN_LAMBDA_BOUND 4
#define GLIM_AMD_ALIGN_NO_CORRESPONDENCES 5
#define GLIM_AMD_ALIGN_NUMERIC 6
typedef struct {
  double T_target_source[12]; /* the last kept pose */
  double error;               /* IntegratedGICPFactor::error there (global_mapping_pose_graph.cpp:404) */
  int64_t num_inliers;        /* inlier_fraction = num_inliers / source size (:405) */
  int32_t iterations;         /* accepted trials */
  int32_t trials;
  int32_t status;             /* GLIM_AMD_ALIGN_* */
  int32_t reserved;
  double lambda;              /* after the last trial */
  double compact[GLIM_AMD_COMPACT_DOUBLES]; /* the record at T_target_source: glim_amd_expand_compact gives the linearisation at the estimate
                                               (what global_mapping.cpp:423-424 relinearises for) */
} glim_amd_align_result;
/* the values above */
int glim_amd_gicp_align_default_params(glim_amd_lm_params* params);
/* `count` problems: targets[i], sources[i], T_init12 + 12 i, max_correspondence_distances[i] -> out[i].  params NULL = the defaults.  All handles
 * belong to ONE context (a target may appear in several problems).  count = 0 is OK.  Nothing is launched when an argument is refused:
 * GLIM_AMD_ERR_INVALID: a NULL argument or handle, count < 0, a distance that is NaN or < 0, handles of two contexts, an empty source or target,
 * a parameter that is not finite, lambda_factor <= 1, max_iterations < 0, max_trials < 0 or > 4096, error_scale <= 0;
 * GLIM_AMD_ERR_STATE: a source or target without covariances; GLIM_AMD_ERR_UNSUPPORTED: a distance beyond the index's ring walk (see
 * glim_amd_nn_index_create). */
int glim_amd_gicp_align_batch(const glim_amd_nn_index* const* targets, const glim_amd_cloud* const* sources, const double* T_init12,
                              const double* max_correspondence_distances, int32_t count, const glim_amd_lm_params* params,
                              glim_amd_align_result* out);
/* the same over device iVox targets, glim_amd_ivox handles (loose_initial_state_estimation.cpp); the maps' neighbour modes may differ */
int glim_amd_gicp_align_batch_incremental(const glim_amd_ivox* const* targets, const glim_amd_cloud* const* sources, const double* T_init12,
                                   const double* max_correspondence_distances, int32_t count, const glim_amd_lm_params* params,
                                   glim_amd_align_result* out);

/* ---- ICP fine registration: the same loop over one unary IntegratedICPFactor, what "run fine registration" of GLIM's manual loop closing does
 *      for clouds without covariances (src/glim/viewer/interactive/manual_loop_close_modal.cpp:485-490, LM <= 200) -- as a batch of B independent
 *      problems over glim_amd_nn_index targets.  The rule is the one written above the glim_amd_lm_params structure (glim_amd/csrc/lm_step.hpp),
 *      unchanged; glim_amd_lm_params and glim_amd_align_result are reused.
 *   record     every trial record is bit for bit what glim_amd_icp_linearize returns at the trial's pose with the same flags
 *   flags      0 or GLIM_AMD_ICP_POINT_TO_PLANE, applied to every problem.  GLIM_AMD_FACTOR_BINARY is refused: the target is fixed.
 *   rounds     ICP takes many small steps, so max_trials defaults to 400 -- and a loop that stops after a dozen trials would leave hundreds of
 *              enqueued rounds that only read a status word.  This loop therefore enqueues at most 41 rounds at a time (the most the other
 *              loops enqueue by default), reads the problems' states back and stops enqueueing when no status is still running: one host
 *              synchronisation per 41 rounds, not one per call.  The state lives on the device between chunks, so the result does not
 *              depend on the chunk length, bit for bit.
 * Deterministic: the same inputs return the same bits, in any batch, in any context of the same device model. */
/* the values of glim_amd_gicp_align_default_params with max_iterations = 200 (manual_loop_close_modal.cpp:490) */
int glim_amd_icp_align_default_params(glim_amd_lm_params* params);
/* `count` problems: targets[i], sources[i], T_init12 + 12 i, max_correspondence_distances[i] -> out[i].  params NULL = the defaults above.
 * Nothing is launched when an argument is refused; the refusals are those of glim_amd_gicp_align_batch with two differences: covariances are
 * not required of either cloud, and GLIM_AMD_ERR_STATE means point-to-plane over a target cloud without normals.  So:
 * GLIM_AMD_ERR_INVALID: a NULL argument or handle, count < 0, a flag other than GLIM_AMD_ICP_POINT_TO_PLANE, a distance that is NaN or < 0,
 * handles of two contexts, an empty source or target, the parameter errors of glim_amd_gicp_align_batch; GLIM_AMD_ERR_UNSUPPORTED: a distance
 * beyond the index's ring walk. */
int glim_amd_icp_align_batch(const glim_amd_nn_index* const* targets, const glim_amd_cloud* const* sources, const double* T_init12,
                             const double* max_correspondence_distances, uint32_t flags, int32_t count, const glim_amd_lm_params* params,
                             glim_amd_align_result* out);

/* ---- VGICP fine registration: the same loop over one unary IntegratedVGICPFactor(Pose3(), 0, target->voxels, source), the loop GLIM runs at
 *      src/glim/mapping/global_mapping_pose_graph.cpp:405-417 (loop-candidate validation with registration_type "VGICP", LM <= 10, then `error`
 *      and `inlier_fraction`, many candidates in parallel :429-450) -- as a batch of B independent problems (voxel map, source, initial
 *      T_target_source) in one call with ONE host synchronisation.  The target is fixed; one voxel map per problem.
 * The rule is the one written above the glim_amd_lm_params structure (glim_amd/csrc/lm_step.hpp), with "the record at a pose" read as follows:
 *   record     the compact record of the VGICP factor.  Every trial record is bit for bit what glim_amd_factor_set_linearize returns for a factor
 *              set that holds the same `count` pairs in the same order with the same flags, evaluated at the trial's poses.  How a factor's points
 *              are cut into partial rows depends on the whole set, so the promise is "the same set", not "the factor alone": the bits of a
 *              problem may differ between batches of different composition (by the rounding of an FP32 sum taken in another order).
 *   flags      0 or GLIM_AMD_FACTOR_SURFACE_VALIDATION, applied to every problem.  GLIM_AMD_FACTOR_BINARY is refused: the target is fixed.
 *   result     glim_amd_align_result as above: `error` and `num_inliers` are those of the record at the returned pose (inlier_fraction =
 *              num_inliers / source size), `compact` goes through glim_amd_expand_compact.
 * Deterministic: the same batch returns the same bits, in any context of the same device model.  The caller's factor sets, their plans and a
 * resident session of the context are not touched. */
/* the values of glim_amd_gicp_align_default_params, unchanged */
int glim_amd_vgicp_align_default_params(glim_amd_lm_params* params);
/* `count` problems: targets[i], sources[i], T_init12 + 12 i -> out[i].  params NULL = the defaults.  All handles belong to ONE context (a map
 * may appear in several problems).  count = 0 is OK.  Nothing is launched when an argument is refused:
 * GLIM_AMD_ERR_INVALID: a NULL argument or handle, count < 0, a flag other than GLIM_AMD_FACTOR_SURFACE_VALIDATION, handles of two contexts,
 * an empty source, the parameter errors of glim_amd_gicp_align_batch; GLIM_AMD_ERR_STATE: a map nothing was inserted into or a source without
 * covariances (as glim_amd_factor_set_add). */
int glim_amd_vgicp_align_batch(const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources, const double* T_init12,
                               uint32_t flags, int32_t count, const glim_amd_lm_params* params, glim_amd_align_result* out);

/* ---- CT-GICP frame alignment: the whole per-frame optimisation of GLIM's LiDAR-only continuous-time odometry
 *      (src/glim/odometry/odometry_estimation_ct.cpp:158-195) in one call with ONE host synchronisation: Levenberg-Marquardt over the two poses
 *      of the sweep, X (begin) and Y (end), on the graph { IntegratedCT_GICPFactor, PriorFactor<Pose3>(X) "location consistency",
 *      BetweenFactor<Pose3>(X, Y) "constant velocity" }.  12 DoF, tangent order [X: omega v | Y: omega v], right perturbation; FP64,
 *      contraction off; one function for host and device: glim_amd/csrc/ct_lm_step.hpp.
 *   record     the factor's 12 x 12 record (H_f, b_f, e_f, inliers) at a pair is what glim_amd_ct_gicp_linearize computes there, with the bucket
 *              pose table computed on the device (it agrees with the host's table to 1e-12).  The state the factor keeps for
 *              glim_amd_ct_gicp_error is not touched.
 *   location   r_p = Log(P^-1 X), J_p = J_r(r_p)^-1: adds k_p J_p^T J_p to H[X,X], k_p J_p^T r_p to b[X], k_p r_p^T r_p to the cost.
 *   between    r_b = Log(D^-1 X^-1 Y), J = [-J_r(r_b)^-1 Ad((X^-1 Y)^-1) | J_r(r_b)^-1]: adds k_b J^T J to H, k_b J^T r_b to b, k_b r_b^T r_b to
 *              the cost.  GLIM passes the identity for D.  A precision of 0 switches a term off.
 *   cost       "the error at a pair" is (e_f + location cost) + between cost from the LINEARISING evaluation at that pair: a trial is one search.
 *   solve      (H + lambda I) delta = -b by 12 x 12 Cholesky; a pivot that is not > 0 is a failed solve (the trial is rejected).
 *   retract    X' = X Exp(delta[0:6]), Y' = Y Exp(delta[6:12]) as in the GICP fine registration; never re-orthonormalised.
 *   the rest   round 0, accept / reject, the lambda updates, the statuses (GLIM_AMD_ALIGN_*), the budgets and max_trials = 0 are those of the
 *              GICP fine registration above; glim_amd_lm_params is reused unchanged.
 * Deterministic: the same inputs return the same bits, in any context of the same device model. */
typedef struct {
  double T_location[12];     /* P: the prior on X (row-major 3 x 4); read only when location_precision > 0 */
  double location_precision; /* k_p >= 0 (GLIM: 1e-3 "location consistency") */
  double T_between[12];      /* D: the measurement of X^-1 Y; read only when between_precision > 0 */
  double between_precision;  /* k_b >= 0 (GLIM: 1e3 "constant velocity", D = identity) */
} glim_amd_ct_align_terms;
typedef struct {
  double X[12];                      /* the last kept pair */
  double Y[12];
  glim_amd_ct_linearized linearized; /* the factor's record at it: bit for bit the record (X, Y) was evaluated with */
  double cost;                       /* (linearized.error + location_cost) + between_cost */
  double location_cost;
  double between_cost;
  double lambda;                     /* after the last trial */
  int32_t iterations;                /* accepted trials */
  int32_t trials;
  int32_t status;                    /* GLIM_AMD_ALIGN_* */
  int32_t reserved;
} glim_amd_ct_align_result;
/* the GICP defaults with GLIM's three CT values: lambda_initial 1e-10, absolute_error_tol 1e-2, max_iterations 8 (:176-183) */
int glim_amd_ct_align_default_params(glim_amd_lm_params* params);
/* `factor`: a continuous-time factor over either kind of target.  terms NULL = no terms; params NULL = the defaults above.  Nothing is launched
 * when an argument is refused: GLIM_AMD_ERR_INVALID: a NULL factor, pose or result, a precision that is NaN or < 0, a term that is on with a
 * pose that is not finite, an empty source or target, the parameter errors of glim_amd_gicp_align_batch; GLIM_AMD_ERR_STATE: a source or target
 * without covariances; GLIM_AMD_ERR_UNSUPPORTED: the factor's distance beyond the index's ring walk. */
int glim_amd_ct_align(glim_amd_ct_gicp_factor* factor, const double* X_init12, const double* Y_init12, const glim_amd_ct_align_terms* terms,
                      const glim_amd_lm_params* params, glim_amd_ct_align_result* out);

/* ---- Sub-map bundle optimisation: the Levenberg-Marquardt optimisation of GLIM's sub-mapping bundle (src/glim/mapping/sub_mapping.cpp:183-216,
 *      276-315, 430-452; the pose-only parts of global_mapping.cpp have the same shape) in one call with ONE host synchronisation: N poses X_k
 *      over F binary IntegratedVGICPFactorGPU (voxel map, cloud, target pose t, source pose s; evaluated at T_f = X_t^-1 X_s), P
 *      PriorFactor<Pose3> (:186) and Q BetweenFactor<Pose3> (:210/:212).  6N DoF, tangent order [X_0: omega v | X_1: omega v | ...], right
 *      perturbation; FP64, contraction off; one definition for host and device: glim_amd/csrc/bundle_lm_step.hpp.
 *   record     round r evaluates all F factors at the candidate's T_f, which the device computes (inverse and compose of
 *              glim_amd/csrc/ct_se3.hpp).  Every trial record of factor f is bit for bit what glim_amd_factor_set_linearize returns for a set
 *              of the same F pairs in the same order with the same flags at those T_f.  flags: 0 or GLIM_AMD_FACTOR_SURFACE_VALIDATION.
 *   blocks     those of glim_amd_expand_compact with GLIM_AMD_FACTOR_BINARY at T_f, bit for bit: H_ss, b_s go to pose s; H_tt = Ad^T H_ss Ad,
 *              b_t = -Ad^T b_s to pose t; H_ts (rows of t, columns of s) and its transpose are the off-diagonal blocks.
 *   terms      prior: r = Log(P^-1 X), J = J_r(r)^-1.  between: r = Log(D^-1 X_i^-1 X_j), J = [-J_r(r)^-1 Ad((X_i^-1 X_j)^-1) | J_r(r)^-1].
 *              Each adds J^T L J to H, J^T L r to b and r^T L r to the cost; L is the 6 x 6 information, of which only the upper triangle is
 *              read.
 *   system     H dense symmetric 6N x 6N.  Every entry of H and b is a sum that starts at +0.0, over the factors by ascending index, then the
 *              priors, then the betweens.  cost = ((sum_f e_f) + sum priors) + sum betweens, each by ascending index.  "The cost at a
 *              candidate" comes from the LINEARISING evaluation: a trial is one evaluation.
 *   solve      (H + lambda I) delta = -b by Cholesky, L[i][j] = (A[i][j] - sum_{k<j} L[i][k] L[j][k]) / L[j][j] with the subtractions one at a
 *              time in ascending k.  A pivot that is not > 0 or not finite is a failed solve (the trial is rejected).  A pose that no factor
 *              or term touches is allowed: its block is lambda I and its step is zero.
 *   retract    X_k' = X_k Exp(delta_k) as in the GICP fine registration; never re-orthonormalised.
 *   the rest   round 0, accept / reject, the lambda updates, the statuses (GLIM_AMD_ALIGN_*), the budgets and max_trials = 0 are those of the
 *              GICP fine registration, with "the error" read as the cost and "inliers" as the sum of the factors' inlier counts (with F = 0
 *              there are none to ask for).  glim_amd_lm_params is reused unchanged.
 * The system lives in one workgroup's LDS (160 KiB on gfx950), which sets GLIM_AMD_BUNDLE_MAX_POSES; the factors' blocks live in device memory.
 * Damping terms and Huber between terms: glim_amd_bundle_align_terms below ("Damping terms and Huber between terms").
 * Out of scope: IMU terms in this LDS bundle (V, B variables and ImuFactor are glim_amd_graph_align_nav's: 32 blocks hold only ten frames once a
 * frame needs X, V and B), ISAM2, pose marginals, CombinedImuFactor, robust priors, M-estimators other than Huber, translating a
 * gtsam::NonlinearFactorGraph, several devices.
 * Deterministic: the same inputs return the same bits, in any context of the same device model.  The caller's factor sets, their plans and a
 * resident session of the context are not touched. */
#define GLIM_AMD_BUNDLE_MAX_POSES 32     /* 192 x 192: 149 760 B of packed triangle and right-hand side in LDS */
#define GLIM_AMD_BUNDLE_MAX_FACTORS 1024 /* every ordered pair of 32 poses is 992 */
#define GLIM_AMD_BUNDLE_MAX_TERMS 1024   /* priors; and betweens; and dampings */
typedef struct {
  int32_t pose;
  int32_t reserved;
  double T[12];            /* P (row-major 3 x 4) */
  double information[36];  /* row-major 6 x 6, (omega, v) order; the upper triangle is read */
} glim_amd_bundle_prior;
typedef struct {
  int32_t pose_i, pose_j;  /* different */
  double T[12];            /* D: the measurement of X_i^-1 X_j */
  double information[36];
} glim_amd_bundle_between;
typedef struct {
  double cost;             /* (factor_cost + prior_cost) + between_cost at the returned poses */
  double factor_cost;
  double prior_cost;
  double between_cost;
  int64_t num_inliers;     /* the sum over the factors */
  int32_t iterations;      /* accepted trials */
  int32_t trials;
  int32_t status;          /* GLIM_AMD_ALIGN_* */
  int32_t reserved;
  double lambda;           /* after the last trial */
} glim_amd_bundle_result;
/* the GICP defaults with max_iterations = 20 (sub_mapping.cpp:431) */
int glim_amd_bundle_align_default_params(glim_amd_lm_params* params);
/* Factor f: targets[f], sources[f], target_pose[f], source_pose[f].  X_init12: num_poses x 12.  params NULL = the defaults.  X_out12: num_poses x
 * 12, the last kept poses; compact_out: NULL or num_factors x 29, the records at them (glim_amd_expand_compact gives the blocks).
 * num_poses = 0 is OK.  num_factors = 0 with at least one term is valid.  Nothing is launched when an argument is refused:
 * GLIM_AMD_ERR_INVALID: a NULL argument or handle (an array may be NULL when its count is 0), a negative count, nothing to optimise over
 * (no factor and no term), a pose index out of range, target_pose[f] == source_pose[f], pose_i == pose_j, a handle of another context than
 * `ctx`, an empty source, GLIM_AMD_FACTOR_BINARY or an unknown bit in `flags`, a pose or an information that is not finite, the parameter errors
 * of glim_amd_gicp_align_batch; GLIM_AMD_ERR_STATE: a map nothing was inserted into or a source without covariances (as
 * glim_amd_factor_set_add); GLIM_AMD_ERR_UNSUPPORTED: more poses, factors or terms than the caps above. */
int glim_amd_bundle_align(glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources, const int32_t* target_pose,
                          const int32_t* source_pose, int32_t num_factors, uint32_t flags, const glim_amd_bundle_prior* priors, int32_t num_priors,
                          const glim_amd_bundle_between* betweens, int32_t num_betweens, const double* X_init12, int32_t num_poses,
                          const glim_amd_lm_params* params, double* X_out12, double* compact_out, glim_amd_bundle_result* result);

/* ---- Global-graph optimisation: the sub-map bundle optimisation above at the size of GLIM's global graph (src/glim/mapping/global_mapping.cpp:
 *      430-484, the pairwise IntegratedVGICPFactorGPU between sub-maps, plus that file's pose-only BetweenFactor<Pose3>): the same graph
 *      description, the same rule (glim_amd/csrc/bundle_lm_step.hpp, whose item functions take N from the graph, not from a cap), larger caps.
 *      N poses over F binary factors, P priors and Q betweens; 6N DoF, the bundle's tangent order and perturbation; FP64, contraction off.
 *   record     the bundle's, word for word: every trial record is the bits of a caller's set of the same pairs at the candidate's T_f.
 *   blocks     the bundle's.  The factors' blocks live in device memory (976 B each, 32 MB at the cap).
 *   terms      the bundle's.
 *   system     the bundle's: the same entries, the same order of every sum.  Both systems (the evaluated one, the kept one) live in device
 *              memory as packed lower triangles.
 *   solve      the bundle's: every entry of L, of y and of delta receives the same FP64 operations in the same order.  The factorisation walks
 *              block columns of 64-wide tiles in ascending order and, inside each, ascending k (glim_amd/csrc/graph_solve.hpp);
 *              the back substitution walks them in descending order.  The solve's matrix is column-major in device memory; the layout is not
 *              part of the rule.  A failed pivot is the bundle's failed solve.
 *   retract    the bundle's.
 *   the rest   the bundle's (lm::decide, called).  A round is a sequence of ordinary launches on the context's first stream; a kernel boundary
 *              is the only ordering.  No kernel waits for another workgroup and none declares more than 64 KiB of LDS.  The rounds are
 *              enqueued a few at a time; between two chunks the host reads the status and stops enqueueing when the loop has finished.  The
 *              state lives on the device: the chunk length moves no bit of a result.
 * With the same arguments within the bundle's caps, glim_amd_graph_align returns what glim_amd_bundle_align returns, bit for bit.
 * Damping terms (LinearDampingFactor) and Huber between terms: glim_amd_graph_align_terms below.
 * Velocity and bias variables, vector priors and betweens and IMU terms: glim_amd_graph_align_nav below.
 * Out of scope: ISAM2 (GLIM's global mapping is incremental; this is one batch optimisation over the poses), pose marginals, CombinedImuFactor,
 * robust priors, M-estimators other than Huber, several devices, translating a gtsam::NonlinearFactorGraph.
 * Deterministic: the same inputs return the same bits, in any context of the same device model.  The caller's factor sets, their plans and a
 * resident session of the context are not touched. */
#define GLIM_AMD_GRAPH_MAX_POSES 256     /* 1536 x 1536 */
#define GLIM_AMD_GRAPH_MAX_FACTORS 32768 /* every pair i < j of 256 poses is 32 640 */
#define GLIM_AMD_GRAPH_MAX_TERMS 1024    /* priors; and betweens; and dampings; and vector priors; and vector betweens; and IMU terms */
/* the defaults of glim_amd_bundle_align_default_params */
int glim_amd_graph_align_default_params(glim_amd_lm_params* params);
/* The arguments, the results and the refusals of glim_amd_bundle_align, with the caps above.  Nothing is launched when an argument is refused. */
int glim_amd_graph_align(glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources, const int32_t* target_pose,
                         const int32_t* source_pose, int32_t num_factors, uint32_t flags, const glim_amd_bundle_prior* priors, int32_t num_priors,
                         const glim_amd_bundle_between* betweens, int32_t num_betweens, const double* X_init12, int32_t num_poses,
                         const glim_amd_lm_params* params, double* X_out12, double* compact_out, glim_amd_bundle_result* result);

/* ---- Damping terms and Huber between terms: the two terms GLIM's global mapping graphs are made of beside factors, priors and Gaussian
 *      betweens, for both optimisations above.  The rule is theirs (glim_amd/csrc/bundle_lm_step.hpp) with two additions:
 *   damping    (pose k, diagonal d[6]) is gtsam_points::LinearDampingFactor (global_mapping.cpp:162, 960,
 *              global_mapping_pose_graph.cpp:136: LinearDampingFactor(X(0), 6, init_pose_damping_scale), d = the scale six times;
 *              global_mapping.cpp:523: (key, 6, 1e3) beside an indeterminate pose; loose_initial_state_estimation.cpp:124: the per-axis form).  From upstream recall its error() is 0 and its linearize() a Hessian
 *              factor with G = diag(d), g = 0, f = 0; the factor's source is not in the reference tree.  It adds d[m] to entry
 *              (6k + m, 6k + m) of H and nothing to any other entry, to b or to the cost.  In every sum it comes after the betweens, by
 *              ascending index.  Several dampings on one pose are allowed.  A pose touched only by dampings has the block diag(sum d) +
 *              lambda I, the right-hand side +0.0 and a zero step.
 *   huber      between q may carry a width k_q >= 0 (0: the Gaussian between): noiseModel::Robust(Huber(k_q), information), as
 *              global_mapping_pose_graph.cpp:465-468 gives every loop factor.  With c = r^T L r and s = sqrt(c), the between is down-weighted
 *              iff k_q > 0 and s > k_q: then w = k_q / s, its J^T L J and J^T L r are multiplied entry by entry by w and its cost becomes
 *              k_q ((s + s) - k_q); otherwise w = 1.0 and its contribution keeps the Gaussian between's bits.  This is gtsam's
 *              Robust::WhitenSystem and Huber loss in the cost convention here (cost = r^T L r, twice gtsam's error).
 * glim_amd_bundle_result is reused: between_cost is the sum of the robust costs.  between_weight_out: NULL, or num_betweens doubles, the weights
 * w of the evaluation at the returned poses (kept on the device with the kept system; 1.0 for a Gaussian between).
 * more == NULL, or no damping and no width that is not 0, returns what the entry point without `_terms` returns, bit for bit.  The refusals are
 * those of that entry point, and, also before anything is launched: GLIM_AMD_ERR_INVALID: a negative num_dampings, NULL dampings with a
 * positive count, a damping's pose out of range, a diagonal entry or a width that is negative or not finite, a graph with dampings but no
 * factor, prior or between (there is nothing to optimise over); GLIM_AMD_ERR_UNSUPPORTED: more dampings than *_MAX_TERMS.
 * Out of scope: ISAM2, pose marginals, CombinedImuFactor, IMU terms in the LDS bundle, robust priors, other M-estimators, several devices. */
typedef struct {
  int32_t pose;
  int32_t reserved;
  double diagonal[6];      /* (omega, v) order; each >= 0 and finite */
} glim_amd_graph_damping;
typedef struct {
  const glim_amd_graph_damping* dampings;
  int32_t num_dampings;
  int32_t reserved;
  const double* between_huber_width; /* NULL, or num_betweens values; 0 = Gaussian */
} glim_amd_graph_terms;
int glim_amd_bundle_align_terms(glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources,
                                const int32_t* target_pose, const int32_t* source_pose, int32_t num_factors, uint32_t flags,
                                const glim_amd_bundle_prior* priors, int32_t num_priors, const glim_amd_bundle_between* betweens, int32_t num_betweens,
                                const double* X_init12, int32_t num_poses, const glim_amd_lm_params* params, double* X_out12, double* compact_out,
                                glim_amd_bundle_result* result, const glim_amd_graph_terms* more, double* between_weight_out);
int glim_amd_graph_align_terms(glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources,
                               const int32_t* target_pose, const int32_t* source_pose, int32_t num_factors, uint32_t flags,
                               const glim_amd_bundle_prior* priors, int32_t num_priors, const glim_amd_bundle_between* betweens, int32_t num_betweens,
                               const double* X_init12, int32_t num_poses, const glim_amd_lm_params* params, double* X_out12, double* compact_out,
                               glim_amd_bundle_result* result, const glim_amd_graph_terms* more, double* between_weight_out);

/* ---- Graph optimisation with velocity and bias variables: the global-graph optimisation above over the graphs GLIM builds with enable_imu =
 *      true (its default).  Sub-mapping (src/glim/mapping/sub_mapping.cpp:218-243): per odometry frame a PriorFactor<Vector3> on V and a
 *      PriorFactor<ConstantBias> on B (:226-227), per consecutive pair a BetweenFactor<ConstantBias> (:235) and an ImuFactor(X_last, V_last,
 *      X_cur, V_cur, B_last) (:237) or, with too few IMU samples, a BetweenFactor<Vector3> on the velocities (:240).  Global mapping
 *      (global_mapping.cpp:168-216, 976-1042): endpoint poses E(2i), E(2i+1) tied to X(i) by pose betweens, bias priors and betweens (:191-192,
 *      :201), an ImuFactor (:216) or a velocity between (:213) from one sub-map's right endpoint to the next one's left.  The same terms:
 *      odometry_estimation_imu.cpp:218-220, 268-283, loose_initial_state_estimation.cpp:105-124, 174.  One definition for host and device:
 *      glim_amd/csrc/nav_terms.hpp, called by glim_amd/csrc/bundle_lm_step.hpp.
 *   nodes      the N <= GLIM_AMD_GRAPH_MAX_POSES six-wide blocks of the system are nodes with a kind.  GLIM_AMD_NODE_POSE: as above, 12 doubles,
 *              retraction X Exp(delta).  GLIM_AMD_NODE_BIAS: 6 doubles in gtsam's ConstantBias::vector() order (acc, gyro), retraction
 *              b + delta.  GLIM_AMD_NODE_VELOCITY: 3 doubles (world frame), retraction v + delta[0..3); its rows 3..5 are touched by nothing and
 *              carry lambda on the diagonal, +0.0 on the right-hand side and a zero step.  Node values travel as rows of 12 doubles: a vector
 *              kind uses the leading 6 / 3 entries, the rest is +0.0 going in and coming out.  The tangent order, the packed system, the solve,
 *              the decision rule, the statuses and the chunked enqueueing are the global-graph optimisation's, unchanged: 6N is the system size.
 *              Factors, pose priors and pose betweens must name POSE nodes; a damping may name any node (LinearDampingFactor(B(0), 6, 1e6),
 *              odometry_estimation_imu.cpp:220).
 *   terms      each adds J^T L J, J^T L r and r^T L r (L r and L J first, sums ascending from +0.0, the upper triangle of L read).
 *              vector prior (node k of kind BIAS or VELOCITY, value p[6], information 6 x 6): r = x_k - p, J = I; for a VELOCITY the leading
 *              3 x 3 of the information and 3 of p are read.  vector between (nodes i != j of one vector kind, measurement d[6]):
 *              r = (x_j - x_i) - d, J = [-I | I].  IMU term (POSE i, VELOCITY vi, POSE j, VELOCITY vj, BIAS b, all distinct): gtsam::ImuFactor.
 *              gtsam's source is not in the reference tree, so the following is UPSTREAM RECALL (PreintegrationBase::computeError without
 *              Coriolis term and body_P_sensor).  With db = b - bias_hat: (., dp_c, dv_c) = delta + H_bias db on the position and velocity
 *              rows in both modes; GLIM_AMD_IMU_TANGENT (gtsam's TangentPreintegration, the build default): theta_c = theta + H_bias[0..3, :]
 *              db; GLIM_AMD_IMU_MANIFOLD (Forster et al.): theta_c = Log(Exp(theta) Exp(H_bias[0..3, 3..6] db_gyro)).  Prediction:
 *              R^ = R_i Exp(theta_c), p^ = p_i + v_i dt + g dt^2 / 2 + R_i dp_c, v^ = v_i + g dt + R_i dv_c.  Residual: r = [Log(R_j^T R^);
 *              R_j^T (p^ - p_j); R_j^T (v^ - v_j)].  J (9 x 24 over the five nodes' used columns) is the exact derivative of r under the
 *              retractions above; its blocks are written out in glim_amd/csrc/nav_terms.hpp.
 *   sums       within a block's list: factors, pose priors, pose betweens, vector priors, vector betweens, IMU terms, dampings, each by
 *              ascending index.  cost = ((((factors + priors) + betweens) + vector priors) + vector betweens) + IMU.
 * With every node a POSE (or nav == NULL) and no new term, glim_amd_graph_align_nav returns the bits of glim_amd_graph_align_terms.
 * The sub-map bundle (glim_amd_bundle_align*) is NOT extended: it keeps its system in LDS, and 32 blocks hold only ten frames once a frame needs
 * X, V and B.
 * Refusals, all before anything is launched: those of glim_amd_graph_align_terms, and GLIM_AMD_ERR_INVALID: an unknown kind or mode; a term
 * naming a node of the wrong kind or out of range; repeated nodes in one term; dt <= 0 or not finite; any input that is not finite; a VELOCITY
 * row whose entries 3..11, or a BIAS row whose entries 6..11, are not +0.0; a negative count or a NULL array with a positive count; a graph with
 * nothing but dampings.  GLIM_AMD_ERR_UNSUPPORTED: more vector priors, vector betweens or IMU terms than GLIM_AMD_GRAPH_MAX_TERMS each.
 * Out of scope: ISAM2 and the fixed-lag smoother, marginals, CombinedImuFactor, the Coriolis term, body_P_sensor, IMU terms in the LDS bundle, a
 * preintegrator for raw IMU samples (the caller's gtsam has one), robust priors, other M-estimators, several devices. */
#define GLIM_AMD_NODE_POSE 0
#define GLIM_AMD_NODE_BIAS 1
#define GLIM_AMD_NODE_VELOCITY 2
#define GLIM_AMD_IMU_TANGENT 0
#define GLIM_AMD_IMU_MANIFOLD 1
typedef struct {
  int32_t node;            /* of kind BIAS or VELOCITY */
  int32_t reserved;
  double value[6];         /* p; a VELOCITY reads 3 */
  double information[36];  /* row-major 6 x 6; the upper triangle (a VELOCITY: of the leading 3 x 3) is read */
} glim_amd_nav_vector_prior;
typedef struct {
  int32_t node_i, node_j;  /* different, of one vector kind */
  double measurement[6];   /* d: the measurement of x_j - x_i */
  double information[36];
} glim_amd_nav_vector_between;
typedef struct {
  int32_t pose_i, velocity_i, pose_j, velocity_j, bias; /* all distinct */
  int32_t mode;            /* GLIM_AMD_IMU_TANGENT or GLIM_AMD_IMU_MANIFOLD */
  double dt;               /* > 0 */
  double gravity[3];       /* gtsam's n_gravity */
  double bias_hat[6];      /* (acc, gyro) */
  double delta[9];         /* (theta, dp, dv): the preintegrated measurement at bias_hat */
  double H_bias[54];       /* row-major 9 x 6: its derivative by (acc, gyro) */
  double information[81];  /* row-major 9 x 9 in (rot, pos, vel) order: the inverse of preintMeasCov; the upper triangle is read */
} glim_amd_nav_imu_term;
typedef struct {
  const int32_t* kinds;    /* num_poses kinds (GLIM_AMD_NODE_*), or NULL: every node is a POSE */
  const glim_amd_nav_vector_prior* vector_priors;
  const glim_amd_nav_vector_between* vector_betweens;
  const glim_amd_nav_imu_term* imu_terms;
  int32_t num_vector_priors, num_vector_betweens, num_imu_terms;
  int32_t reserved;
} glim_amd_nav_terms;
typedef struct {
  double cost;             /* ((((factor + prior) + between) + vector_prior) + vector_between) + imu at the returned nodes */
  double factor_cost;
  double prior_cost;
  double between_cost;
  double vector_prior_cost;
  double vector_between_cost;
  double imu_cost;
  int64_t num_inliers;
  int32_t iterations;
  int32_t trials;
  int32_t status;          /* GLIM_AMD_ALIGN_* */
  int32_t reserved;
  double lambda;
} glim_amd_nav_result;
/* The arguments of glim_amd_graph_align_terms with `X` read as node values (num_poses x 12), a result of its own and the node kinds and new
 * terms in `nav` (NULL: none).  more and between_weight_out may be NULL. */
int glim_amd_graph_align_nav(glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources,
                             const int32_t* target_pose, const int32_t* source_pose, int32_t num_factors, uint32_t flags,
                             const glim_amd_bundle_prior* priors, int32_t num_priors, const glim_amd_bundle_between* betweens, int32_t num_betweens,
                             const double* X_init12, int32_t num_poses, const glim_amd_lm_params* params, double* X_out12, double* compact_out,
                             glim_amd_nav_result* result, const glim_amd_graph_terms* more, double* between_weight_out,
                             const glim_amd_nav_terms* nav);

/* ---- Scan-to-keyframes VGICP registration: the LiDAR part of GLIM's frame-to-keyframes matching cost
 *      (src/glim/odometry/odometry_estimation_gpu.cpp:150-165, 183-203): one unary IntegratedVGICPFactorGPU(fixed_target_pose, X(current),
 *      voxelmap, frame) per keyframe and per voxel-map level, ALL on the same pose variable -- as a batch of `count` independent problems, each
 *      one pose X_i (T_world_source) over M_i targets with fixed poses P_f (T_world_target), in one call with ONE host synchronisation.  Also a
 *      multi-resolution loop-candidate check.  One definition for host and device: glim_amd/csrc/keyframe_lm_step.hpp.
 * A sum of compact records is a compact record, so the rule is the one written above the glim_amd_lm_params structure
 * (glim_amd/csrc/lm_step.hpp), unchanged, applied to the summed record; glim_amd_lm_params and glim_amd_align_result are reused.
 *   poses      factor f of problem i is evaluated at T_f = P_f^-1 X_i (inverse and compose of glim_amd/csrc/ct_se3.hpp, FP64).  With right
 *              perturbation X Exp(d) gives T_f Exp(d): the H_ss and b_s of every factor are already expressed in d of X and simply add.
 *   record     every trial record of factor f is bit for bit what glim_amd_factor_set_linearize returns for a set of the same F (map, source)
 *              pairs in the same order with the same flags at those T_f.  The promise is tied to "the same set", not to the factor alone (see
 *              the VGICP fine registration above).
 *   sum        each of the 29 entries of the problem's record is ((+0.0 + r_first) + ...) + r_last over its factors by ascending index, FP64.
 *   prior      at most one per problem (.pose = the problem's index): r = Log(P^-1 X), J = J_r(r)^-1, the bundle's definitions; J^T L J is
 *              added to H, J^T L r to b and r^T L r to the error, LAST, after the factors; only the upper triangle of L is read.  The inlier
 *              count is the factors' sum only: a prior alone never makes a candidate acceptable.
 *   result     T_target_source holds the last kept X; `error`, `num_inliers` and `compact` are the summed record there (prior included): its
 *              H_ss is the information a caller hands to a pose graph.  Statuses, budgets and max_trials = 0 are as in the GICP section.
 *   non-finite an X_init or a P_f that is not finite ends ITS problem with GLIM_AMD_ALIGN_NUMERIC in round 0 (X_init is returned), as a
 *              non-finite initial pose does in the GICP section; the other problems of the batch run.  Round 0 still evaluates that problem's
 *              factors at the non-finite T_f, as the VGICP fine registration does for a non-finite T_init; nothing of it is kept.  A
 *              non-finite prior is refused.
 *   flags      0 or GLIM_AMD_FACTOR_SURFACE_VALIDATION (GLIM sets it at :162), for every factor.  GLIM_AMD_FACTOR_BINARY is refused.
 * Deterministic: the same batch returns the same bits, in any context of the same device model.  The caller's factor sets, the context's plans
 * and a resident session are not touched. */
#define GLIM_AMD_KEYFRAME_ALIGN_MAX_TARGETS 64 /* per problem; GLIM: (15 keyframes + 2 window frames) x 2 levels = 34 */
/* the values of glim_amd_gicp_align_default_params, unchanged */
int glim_amd_keyframe_align_default_params(glim_amd_lm_params* params);
/* sources: `count`, one per problem.  first_target: count + 1 offsets into the next two arrays, M_i = first_target[i + 1] - first_target[i].
 * targets: F = first_target[count] maps (a map may appear several times); T_world_target12: F x 12, P_f; X_init12: count x 12.  priors: NULL
 * with num_priors = 0, or num_priors entries.  params NULL = the defaults.  out: count.  factor_compact_out: NULL or F x 29, every factor's
 * record at the returned pose of its problem: the records of the last round that was kept.  A problem that ends in round 0 with
 * NO_CORRESPONDENCES kept round 0: its records are round 0's, with zero inliers.  A problem that kept nothing (NUMERIC in round 0) has zeros.
 * count = 0 is OK.  Nothing is launched when an argument is refused:
 * GLIM_AMD_ERR_INVALID: a NULL argument or handle, count < 0, num_priors < 0, offsets that do not ascend from 0, a problem with no target,
 * handles of two contexts, an empty source, a prior whose pose or information is not finite, a prior index out of range, a second prior for
 * one problem, GLIM_AMD_FACTOR_BINARY or an unknown bit in `flags`, the parameter errors of glim_amd_gicp_align_batch; GLIM_AMD_ERR_STATE: a
 * map nothing was inserted into or a source without covariances (as glim_amd_factor_set_add); GLIM_AMD_ERR_UNSUPPORTED: more than
 * GLIM_AMD_KEYFRAME_ALIGN_MAX_TARGETS targets in a problem. */
int glim_amd_keyframe_align_batch(const glim_amd_cloud* const* sources, const int32_t* first_target, const glim_amd_voxelmap* const* targets,
                                  const double* T_world_target12, const double* X_init12, const glim_amd_bundle_prior* priors, int32_t num_priors,
                                  uint32_t flags, int32_t count, const glim_amd_lm_params* params, glim_amd_align_result* out,
                                  double* factor_compact_out);

/* ---- Plane / edge bundle-adjustment factors and ball selection ------------------------------------------------------------------------
 * The device side of the reference's plane bundle-adjustment tool (src/glim/viewer/interactive/bundle_adjustment_modal.cpp): the ball
 * selection of extract_points (:143-161), the statistics of calc_eigenvalues (:163-184), the radius search of auto_radius (:186-227) and the
 * factor create_factor builds (:229-245), gtsam_points::PlaneEVMFactor (and its sibling EdgeEVMFactor).
 *
 *   inputs     S device clouds, S poses T_s (3x4 row-major FP64, world <- sub-map), a centre c and a radius r.  A point's coordinates are the
 *              cloud's exact FP64 points where it keeps them (preprocessed, deskewed, merged and glim_amd_cloud_create_exact clouds), otherwise
 *              its FP32 points widened to double.  Known difference: the reference's points are doubles and glim_amd_cloud_create rounds
 *              them to float; a caller who needs the reference's booleans at the ball's surface uploads with glim_amd_cloud_create_exact.
 *   selection  d = t - c is rounded once (three subtractions), then per point
 *                  q_x = ((R00 p_x + R01 p_y) + R02 p_z) + d_x      (likewise q_y, q_z; every product and sum rounded, no FMA)
 *                  qq  = (q_x q_x + q_y q_y) + q_z q_z
 *              and the point is selected iff qq < r r (r r rounded once; strict, as at :154).  Pairs (sub-map index, point index) come out
 *              ascending in sub-map, then in point -- the reference's loop order -- by a stable compaction over a prefix sum; no atomic
 *              decides an order.  The call always reports the total count and writes at most `capacity` pairs, the first ones.
 *   statistics N, s = sum q and S = sum q q^T (00 01 02 11 12 22) over the selection, then mean = s / N, cov = (S - mean s^T) / N (:177-178)
 *              and the three eigenvalues, ascending, by the closed-form solver the reference calls (computeDirect, :181).  N = 0 gives zero
 *              sums and NaN eigenvalues.  Every FP64 sum runs in an order that depends on the point order alone: the points are cut into
 *              blocks of 256 in (sub-map, point) order, a block sums its values by one fixed tree over its lanes, and an ordered pass
 *              adds the block sums: by ascending block inside 64 runs of consecutive blocks, then the 64 run sums by ascending run.  No
 *              floating-point atomic.  Two calls give the same bits.
 *   auto radius the rule of :186-227 with radii as doubles.  r0 is evaluated; then at most GLIM_AMD_BA_MAX_TRIALS trials, each at 0.8 r if
 *              lambda_0 / lambda_2 > plane_eps at the current radius r, otherwise at 1.1 r.  The search stops without taking the trial when
 *              the trial leaves [min_radius, max_radius], or selects fewer than 10 points, or is larger than r0 with
 *              lambda_0 / lambda_2 > plane_eps.  Every trial is enqueued up front, a small device state decides each, later rounds idle
 *              once the search has stopped, and the host synchronises ONCE.  The transformed points are kept across the rounds (32 B per
 *              point), so a trial is a filtered reduction.
 *   factor     K <= GLIM_AMD_BA_MAX_FRAMES frames, each with points in its own local frame.  kind GLIM_AMD_BA_PLANE: cost lambda_0;
 *              GLIM_AMD_BA_EDGE: cost lambda_0 + lambda_1.  Creation is the only pass over points: per frame f, with c_f the frame's first
 *              point in factor order, it keeps n_f, v_f = sum (p - c_f) and P_f = sum (p - c_f)(p - c_f)^T (FP64, ordered sums as above,
 *              per frame).  error() and linearize() take K poses -- any poses -- and read the moments only:
 *                  tau = R c_f + t,  sum q = sum_f (R v + n tau),  sum q q^T = sum_f (R P R^T + R v tau^T + tau (R v)^T + n tau tau^T),
 *                  m = sum q / N,  C = sum q q^T / N - m m^T,  eigenpairs (lambda_k, u_k) of C (same solver)
 *              with tau taken about the tau of frame 0 (C does not depend on the origin; only tau - m is used below).  For the eigenvalue
 *              index e (0; edge: 0 and 1, the results added) and k != e, per frame: c_k = R^T u_k, alpha_k = u_k . (tau - m),
 *              A_k = c_k . v + n alpha_k, B_k = P c_k + alpha_k v + A_k c_f, s = v + n c_f, Pt = P + v c_f^T + c_f v^T + n c_f c_f^T.
 *              Tangent order [rotation, translation], perturbation T Exp(xi) (dq/dxi = [-R hat(p), R]):
 *                  g_f  = (2 / N) [B_e x c_e ; A_e c_e]
 *                  H_ff += (2 / N) [[hat(c_e) Pt hat(c_e)^T, (s x c_e) c_e^T], [. ^T, n c_e c_e^T]]
 *                  H   -= (2 / N^2) S S^T,  S_f = [s x c_e ; n c_e]
 *                  H   += sum_{k != e} (2 / N^2) / (lambda_e - lambda_k) W_k W_k^T,  W_k,f = [B_e x c_k + B_k x c_e ; A_e c_k + A_k c_e]
 *              For the edge kind the k = 1 term of e = 0 and the k = 0 term of e = 1 are the same W W^T with opposite coefficients: their
 *              sum is zero and neither is formed (nor can their gap set the DEGENERATE bit).
 *              H is symmetric (bit for bit) and in general indefinite -- the last terms are negative for lambda_0 --: callers damp it.
 *              When |lambda_e - lambda_k| <= 1e-12 max(lambda_2, DBL_MIN) that k term is dropped and GLIM_AMD_BA_DEGENERATE is set in the
 *              status word.  A factor of fewer than 3 points is refused (GLIM_AMD_ERR_INVALID).  The cost is the eigenvalue sum, unscaled.
 * Deterministic: the same call returns the same bits. */
#define GLIM_AMD_BA_MAX_FRAMES 128
#define GLIM_AMD_BA_MAX_TRIALS 10
#define GLIM_AMD_BA_PLANE 0
#define GLIM_AMD_BA_EDGE 1
#define GLIM_AMD_BA_DEGENERATE 0x1u
#define GLIM_AMD_BA_MOMENT_DOUBLES 13 /* per frame: n | c_f (3) | v_f (3) | P_f (00 01 02 11 12 22) */
enum { /* why the radius search ended */
  GLIM_AMD_BA_STOP_TRIALS = 0,     /* all GLIM_AMD_BA_MAX_TRIALS trials were taken */
  GLIM_AMD_BA_STOP_RANGE = 1,      /* the next trial left [min_radius, max_radius] */
  GLIM_AMD_BA_STOP_FEW_POINTS = 2, /* the trial selected fewer than 10 points */
  GLIM_AMD_BA_STOP_PLANE_EPS = 3   /* a trial larger than r0 had lambda_0 / lambda_2 > plane_eps */
};
typedef struct glim_amd_ba_params { /* bundle_adjustment_modal.cpp:21-25 */
  double min_radius; /* 0.1 */
  double max_radius; /* 5.0 */
  double plane_eps;  /* 0.01 */
} glim_amd_ba_params;
typedef struct glim_amd_ba_stats {
  int64_t num_points;
  double sum[3];
  double sum_cross[6]; /* 00 01 02 11 12 22 */
  double eigenvalues[3];
} glim_amd_ba_stats;
typedef struct glim_amd_ba_radius_result {
  double radius;      /* the last radius that was kept */
  int64_t num_points; /* selected at that radius */
  double eigenvalues[3];
  int32_t trials; /* trials that were evaluated (<= GLIM_AMD_BA_MAX_TRIALS; r0 itself is not a trial) */
  int32_t stop;   /* GLIM_AMD_BA_STOP_* */
} glim_amd_ba_radius_result;
typedef struct glim_amd_ba_factor glim_amd_ba_factor; /* a child of its context */

int glim_amd_ba_default_params(glim_amd_ba_params* params);
/* clouds: num_clouds >= 1 handles of one context (a cloud may be empty); T_world_submap12: num_clouds x 12; pairs: NULL with capacity 0, or
 * capacity x 2 int32.  GLIM_AMD_ERR_INVALID: a NULL argument or handle, num_clouds < 1, clouds of two contexts, a radius that is NaN,
 * infinite or <= 0, capacity < 0, a pose or centre that is not finite, more than 2^31 - 257 points in all. */
int glim_amd_ba_ball_select(const glim_amd_cloud* const* clouds, int32_t num_clouds, const double* T_world_submap12, const double* center3,
                            double radius, int64_t capacity, int32_t* pairs, int64_t* count);
int glim_amd_ba_ball_stats(const glim_amd_cloud* const* clouds, int32_t num_clouds, const double* T_world_submap12, const double* center3,
                           double radius, glim_amd_ba_stats* out);
/* params NULL = the defaults.  Also GLIM_AMD_ERR_INVALID: min_radius > max_radius, or a parameter that is NaN. */
int glim_amd_ba_auto_radius(const glim_amd_cloud* const* clouds, int32_t num_clouds, const double* T_world_submap12, const double* center3,
                            double radius0, const glim_amd_ba_params* params, glim_amd_ba_radius_result* out);
/* A factor from host arrays: points3 is n x 3 (frame-local), frame_index n entries in [0, num_frames).  Factor order is ascending frame
 * index, then the order given.  Frames without a point are dropped; glim_amd_ba_factor_info returns the kept indices, ascending.
 * GLIM_AMD_ERR_INVALID: a NULL argument, a kind other than GLIM_AMD_BA_PLANE / GLIM_AMD_BA_EDGE, n < 3, num_frames < 1 or
 * > GLIM_AMD_BA_MAX_FRAMES, a frame index out of range, a point that is not finite. */
int glim_amd_ba_factor_create(glim_amd_ctx* ctx, int32_t kind, int64_t n, const double* points3, const int32_t* frame_index,
                              int32_t num_frames, glim_amd_ba_factor** out);
/* A factor from the ball selection, which never leaves the device: frame f holds the selected points of the f-th sub-map that has any,
 * in point order, in that sub-map's frame.  Arguments as glim_amd_ba_ball_select; also GLIM_AMD_ERR_INVALID: fewer than 3 points selected
 * or more than GLIM_AMD_BA_MAX_FRAMES sub-maps with a selected point. */
int glim_amd_ba_factor_create_from_ball(const glim_amd_cloud* const* clouds, int32_t num_clouds, const double* T_world_submap12,
                                        const double* center3, double radius, int32_t kind, glim_amd_ba_factor** out);
/* any output may be NULL.  kept_index: K entries; moments: K x GLIM_AMD_BA_MOMENT_DOUBLES */
int glim_amd_ba_factor_info(const glim_amd_ba_factor* factor, int32_t* num_frames, int64_t* num_points, int32_t* kind, int32_t* kept_index,
                            double* moments);
/* poses12: K x 12, the poses of the kept frames in their order.  status: GLIM_AMD_BA_DEGENERATE or 0 (may be NULL).
 * GLIM_AMD_ERR_INVALID: a NULL factor, pose array or output, a pose that is not finite. */
int glim_amd_ba_factor_error(const glim_amd_ba_factor* factor, const double* poses12, double* cost, uint32_t* status);
/* g: 6 K; H: 6 K x 6 K row-major, the whole matrix.  One small kernel over the frames and one fill over the block pairs; no point is read. */
int glim_amd_ba_factor_linearize(const glim_amd_ba_factor* factor, const double* poses12, double* cost, double* g, double* H,
                                 uint32_t* status);
int glim_amd_ba_factor_destroy(glim_amd_ba_factor* factor);

/* ---- Map editing: point selection, segmentation, removal -------------------------------------------------------------------------------
 * The device side of the reference's map editor (src/glim/viewer/editor/points_selector.cpp): the box / sphere gizmo (:623-674), the
 * radius selection (:677-700), the statistical outliers in a radius (:703-759), region growing (:798-810) and the removal of the selection
 * from the sub-map clouds (:513-562), and min-cut segmentation (:774-797), the editor's default segmentation method.
 *
 *   inputs     S device clouds and S matrices M_s (3x4 row-major FP64); point coordinates as for the ball selection above (the exact FP64
 *              points where the cloud keeps them, FP32 widened otherwise).  The transformed point is
 *                  v_x = ((M00 p_x + M01 p_y) + M02 p_z) + M03      (likewise v_y, v_z; every product and sum rounded, no FMA)
 *   selection  pairs (sub-map index, point index), int32, ascending in sub-map and then in point, by a stable compaction over a prefix
 *              sum; no atomic decides an order or a result.  Every call reports the true count and writes at most `capacity` pairs, the
 *              first ones.  Modes:
 *                BOX / SPHERE   M_s = T_local_submap = inv(gizmo model matrix) T_world_submap, formed by the caller (:630, :637; the C++
 *                               and Python mirrors do it).  Box: -0.5 < v_k < 0.5 for all k (:648).  Sphere: (v_x v_x + v_y v_y) + v_z v_z
 *                               < 1.0 (:654).  Both strict.
 *                WINDOW         M_s = T_world_submap.  collect_neighbor_point_ids (:85-112) as a set: the point's cell is
 *                               floor(v_k * (1.0 / resolution)) -- the product of :177 / :593 --, the window's centre cell is
 *                               floor(c_k / resolution) -- the division of :87 --, and the point is kept iff every cell coordinate lies
 *                               within `window` cells of the centre's.
 *                WINDOW_BALL    WINDOW and e = v - c, qq = (e_x e_x + e_y e_y) + e_z e_z, qq < r r (r r rounded once; strict, :690-691).
 *                               The point is transformed first and the centre subtracted after: not the d = t - c form of
 *                               glim_amd_ba_ball_select.
 *   outliers   (:703-759) candidates = WINDOW_BALL with radius r + radius_offset; their world points go into a transient cloud in pair
 *              order (its FP32 image holds e = v - c, which keeps the neighbour search's rounding to that of a few metres); the exact kNN
 *              (k = num_neighbors <= 32, query included) and the statistic of glim_amd_preprocess's outlier removal run on it: d_i = mean
 *              distance to the k neighbours, threshold = mean(d) + stddev_thresh * std(d), inlier iff d_i < threshold.  Returned: the
 *              candidates with qq < r r that are not inliers.  Candidates between r and r + radius_offset take part in the statistic and
 *              are never returned.  Fewer candidates than k: count 0 and status GLIM_AMD_EDIT_FEW_POINTS (:730-733).
 *   region growing  gtsam_points::region_growing_* is not in the reference tree; these semantics are this project's and do not depend on
 *              a traversal order.  Candidates: the WINDOW selection around the picked point c (:800).  Seed: the candidate with the
 *              smallest qq to c, ties to the smaller pair.  Edge i-j: dd = (dx dx + dy dy) + dz dz < distance_threshold^2 (rounded once),
 *              strict; with use_normals additionally |n_i . n_j| >= cos_angle_threshold, n the cloud's FP32 normal widened and rotated
 *              to world in the order above (every cloud that has points needs normals: GLIM_AMD_ERR_STATE otherwise).  Cluster: the connected component
 *              of the seed; level = hop count from the seed (seed 0); max_hops > 0 keeps levels <= max_hops.  Dilation: with
 *              dilation_radius > 0 every other candidate strictly within it of a cluster point joins at level (last level + 1); no normal
 *              test.  No candidate: count 0 and status GLIM_AMD_EDIT_EMPTY.  The growth is rounds of one kernel in which every
 *              unassigned candidate looks for a neighbour of a lower level in a uniform grid; the rounds are enqueued
 *              GLIM_AMD_EDIT_ROUNDS_PER_LOOK at a time and the host reads the rounds' counters between chunks, so a cluster of any
 *              diameter terminates.  `rounds` is the number of growth rounds that assigned a point (= the last level before dilation).
 *   min-cut    gtsam_points::min_cut is not in the reference tree; these semantics are this project's and are a function of the point set
 *              alone.  Candidates: WINDOW_BALL around the picked point c with radius background_mask_radius + 1.0, strict (:777-780), m
 *              of them.  m = 0: status GLIM_AMD_EDIT_EMPTY; m < k_neighbors + 1: GLIM_AMD_EDIT_FEW_POINTS.  Neighbours: the candidates'
 *              world points go into a transient cloud in pair order as for the outliers (FP32 image e = v - c, the FP64 points beside
 *              it) and the exact kNN runs with K = k_neighbors + 1; entries equal to the query's own index are dropped wherever they
 *              stand.  Edges: undirected, {i, j} exists iff j is among i's neighbours or i among j's; duplicates are merged by sorting
 *              the keys (min << 32 | max) and comparing with the predecessor, so the edge list is in ascending key order and no atomic
 *              decides anything.  Edge weight, FP64, every product and sum rounded on its own:
 *                  dd = (dx dx + dy dy) + dz dz  on the FP64 world points;   w = exp(-(dd / (sigma_d sigma_d)))
 *                  with use_normals:  w = w exp(-((t t) / (sigma_a sigma_a))),  t = acos(min(1, |n_i . n_j|)),  n as in region growing
 *                  capacity = (int32) floor(w * GLIM_AMD_EDIT_CAP_SCALE + 0.5), the same in both directions; an edge of capacity 0 is
 *                  kept and carries nothing.
 *              Terminals: a foreground point (qq < fg fg, strict) is tied to the source with floor(foreground_weight * 65536 + 0.5), a
 *              background point (qq >= bg bg) to the sink with the background weight quantised the same way; qq is the predicate's.  No
 *              foreground point: count 0 and status GLIM_AMD_EDIT_NO_SEED.  Result: the points reachable from the source in the
 *              residual graph of a maximum flow (the two terminals are no points).  This is the minimal source side of a minimum cut,
 *              the same set for every maximum flow, hence independent of the order of pushes; a foreground point whose terminal arc is
 *              saturated and which no other residual path reaches is, by this definition, NOT in the set.  Solver: a round-based
 *              push-relabel without a deciding atomic (csrc/min_cut.hip), run from the background side; push rounds are enqueued
 *              GLIM_AMD_EDIT_ROUNDS_PER_LOOK at a time, each chunk is followed by an exact relabelling and one look of the host, and the
 *              call stops when no point with excess reaches absorbing capacity -- or after max_rounds push rounds with status
 *              GLIM_AMD_EDIT_ROUND_LIMIT, count 0 and no pairs.
 *   removal    a NEW cloud of the points whose index is not listed, in their original order (gtsam_points::sample with the surviving
 *              indices, :561); the input cloud is untouched.  Every per-point array the cloud holds (FP32 / FP64 points, covariances,
 *              normals, times, intensities, the host copy of the times) is gathered bit for bit; has-covariances, has-normals and the
 *              plane form are carried over; neighbour lists are dropped (their indices are stale); factor streams rebuild on first use.
 *              Indices in any order, duplicates allowed (:554 marks a slot twice without harm); an index outside [0, size) is refused --
 *              the `>` of :549 is an off-by-one and is not reproduced.
 * Deterministic: the same call returns the same bits.  Without a device every call returns GLIM_AMD_ERR_NO_DEVICE. */
#define GLIM_AMD_EDIT_BOX 0
#define GLIM_AMD_EDIT_SPHERE 1
#define GLIM_AMD_EDIT_WINDOW 2
#define GLIM_AMD_EDIT_WINDOW_BALL 3
#define GLIM_AMD_EDIT_ROUNDS_PER_LOOK 32 /* growth rounds enqueued between two looks of the host */
enum { GLIM_AMD_EDIT_OK = 0, GLIM_AMD_EDIT_EMPTY = 1 /* no candidate in the window */, GLIM_AMD_EDIT_FEW_POINTS = 2 /* fewer candidates than k */ };
/* min-cut segmentation only */
enum { GLIM_AMD_EDIT_NO_SEED = 3 /* no foreground point */, GLIM_AMD_EDIT_ROUND_LIMIT = 4 /* max_rounds push rounds did not finish the flow */ };
#define GLIM_AMD_EDIT_CAP_SCALE 65536       /* capacity units per unit of weight */
#define GLIM_AMD_EDIT_MIN_CUT_MAX_ROUNDS 65536 /* push rounds after which a call gives up (max_rounds = 0) */
typedef struct glim_amd_edit_window { /* points_selector.cpp:22-23 */
  double center[3];  /* the picked point */
  double resolution; /* map_cell_resolution, 2.0 */
  int32_t window;    /* cell_selection_window, 5 */
  int32_t reserved;  /* 0 */
} glim_amd_edit_window;
typedef struct glim_amd_edit_outlier_params { /* :35-37 */
  double radius_offset;  /* 1.0 */
  double stddev_thresh;  /* 2.0 */
  int32_t num_neighbors; /* 10 */
  int32_t reserved;      /* 0 */
} glim_amd_edit_outlier_params;
/* The three thresholds' defaults are a recollection of gtsam_points::RegionGrowingParams, which is not in the reference tree. */
typedef struct glim_amd_edit_region_growing_params {
  double distance_threshold;  /* 0.5 (recollection) */
  double cos_angle_threshold; /* cos(10 degrees) = 0.984807753012208 (recollection); the caller takes the cosine, once */
  double dilation_radius;     /* 0.5 (recollection); 0 = no dilation */
  int32_t use_normals;        /* 0 */
  int32_t max_hops;           /* 0 = unlimited */
} glim_amd_edit_region_growing_params;
typedef struct glim_amd_edit_region_result {
  int64_t count;          /* points of the cluster, whatever the capacity */
  int64_t num_candidates; /* points in the window */
  int32_t seed[2];        /* (sub-map, point); -1 -1 without a candidate */
  int32_t rounds;         /* growth rounds that assigned a point */
  int32_t status;         /* GLIM_AMD_EDIT_OK / GLIM_AMD_EDIT_EMPTY */
  double seed_qq;         /* squared distance of the seed to the picked point */
} glim_amd_edit_region_result;

/* matrices12: num_clouds x 12 -- T_local_submap for BOX / SPHERE (window may be NULL, radius is ignored), T_world_submap otherwise.
 * num_clouds may be 0 (count 0).  pairs: NULL with capacity 0, or capacity x 2 int32.  GLIM_AMD_ERR_INVALID: a NULL argument or handle,
 * num_clouds < 0, clouds of two contexts, an unknown mode, capacity < 0, a matrix or centre that is not finite, a resolution that is NaN,
 * infinite or <= 0, window < 0, (WINDOW_BALL) a radius that is NaN, infinite or <= 0, more than 2^31 - 257 points in all. */
int glim_amd_edit_select(const glim_amd_cloud* const* clouds, int32_t num_clouds, const double* matrices12, int32_t mode,
                         const glim_amd_edit_window* window, double radius, int64_t capacity, int32_t* pairs, int64_t* count);
/* select_outlier_points_radius (:703-759).  params NULL = the defaults; status may be NULL.  Also GLIM_AMD_ERR_INVALID: num_neighbors < 1, an
 * offset < 0 or a parameter that is not finite; GLIM_AMD_ERR_UNSUPPORTED: num_neighbors > 32. */
int glim_amd_edit_select_outliers(const glim_amd_cloud* const* clouds, int32_t num_clouds, const double* T_world_submap12,
                                  const glim_amd_edit_window* window, double radius, const glim_amd_edit_outlier_params* params, int64_t capacity,
                                  int32_t* pairs, int64_t* count, int32_t* status);
/* select_points_segmentation, region growing (:798-810).  params NULL = the defaults; levels: NULL, or capacity int32 (the level of each
 * returned pair).  Also GLIM_AMD_ERR_INVALID: a distance threshold that is NaN, infinite or <= 0, a dilation radius that is NaN, infinite
 * or < 0, a cosine that is NaN, max_hops < 0; GLIM_AMD_ERR_STATE: use_normals and a cloud without normals. */
int glim_amd_edit_region_grow(const glim_amd_cloud* const* clouds, int32_t num_clouds, const double* T_world_submap12,
                              const glim_amd_edit_window* window, const glim_amd_edit_region_growing_params* params, int64_t capacity,
                              int32_t* pairs, int32_t* levels, glim_amd_edit_region_result* out);
/* remove_selected_points (:537-562) for one sub-map.  indices: n entries (NULL with n 0).  *out: a new cloud of the same context, to be
 * destroyed by the caller.  GLIM_AMD_ERR_INVALID: a NULL cloud or output, n < 0, an index outside [0, size). */
int glim_amd_edit_remove_points(const glim_amd_cloud* cloud, int64_t n, const int32_t* indices, glim_amd_cloud** out);
/* The defaults marked "recollection" are a recollection of gtsam_points::MinCutParams, which is not in the reference tree. */
typedef struct glim_amd_edit_min_cut_params {
  double distance_sigma;         /* 0.25 (recollection) */
  double angle_sigma;            /* 10 degrees in radians, 0.17453292519943295 (recollection); used only with use_normals */
  double foreground_mask_radius; /* 0.5 (points_selector.cpp:43) */
  double background_mask_radius; /* 5.0 (:44) */
  double foreground_weight;      /* 10.0 (:42) */
  double background_weight;      /* 0 = the foreground weight */
  int32_t k_neighbors;           /* 20 (recollection); <= 31 */
  int32_t use_normals;           /* 0 */
  int32_t max_rounds;            /* 0 = GLIM_AMD_EDIT_MIN_CUT_MAX_ROUNDS */
  int32_t reserved;              /* 0 */
} glim_amd_edit_min_cut_params;
typedef struct glim_amd_edit_min_cut_result {
  int64_t count;          /* points of the segment, whatever the capacity */
  int64_t num_candidates; /* points in the ball */
  int64_t num_edges;      /* undirected edges of the neighbour graph */
  int64_t num_foreground; /* points tied to the source */
  int64_t num_background; /* points tied to the sink */
  int64_t flow;           /* the maximum flow in capacity units */
  int32_t rounds;         /* push rounds enqueued */
  int32_t looks;          /* chunks, i.e. exact relabellings after the first */
  int32_t status;         /* GLIM_AMD_EDIT_OK / _EMPTY / _FEW_POINTS / _NO_SEED / _ROUND_LIMIT */
  int32_t reserved;
} glim_amd_edit_min_cut_result;
/* select_points_segmentation, min-cut (:774-797).  params NULL = the defaults.  Also GLIM_AMD_ERR_INVALID: a parameter that is not finite,
 * a sigma <= 0, radii that are not 0 < foreground < background, a foreground weight <= 0, a background weight < 0, k_neighbors < 1,
 * max_rounds < 0, a weight whose quantised value does not fit 31 bits, more than 2^31 - 257 neighbour entries (candidates x (k + 1));
 * GLIM_AMD_ERR_UNSUPPORTED: k_neighbors > 31 (the kNN's limit of 32 with the query included); GLIM_AMD_ERR_STATE: use_normals and a cloud
 * that has points and no normals. */
int glim_amd_edit_min_cut(const glim_amd_cloud* const* clouds, int32_t num_clouds, const double* T_world_submap12,
                          const glim_amd_edit_window* window, const glim_amd_edit_min_cut_params* params, int64_t capacity, int32_t* pairs,
                          glim_amd_edit_min_cut_result* out);

/* ---- Resampling a resident cloud ------------------------------------------------------------------------------------------------------
 * gtsam_points::random_sampling (mapping/sub_mapping.cpp:385, global_mapping.cpp:248 / :734, global_mapping_pose_graph.cpp:263 / :268,
 * sub_mapping_passthrough.cpp:151, odometry_estimation_cpu.cpp:181), gtsam_points::sample (points_selector.cpp:561,
 * cloud_preprocessor.cpp:136) and gtsam_points::transform (odometry_estimation_cpu.cpp:184, sub_mapping_passthrough.cpp:75 / :147,
 * manual_loop_close_modal.cpp:332, loose_initial_state_estimation.cpp:77) on a cloud that is already on the device.  Each call returns a NEW
 * cloud of the input's context, to be destroyed by the caller; the input is never modified and may be destroyed before the result.
 *
 * The result carries every per-point array the input holds: the FP32 points, covariances and normals, the exact FP64 points, times,
 * intensities and FP64 covariances.  random_sample and sample gather them bit for bit, and "has covariances", "has normals" and the plane
 * form follow the input.  Neighbour lists are NOT carried over (their indices would be wrong), and whatever a cloud builds on first use is
 * built again for the result on its first use. */
/* The m = (int64)((double)size * rate) points with the smallest (sample_hash(seed, i) >> 32, i), compared lexicographically, in
 * ascending i; sample_hash is splitmix64 of seed + (i + 1) * 0x9E3779B97F4A7C15 (csrc/sample_hash.hpp).  This is the rule of the draw that
 * ends glim_amd_merge_frames.  rate >= 0.99 returns a copy of the whole cloud: upstream's own
 * shortcut AS RECALLED (gtsam_points' source is not in the reference tree; the guards at global_mapping.cpp:245 and
 * global_mapping_pose_graph.cpp:265 show the same constant).  m == 0 and an empty input give an empty cloud.
 * GLIM_AMD_ERR_INVALID: a NULL cloud or output, a rate that is NaN, infinite or < 0. */
int glim_amd_cloud_random_sample(const glim_amd_cloud* cloud, double rate, uint64_t seed, glim_amd_cloud** out);
/* out[j] = in[indices[j]] for j < m: any order, duplicates allowed, m may exceed the input's size (and may be 0, indices NULL).
 * GLIM_AMD_ERR_INVALID: a NULL cloud or output, m < 0 or m > 2^28, NULL indices with m > 0, an index outside [0, size). */
int glim_amd_cloud_sample(const glim_amd_cloud* cloud, int64_t m, const int32_t* indices, glim_amd_cloud** out);
/* T12: row-major 3 x 4 [L | t]; L need not be a rotation.  FP64 throughout, every product and sum rounded on its own, in this order:
 *   point       out_r = ((T[4r] p0 + T[4r+1] p1) + T[4r+2] p2) + T[4r+3] p3, and p3 is copied
 *   covariance  (L C) L^T, rows by columns, left to right, the upper triangle only
 *   normal      out_r = (T[4r] n0 + T[4r+1] n1) + T[4r+2] n2
 * Where the cloud holds FP64 points / covariances those are transformed and the FP32 arrays of the result are their roundings; where it
 * holds FP32 only, they are promoted, transformed and rounded.  Times and intensities are copied.  The plane form is decided anew on the
 * result's arrays, as an upload of them would.  A point that is not finite gives whatever the expressions give.
 * GLIM_AMD_ERR_INVALID: a NULL argument, an entry of T12 that is not finite. */
int glim_amd_cloud_transform(const glim_amd_cloud* cloud, const double* T12, glim_amd_cloud** out);

#ifdef __cplusplus
}
#endif
#endif /* GLIM_AMD_H */
