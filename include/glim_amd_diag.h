/*
 * glim_amd_diag.h -- measurement, test and tuning hooks of libglim_amd.so.  NOT part of the drop-in boundary.
 *
 * include/glim_amd.h is the stable C ABI a GLIM maintainer binds (every entry point there names the reference interface it replaces,
 * INTEGRATION.md 1).  Everything in THIS header has no counterpart in the reference: timing loops measured inside the library
 * (bench.py, tools/), counters, the diagnostic switches, debug views for the parity tests, failure injection.  Nothing under adapters/ or
 * examples/ includes it (tests/test_abi_cpu.py checks that), and a production build of GLIM never needs it.  Entry points may change
 * between versions without notice.
 */
#ifndef GLIM_AMD_DIAG_H
#define GLIM_AMD_DIAG_H

#include "glim_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- diagnostic / tuning switches ------------------------------------------------------------------------------ */
/* Diagnostic / tuning switches of a context (no counterpart in the reference; none is needed in production).  key_values:
 * "key=value,key=value"; NULL or "" restores the process defaults, which come from the ONE environment variable the library reads,
 * GLIM_AMD_DIAG (same syntax, parsed once per process).  Keys: knn_path=auto|brute (brute: the exhaustive kNN kernel answers
 * at every size), plane=0|1, curve_order=0|1, ppt=<n>, poll=0|1, inline_pose=0|1, bucket_factor=<n>, plan_cache=0|1, plan_recycle=0|1, host_poses=0|1, host_pack=0|1, pull_gated=0|1, frame_fused=0|1,
 * view_fused=0|1 (a voxel map built from a plane-form cloud gets its plane view -- the (C_B + I)^-1 records the plane-form factor kernel reads --
 * from the map's own finalise kernel; 0: on the first factor that needs it),
 * fuse=0|1 (small synchronous sets in ONE dispatch), host_rotate=0|1 (linearisations of the smallest such sets, and of a resident session's, return
 * raw sums and the host applies the R^T B R rotation of the record; 0: the device's finalisers do; same bits either way),
 * fin_pieces=0|1 (a resident session that returns raw sums finalises every factor in ten blocks, one per piece of the record, each thread waiting for
 * one granule of one row; 0: one block per factor; same bits either way, a live session is restarted when the switch flips), resident=0|1|auto + resident_idle_us=<n> (repeated synchronous linearisations of a small set
 * served by a resident kernel that leaves after <n> us without a request; auto, the default: only in a context created with priority 1 -- the
 * session costs whatever else runs on the device 1.3-1.4x while it is alive, so it is opt-in),
 * resident_post=lines|direct|auto (how a session gets its poses: request lines in host memory that its leader fetches and re-publishes on the device,
 * or granules the host stores straight into device memory through the large BAR; auto, the default: direct where the device's memory is host-visible
 * and the set is small, lines otherwise; same bits either way, a live session is restarted when the switch flips), pp_fast=0|1 (random-grid preprocessing without sorts),
 * small_rows=<n> (partial rows ONE factor of a small synchronous set is planned into at most; 0, the default: one per compute unit -- round 5: two),
 * knn_debug=<file>; and, in GLIM_AMD_DIAG ONLY (they are process-wide: set_diag refuses them), pool=0|1, multi_rccl=0|1,
 * multi_host_gather=0|1, multi_virtual=0|1 (glim_amd_multi_create accepts one physical device several times, see
 * glim_amd_debug_multi_create_virtual below).  Unknown keys / bad values: GLIM_AMD_ERR_INVALID and nothing changes.  get_diag prints the current state in the
 * same syntax. */
int glim_amd_ctx_set_diag(glim_amd_ctx* ctx, const char* key_values);
int glim_amd_ctx_get_diag(glim_amd_ctx* ctx, char* buf, size_t len);

/* ---- parity / debug views (host arithmetic or a single device pass; tests only) ------------------------------------- */
/* parity / debug only (host arithmetic, no device needed): the time table CloudDeskewing::deskew builds (cloud_deskewing.cpp:22-45 / :70-124) --
 * entry_out[i] = table entry of point i (n, may be NULL), table12_out = one row-major 3x4 T_lidar0_lidar1 per entry (table_cap entries, may
 * be NULL), *table_size = number of entries.  The deskewing kernels gather from exactly this table. */
int glim_amd_debug_deskew_table(int64_t n, const double* times, const double* T_imu_lidar12, int32_t n_imu, const double* imu_times, const double* imu_poses12,
                                double stamp, const double* linear_vel3, const double* angular_vel3, int32_t* entry_out, double* table12_out, int32_t table_cap,
                                int32_t* table_size);
/* parity / debug only (host arithmetic, no device work): what glim_amd_ct_gicp_* evaluates at (X, Y) -- *num_buckets = size of the factor's
 * time table; for the first table_cap buckets: table_out the normalised bucket times, T12_out row-major 3x4 T_k, D0_out / D1_out row-major
 * 6x6 dT_k/dX, dT_k/dY; time_index_out (source size) the bucket of every point.  Any output may be NULL. */
int glim_amd_debug_ct_gicp_poses(const glim_amd_ct_gicp_factor* factor, const double* X12, const double* Y12, int32_t* num_buckets, int32_t table_cap,
                                 double* table_out, double* T12_out, double* D0_out, double* D1_out, int32_t* time_index_out);
/* test hooks of the device iVox (glim_amd.h): the slot capacity its first insert allocates (default 1024; a tiny value forces the growth path of
 * the slot arrays and of the table; GLIM_AMD_ERR_STATE once the map has been inserted into), and the capacities it holds now. */
int glim_amd_debug_ivox_set_initial_capacity(glim_amd_ivox* ivox, int32_t slots);
int glim_amd_debug_ivox_capacity(const glim_amd_ivox* ivox, int32_t* slot_capacity, int32_t* table_size);
/* test hook: writes `value` into 32-bit word `word` (< 256) of the context's pinned scratch block -- what an earlier read-back (kNN counters, kept
 * points) may have left where the polled voxel-map builds keep their completion word (word 2; 4 * (levels - 1) + 2 for glim_amd_frame_create).
 * value = 0xffffffff stands for "the sequence number the context's NEXT polled build will wait for". */
int glim_amd_debug_scratch_poke(glim_amd_ctx* ctx, int32_t word, uint32_t value);
/* parity / debug only: the stable device radix sort behind the preprocessing (sorts by the low `bits` key bits; vals_in NULL = 0..n-1). */
int glim_amd_debug_sort_pairs(glim_amd_ctx* ctx, int64_t n, int32_t bits, const uint64_t* keys_in, const uint32_t* vals_in, uint64_t* keys_out,
                              uint32_t* vals_out);
/* parity / debug only: the device's exclusive prefix sum of 32-bit integers (csrc/scan.hpp) behind every stable compaction -- the map editor's
 * selections and removal, the ball selection, the kNN grid, the preprocessing: out[i] = in[0] + ... + in[i - 1], out[0] = 0, 32-bit wrap-around.
 * n == 0: GLIM_AMD_OK, nothing is touched.  GLIM_AMD_ERR_INVALID: a NULL context, n < 0, n > 2^28, a NULL array with n > 0. */
int glim_amd_debug_exclusive_scan(glim_amd_ctx* ctx, int64_t n, const int32_t* in, int32_t* out);
/* parity / debug only: the selection stage of the random sampling of a cloud (glim_amd.h; csrc/resample.hip) on a caller's 32-bit keys -- keep_out[i] = 1
 * iff (keys32[i], i) is among the m lexicographically smallest pairs, else 0.  Keys that tie at the threshold cannot be provoked through the
 * generator at test sizes; here they can.  n == 0: GLIM_AMD_OK, nothing is touched.  GLIM_AMD_ERR_INVALID: a NULL context, n < 0, n > 2^28,
 * m < 0, m > n, a NULL array with n > 0. */
int glim_amd_debug_select_smallest(glim_amd_ctx* ctx, int64_t n, const uint32_t* keys32, int64_t m, int32_t* keep_out);

/* The hypotheses [first, first + count) of glim_amd_ransac_align on the same arguments, every one scored, no early stop: samples (count x 3
 * source indices), status (count), poses12 (count x 12; the identity where status != 0), inliers (count; 0 where status != 0); any of them may
 * be NULL.  table_slots / table_in_lds: size of the occupancy table and whether the scoring kernel held it in LDS.  A source of 0 points is
 * GLIM_AMD_ERR_INVALID here (nothing to draw from). */
int glim_amd_ransac_debug_hypotheses(const glim_amd_cloud* target, const glim_amd_cloud* source, const int32_t* nearest,
                                     const glim_amd_ransac_params* params, int32_t first, int32_t count, int32_t* samples, int32_t* status,
                                     double* poses12, int32_t* inliers, int32_t* table_slots, int32_t* table_in_lds);
/* Largest occupancy table the RANSAC scoring kernel of THIS THREAD's calls copies into LDS, in slots (default and maximum 8192; 0: always probe
 * global memory).  Lets a test or a timing run take both forms on one input. */
int glim_amd_debug_ransac_max_lds_slots(int32_t slots);

/* glim_amd_gnc_align on the same arguments with every intermediate: the final list (list_pairs: source index, target index per entry, room for
 * list_capacity entries -- N_source, or 3 max_num_tuples with tuple_check, always suffices; GLIM_AMD_ERR_INVALID when the list is longer),
 * frame7 = c_s, c_t, D^2, iterations15 = per iteration of max_iterations the mu used, W, cost and the 12 pose doubles (only the first
 * result->iterations_run rows are written), weights = the weights of the last completed iteration, one per list entry (an iteration that ends the
 * loop without a finite result does not overwrite them).  Any output but result
 * and list_length may be NULL. */
int glim_amd_gnc_debug_trace(const glim_amd_cloud* target, const glim_amd_cloud* source, const int32_t* nearest, const glim_amd_gnc_params* params,
                             int64_t list_capacity, int32_t* list_pairs, int64_t* list_length, double* frame7, double* iterations15,
                             double* weights, glim_amd_registration_result* result, glim_amd_gnc_info* info);

/* ---- timing loops measured inside the library (bench.py, tools/) -------------------------------------------------- */
/* Timing aid used by bench.py: runs `iters` back-to-back launches bracketed by HIP events on the set's stream.
 * ms_vgicp_kernel: average duration of the fused lookup+residual+Jacobian+reduce kernel alone;
 * ms_linearize: average duration of the whole device-resident linearise (kernel + finalise). */
int glim_amd_factor_set_profile(glim_amd_factor_set* set, const double* T_target_source, int iters, float* ms_vgicp_kernel,
                                float* ms_linearize);
/* wall-clock milliseconds per synchronous glim_amd_factor_set_linearize call (pose upload, launches, result in host memory),
 * measured inside the library so that no binding overhead is included. */
int glim_amd_factor_set_profile_sync(glim_amd_factor_set* set, const double* T_target_source, int iters, float* ms_per_call);
/* timing aid: EXACTLY `iters` synchronous glim_amd_factor_set_linearize calls from C, no warm-up, no clock -- the caller times it.  Call i
 * linearises at pose set i % num_pose_sets of T_target_source (num_pose_sets x n x 12: an optimiser moves the poses between its
 * relinearisations); out_last (n records, may be NULL) receives the last call's result. */
int glim_amd_factor_set_linearize_repeat(glim_amd_factor_set* set, const double* T_target_source, int num_pose_sets, int iters,
                                         glim_amd_linearized6* out_last);
/* GLIM's live call pattern (odometry_estimation_gpu.cpp:383-385; the optimisers' linearisation hook does clear -> add(graph) -> linearize per
 * iteration): a FRESH factor set per linearisation -- create, add the n factors, synchronous linearize (poses T: n x 12), destroy -- `iters`
 * times; microseconds per iteration, measured inside the library. */
int glim_amd_factor_set_profile_fresh(glim_amd_ctx* ctx, int32_t n, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources,
                                      const uint32_t* flags, const double* T_target_source, int iters, float* us_per_iteration);
/* Measurement aid: wavefront trips of the general (36 B/pt) factor kernel that found no correspondence in any lane and skipped the record gather
 * and the algebra, summed over every evaluation of the set's current plan since the last reset, and the trips ONE evaluation of the plan makes
 * (blocks x 4 wavefronts x points per thread).  bench.py prices the kernel's instruction floor with the measured share instead of a constant. */
int glim_amd_factor_set_trip_stats(glim_amd_factor_set* set, uint64_t* skipped_trips, uint64_t* total_trips_per_evaluation, int reset);
/* The same pattern with every iteration timed on its own (samples_us: `iters` entries) and `gap_us` of host busy-waiting between iterations -- the
 * optimiser's own work between two linearisations --, for latency percentiles while other threads load the device (bench.py
 * --workload odometry_under_load). */
int glim_amd_factor_set_profile_fresh_samples(glim_amd_ctx* ctx, int32_t n, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources,
                                              const uint32_t* flags, const double* T_target_source, int iters, double gap_us, float* samples_us);
/* One Levenberg-Marquardt iteration as the optimisers drive it (sub_mapping.cpp:435-443, odometry_estimation_cpu.cpp:116-149): a synchronous
 * linearize() of the whole set (records expanded on the host) and a synchronous error() at the trial values, each timed over `iters` calls. */
int glim_amd_factor_set_profile_lm(glim_amd_factor_set* set, const double* T_target_source, int iters, float* ms_linearize, float* ms_error);
/* timing aid: `iters` calls of glim_amd_cloud_find_neighbors with this k; wall milliseconds per call, and the HIP-event duration (events on the call's own
 * stream) of the query-group kernel inside it -- the dominant kernel of the kNN-led workloads, whose roofline bench.py quotes (0 when another kernel
 * answered: clouds <= 2 048 points, knn_path=brute). */
int glim_amd_cloud_profile_neighbors(glim_amd_cloud* cloud, int k, int iters, float* ms_per_call, float* ms_qgroup_kernel);
/* timing aid: `iters` back-to-back glim_amd_overlap_batch calls with these arguments; microseconds per call, measured inside the library. */
int glim_amd_overlap_profile(glim_amd_ctx* ctx, int32_t num_queries, const int32_t* num_targets, const glim_amd_voxelmap* const* targets,
                             const double* T_target_source, const glim_amd_cloud* const* sources, int iters, float* us_per_call);

/* One RANSAC round (min(1024, max_iterations) hypotheses from 0) `iters` times after two warm-up rounds: mean microseconds of the hypothesis,
 * scoring and fold kernels by HIP events around each. */
int glim_amd_ransac_profile(const glim_amd_cloud* target, const glim_amd_cloud* source, const int32_t* nearest, const glim_amd_ransac_params* params,
                            int iters, float* us_hypothesis, float* us_score, float* us_fold, int32_t* table_slots, int32_t* table_in_lds);

/* glim_amd_gnc_align `iters` times after one warm-up call: mean microseconds, by HIP events, of the selection (mark, scan, compaction), the tuple
 * test (0 without tuple_check), the gather and the solve kernel, the occupancy table and the scoring of the final pose. */
int glim_amd_gnc_profile(const glim_amd_cloud* target, const glim_amd_cloud* source, const int32_t* nearest, const glim_amd_gnc_params* params,
                         int iters, float* us_select, float* us_tuples, float* us_solve, float* us_table, float* us_score);

/* ---- state of the resident session, the plan cache and the last frame_create ---------------------------------------- */
/* parity / debug only: the device's resident session (repeated synchronous linearisations of a small factor list are served by a kernel that stays
 * on the device and takes its requests through host-mapped memory; it leaves by itself after `resident_idle_us` without a request): kernel
 * launches and requests served so far, whether one is alive right now. */
int glim_amd_debug_resident_stats(int device, uint64_t* launches, uint64_t* requests, int32_t* alive);
/* ... and how its requests were posted so far (switch resident_post): granules stored by the host into device memory (direct), or request lines in
 * host memory (lines).  Either pointer may be NULL. */
int glim_amd_debug_resident_post_stats(int device, uint64_t* direct, uint64_t* lines);
/* Device timeline of the resident session's LAST request: ends the session, reports (us / num_fields may be NULL / 0: switch only)
 * and leaves the stamps on (enable != 0) or off for the sessions that start afterwards.  Microseconds, device stamps (s_memrealtime, 10 ns) relative
 * to the moment the session's leader saw the request in host memory (a session whose host posts the poses itself, resident_post=direct, has no such
 * moment and no re-publication: [1] is 0 there and everything is relative to the leader block seeing the pose in device memory, i.e. [11] is 0 too,
 * and the stamps sit earlier by the host -> device transit that [0] - [15] then contains in full):
 *   [0] host clock: posting the request -> last record granule seen      [1] leader: poses re-published on the device
 *   [2..4] worker blocks: pose seen, min / median / max   [5..7] first row computed   [8..10] row granules published
 *   [11] finaliser of factor 0: pose seen   [12] every row of its factor summed   [13] record stored towards the host
 *   [14] worker blocks with a complete account   [15] = [13]: the device's share of [0]
 *   [16..18] worker blocks: point loop left (before the wave / block reduction), min / median / max
 *   [19] finaliser: its 32 group sums added   [20] its 3x3 blocks rotated (the record store follows; = [19] for a raw record, which the host rotates)
 *   [21] NOT a time: the shader clock the session ran at between [11] and [13], MHz (s_memtime ticks per s_memrealtime microsecond)
 * A caller that passes more than GLIM_AMD_RESIDENT_TIMELINE_FIELDS fields also gets the account block by block (who is late, and where it runs):
 *   [22] blocks of the launch (B)   [23] its worker blocks (blocks 0 .. [23] - 1; the others finalise)
 *   [24 + 5 b + {0, 1, 2, 3}] block b: pose seen, first row computed, row granules published, point loop left; -1 where the block has no such
 *       stamp (a finalising block, a worker without a row)
 *   [24 + 5 b + 4] where block b runs: HW_REG_HW_ID + 2^32 * HW_REG_XCC_ID as the block read them (gfx9 HW_ID layout: compute unit in bits 8..11,
 *       shader array bit 12, shader engine from bit 13).  Two blocks share a compute unit when XCC_ID and bits 8..15 of HW_ID agree.
 *   GLIM_AMD_RESIDENT_TIMELINE_FIELDS + 2 + 5 * GLIM_AMD_RESIDENT_TIMELINE_MAX_BLOCKS fields hold every launch.
 * GLIM_AMD_ERR_STATE: a request is in flight, or no session has run with the stamps on. */
#define GLIM_AMD_RESIDENT_TIMELINE_FIELDS 22
#define GLIM_AMD_RESIDENT_TIMELINE_BLOCK_FIELDS 5
#define GLIM_AMD_RESIDENT_TIMELINE_MAX_BLOCKS 2048
int glim_amd_debug_resident_timeline(int device, int enable, double* microseconds, int32_t num_fields);
/* ends the device's resident session now instead of letting it idle out (GLIM_AMD_ERR_STATE while a request is in flight). */
int glim_amd_debug_resident_stop(int device);
/* parity / debug only: factor plans this context has built for new factor lists, how many of them took over the buffers of the plan its full
 * cache was about to evict (a new list of the same shape: GLIM's odometry brings one per frame), idle plans cached right now. */
int glim_amd_debug_plan_stats(glim_amd_ctx* ctx, uint64_t* built, uint64_t* recycled, int32_t* cached);
/* parity / debug only: calls of this process that went PAST the library's block caches to the runtime so far -- hipMalloc, hipFree, hipHostMalloc --
 * and the bytes the calling thread's current device holds in its cache of freed blocks.  A steady-state loop should add none (a real allocation
 * stalls everything on the device, not only its caller: tools/odometry_frame_loop.cpp reports the count per slow frame).  Any pointer may be NULL. */
int glim_amd_debug_pool_stats(uint64_t* device_mallocs, uint64_t* device_frees, uint64_t* pinned_mallocs, uint64_t* cached_bytes);
/* measurement only: hipStreamQuery on every stream of the context (how many still have work: *busy).  tools/odometry_frame_loop.cpp uses it to
 * ask whether the runtime retires its finished commands when a loop that only ever POLLS completion words looks at its streams now and then. */
int glim_amd_debug_ctx_query_streams(glim_amd_ctx* ctx, int32_t* busy);
/* parity / debug only: host-side account of the calling thread's LAST one-submission glim_amd_frame_create, microseconds since its entry:
 * [0] cloud allocated, [1] staging block + stream allocations, [2] pull kernel launched, [3] host conversion done, [4] voxel-map kernels
 * enqueued, [5] completion word seen, [6] return (tools/odometry_frame_loop.cpp prints the medians). */
int glim_amd_debug_frame_stages(double* microseconds, int32_t num_fields);

/* ---- multi-device evaluation: measurement, knobs, virtual devices, failure injection ---------------------------------- */
/* wall-clock milliseconds per whole-cost evaluation (all devices + collective + host expansion skipped), over `iters` evaluations */
int glim_amd_multi_profile(glim_amd_multi* multi, const double* T_target_source, int iters, float* ms_per_evaluation);
/* per device, HIP-event milliseconds of the LAST evaluation: its factor kernels + finalise (kernel_ms[d]) and the collective + copy-out behind
 * them (gather_ms[d]); num_devices entries each, either may be NULL */
int glim_amd_multi_last_timing(const glim_amd_multi* multi, float* kernel_ms, float* gather_ms);
/* host-side account of the LAST evaluation on one device's thread, microseconds, GLIM_AMD_MULTI_BREAKDOWN_FIELDS values:
 *   [0] post        caller: handing the evaluation to the other devices' threads          (device 0 only)
 *   [1] wake        from the caller's entry to the start of this device's task            (0 for device 0: the caller's own thread)
 *   [2] pose_stage  this shard's poses copied into the pinned ring
 *   [3] enqueue     plan check + H2D pose copy + kernel launches
 *   [4] barrier     waiting until every device has enqueued (no collective starts before)
 *   [5] collective  ncclAllGather calls + copy-out enqueue
 *   [6] wait        hipStreamSynchronize: the device working
 *   [7] join        caller: waiting for the other devices' threads                        (device 0 only)
 *   [8] scan        caller: total error + expansion of the records in factor order        (device 0 only)
 *   [9] total       the whole glim_amd_multi_linearize call                                (device 0 only)
 *   [10] library_calls   inside the ncclAllGather calls (part of [5])
 *   [11] device_gather   HIP events: from this device's last kernel to the end of its last all-gather
 *   [12] device_copy_out HIP events: from there to the end of the copy-out and the error sum  ([11] + [12] = gather_ms of last_timing) */
#define GLIM_AMD_MULTI_BREAKDOWN_FIELDS 13
int glim_amd_multi_last_breakdown(const glim_amd_multi* multi, int32_t device, double* microseconds, int32_t num_fields);
/* how a device's shard is evaluated: n >= 2 = as n pieces (at most 8), the all-gather and copy-out of one piece overlapping the kernels of
 * the next; 0 or 1 = as one set and one all-gather; -1 (default) = pieces of at least 2048 factors, at most 4.  Takes effect with the next
 * glim_amd_multi_set_factors. */
int glim_amd_multi_set_split(glim_amd_multi* multi, int32_t mode);
/* ONE device has nothing to gather, so its evaluations make no library call; the binding is exercised when the handle is created (an in-place
 * one-rank all-gather that must come back unchanged; glim_amd_multi_info uses_rccl says whether it did).  on != 0: make the no-op
 * ncclAllGather in every evaluation as well (measurement aid: bench.py prices it).  No effect on several devices. */
int glim_amd_multi_set_one_rank_collective(glim_amd_multi* multi, int32_t on);
/* how every device's own records reach the host array (glim_amd_multi_records, the `out` of glim_amd_multi_linearize): 1 (default) = its
 * finalising kernels store them there as well (host-mapped memory, 232 B per factor over the device's PCIe link while the launch runs: nothing
 * is copied behind the kernels); 0 = device-to-host copies on the collective's stream behind each piece.  Takes effect with the next
 * glim_amd_multi_set_factors. */
int glim_amd_multi_set_host_records(glim_amd_multi* multi, int32_t mode);
/* The N > 1 path on a box with ONE GPU ("virtual devices"): like glim_amd_multi_create, but a device ordinal may be listed several times.  Every
 * entry gets its own context, host thread, shard, pieces, upload / collective streams and gathered array; RCCL refuses one device twice, so the
 * exchange of a piece is a same-device stand-in for the in-place ncclAllGather -- every entry copies its slot into the others' arrays on its
 * collective stream, behind the piece's event (distinct devices still go through ncclCommInitAll / ncclAllGather).  The same happens in
 * glim_amd_multi_create itself when GLIM_AMD_DIAG holds multi_virtual=1.  glim_amd_multi_info reports uses_rccl = 0 for such a handle. */
int glim_amd_debug_multi_create_virtual(const int32_t* devices, int32_t num_devices, glim_amd_multi** out);
/* failure injection, one shot: the NEXT glim_amd_multi_linearize fails on `device` (index into the handle's list) -- where = 1: before the host
 * barrier (its kernels are never enqueued; no device starts an exchange, every thread returns the error, the handle stays usable); where = 2:
 * inside its exchange of the last piece (the others are in theirs: the communicators are aborted and the handle is retired -- every later
 * evaluation returns GLIM_AMD_ERR_STATE).  where = 0 or device = -1 disarms. */
int glim_amd_debug_multi_inject_failure(glim_amd_multi* multi, int32_t device, int32_t where);
/* glim_amd_ctx_set_diag on every context of the handle (e.g. "ppt=16": the same points-per-thread rule -- hence the same per-factor block
 * partition and the same bits -- as an unsharded set evaluated with that switch) */
int glim_amd_debug_multi_set_diag(glim_amd_multi* multi, const char* key_values);
/* the DEVICE-resident gathered array of `device` after the exchange, copied back and put in factor order like glim_amd_multi_records: what a
 * device-side consumer on that device would read (tests: every device must hold every record, bit for bit) */
int glim_amd_debug_multi_gathered_download(glim_amd_multi* multi, int32_t device, int64_t first, int64_t count, double* compact29);
/* test window of the GICP fine registration (glim_amd.h "GICP fine registration"): the search-index entry point when ivox = 0 (targets are
 * glim_amd_nn_index handles), the iVox one when ivox = 1 (glim_amd_ivox handles), with the same arguments and results, plus one
 * entry per problem and round: trace[i * (1 + max_trials) + r], max_trials as resolved (0 = 2 x max_iterations).  Round 0 is the initial pose;
 * the entries of problem i are valid for r <= out[i].trials, the rest are zero. */
typedef struct {
  double T_candidate[12]; /* the pose the round evaluated */
  double lambda;          /* the lambda its step was solved with (lambda_initial in round 0) */
  double compact[29];     /* the record there */
  int32_t accepted;
  int32_t status;         /* after the round; 0 = still running */
} glim_amd_align_trace_entry;
int glim_amd_debug_gicp_align_trace(int32_t ivox, const void* const* targets, const glim_amd_cloud* const* sources, const double* T_init12,
                                    const double* max_correspondence_distances, int32_t count, const glim_amd_lm_params* params,
                                    glim_amd_align_result* out, glim_amd_align_trace_entry* trace);
/* test window of the ICP fine registration (glim_amd.h "ICP fine registration"): glim_amd_icp_align_batch with the same arguments and results,
 * plus trace[i * (1 + max_trials) + r] as above, and the number of rounds enqueued between two looks at the statuses (0 = the call's own 41;
 * any value >= 1 + max_trials enqueues every round up front).  The chunk length moves no bit of `out` or `trace`. */
int glim_amd_debug_icp_align_trace(const glim_amd_nn_index* const* targets, const glim_amd_cloud* const* sources, const double* T_init12,
                                   const double* max_correspondence_distances, uint32_t flags, int32_t count, const glim_amd_lm_params* params,
                                   glim_amd_align_result* out, glim_amd_align_trace_entry* trace, int32_t rounds_per_chunk);
/* test window of the VGICP fine registration (glim_amd.h "VGICP fine registration"): glim_amd_vgicp_align_batch with the same arguments and
 * results, plus trace[i * (1 + max_trials) + r] as above */
int glim_amd_debug_vgicp_align_trace(const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources, const double* T_init12,
                                     uint32_t flags, int32_t count, const glim_amd_lm_params* params, glim_amd_align_result* out,
                                     glim_amd_align_trace_entry* trace);
/* test window of the CT-GICP frame alignment (glim_amd.h): the same call plus one entry per round, trace[r] for r < 1 + max_trials (max_trials
 * as resolved).  Round 0 is the initial pair; entries are valid for r <= out->trials, the rest are zero. */
typedef struct {
  double X[12];       /* the pair the round evaluated */
  double Y[12];
  double lambda;      /* the lambda its step was solved with (lambda_initial in round 0) */
  double record[92];  /* the factor's record there: num_inliers, error, 78 upper entries of the 12 x 12 H (row-major), 12 of b */
  double cost;        /* the total cost there */
  int32_t accepted;
  int32_t status;     /* after the round; 0 = still running */
} glim_amd_ct_align_trace_entry;
int glim_amd_debug_ct_align_trace(glim_amd_ct_gicp_factor* factor, const double* X_init12, const double* Y_init12, const glim_amd_ct_align_terms* terms,
                                  const glim_amd_lm_params* params, glim_amd_ct_align_result* out, glim_amd_ct_align_trace_entry* trace);
/* the pose table kernel of the CT-GICP frame alignment alone at (X, Y): T_k | D0_k | D1_k as the device computes them, `table_cap` buckets at
 * most (12 / 36 / 36 doubles each; any output may be NULL).  The host's table is glim_amd_debug_ct_gicp_poses. */
int glim_amd_debug_ct_align_poses(glim_amd_ct_gicp_factor* factor, const double* X12, const double* Y12, int32_t* num_buckets, int32_t table_cap,
                                  double* T12_out, double* D0_out, double* D1_out);
/* test window of the sub-map bundle optimisation (glim_amd.h): glim_amd_bundle_align with the same arguments and results, plus, per round
 * r < 1 + max_trials (max_trials as resolved; round 0 is the initial poses; valid for r <= result->trials, the rest are zero):
 * X_trace[r] (num_poses x 12, the candidate poses the round evaluated), Tf_trace[r] (num_factors x 12, the relative poses as the device computed
 * them), compact_trace[r] (num_factors x 29, the records there) and rounds[r].  one_thread != 0: the decide step is bundle_lm_step.hpp's step()
 * run by ONE device thread, the cross-check of the workgroup form (same bits); it is no production path. */
typedef struct {
  double lambda;      /* the lambda the round's step was solved with (lambda_initial in round 0) */
  double cost;        /* the total cost the round's evaluation gave */
  int32_t accepted;
  int32_t status;     /* after the round; 0 = still running */
} glim_amd_bundle_trace_round;
int glim_amd_debug_bundle_align_trace(glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources,
                                      const int32_t* target_pose, const int32_t* source_pose, int32_t num_factors, uint32_t flags,
                                      const glim_amd_bundle_prior* priors, int32_t num_priors, const glim_amd_bundle_between* betweens,
                                      int32_t num_betweens, const double* X_init12, int32_t num_poses, const glim_amd_lm_params* params,
                                      double* X_out12, double* compact_out, glim_amd_bundle_result* result, int32_t one_thread, double* X_trace,
                                      double* Tf_trace, double* compact_trace, glim_amd_bundle_trace_round* rounds);
/* test window of the global-graph optimisation (glim_amd.h): glim_amd_graph_align with the same arguments and results and the trace arrays of
 * glim_amd_debug_bundle_align_trace, plus two arguments.  rounds_per_chunk: how many rounds are enqueued between two looks at the status (0: the
 * default; it moves no bit of a result).  one_thread != 0: every round is bundle_lm_step.hpp's step() as it stands, run by ONE device thread with
 * its working system in device memory -- the cross-check of the launches (same bits); it is no production path and takes seconds beyond a few
 * dozen poses. */
int glim_amd_debug_graph_align_trace(glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources,
                                     const int32_t* target_pose, const int32_t* source_pose, int32_t num_factors, uint32_t flags,
                                     const glim_amd_bundle_prior* priors, int32_t num_priors, const glim_amd_bundle_between* betweens,
                                     int32_t num_betweens, const double* X_init12, int32_t num_poses, const glim_amd_lm_params* params,
                                     double* X_out12, double* compact_out, glim_amd_bundle_result* result, int32_t one_thread, double* X_trace,
                                     double* Tf_trace, double* compact_trace, glim_amd_bundle_trace_round* rounds, int32_t rounds_per_chunk);
/* the two test windows above for the entry points with damping terms and Huber between terms (glim_amd.h "Damping terms and Huber between
 * terms"): the same trace arrays and switches behind the two further arguments of those entry points */
int glim_amd_debug_bundle_align_terms_trace(glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources,
                                            const int32_t* target_pose, const int32_t* source_pose, int32_t num_factors, uint32_t flags,
                                            const glim_amd_bundle_prior* priors, int32_t num_priors, const glim_amd_bundle_between* betweens,
                                            int32_t num_betweens, const double* X_init12, int32_t num_poses, const glim_amd_lm_params* params,
                                            double* X_out12, double* compact_out, glim_amd_bundle_result* result, const glim_amd_graph_terms* more,
                                            double* between_weight_out, int32_t one_thread, double* X_trace, double* Tf_trace, double* compact_trace,
                                            glim_amd_bundle_trace_round* rounds);
int glim_amd_debug_graph_align_terms_trace(glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources,
                                           const int32_t* target_pose, const int32_t* source_pose, int32_t num_factors, uint32_t flags,
                                           const glim_amd_bundle_prior* priors, int32_t num_priors, const glim_amd_bundle_between* betweens,
                                           int32_t num_betweens, const double* X_init12, int32_t num_poses, const glim_amd_lm_params* params,
                                           double* X_out12, double* compact_out, glim_amd_bundle_result* result, const glim_amd_graph_terms* more,
                                           double* between_weight_out, int32_t one_thread, double* X_trace, double* Tf_trace, double* compact_trace,
                                           glim_amd_bundle_trace_round* rounds, int32_t rounds_per_chunk);
/* the same for the entry point of include/glim_amd.h "Graph optimisation with velocity and bias variables": the trace's X rows are node
 * values.  one_thread: every round is bundle_lm_step.hpp's step() in one device thread, the new terms included */
int glim_amd_debug_graph_align_nav_trace(glim_amd_ctx* ctx, const glim_amd_voxelmap* const* targets, const glim_amd_cloud* const* sources,
                                         const int32_t* target_pose, const int32_t* source_pose, int32_t num_factors, uint32_t flags,
                                         const glim_amd_bundle_prior* priors, int32_t num_priors, const glim_amd_bundle_between* betweens,
                                         int32_t num_betweens, const double* X_init12, int32_t num_poses, const glim_amd_lm_params* params,
                                         double* X_out12, double* compact_out, glim_amd_nav_result* result, const glim_amd_graph_terms* more,
                                         double* between_weight_out, const glim_amd_nav_terms* nav, int32_t one_thread, double* X_trace,
                                         double* Tf_trace, double* compact_trace, glim_amd_bundle_trace_round* rounds, int32_t rounds_per_chunk);
/* the device's blocked solve alone (glim_amd/csrc/graph_solve.hpp) on a caller's system: S is the packed lower triangle of H by rows (row i at
 * i (i + 1) / 2), then b; 1 <= n <= 6 GLIM_AMD_GRAPH_MAX_POSES.  Solves (H + lambda I) delta = -b.  delta_out: n doubles, +0.0 after a failed
 * pivot; *ok_out: 1, or 0 after a failed pivot. */
int glim_amd_debug_graph_solve(glim_amd_ctx* ctx, const double* S, int32_t n, double lambda, double* delta_out, int32_t* ok_out);
/* test window of the scan-to-keyframes VGICP registration (glim_amd.h): glim_amd_keyframe_align_batch with the same arguments and results,
 * plus, with R = 1 + max_trials rounds (max_trials as resolved; round 0 is the initial pose; valid for r <= out[i].trials, the rest are zero):
 * per problem i and round r, rounds[i * R + r] -- T_candidate: the X the round evaluated, lambda: the one its step was solved with, compact:
 * the SUMMED record (prior included), accepted, status -- and prior_trace[(i * R + r) * 28 ..]: the prior's contribution, the 21 upper entries
 * of J^T L J, the 6 of J^T L r, then r^T L r (zero without a prior); per round r and factor f of the batch, Tf_trace[(r * F + f) * 12 ..]: T_f as
 * the device computed it, and compact_trace[(r * F + f) * 29 ..]: the factor's record there.  All four arrays are required. */
int glim_amd_debug_keyframe_align_trace(const glim_amd_cloud* const* sources, const int32_t* first_target, const glim_amd_voxelmap* const* targets,
                                        const double* T_world_target12, const double* X_init12, const glim_amd_bundle_prior* priors,
                                        int32_t num_priors, uint32_t flags, int32_t count, const glim_amd_lm_params* params, glim_amd_align_result* out,
                                        double* factor_compact_out, glim_amd_align_trace_entry* rounds, double* prior_trace, double* Tf_trace,
                                        double* compact_trace);
/* test window of the radius search of the plane bundle-adjustment tool (glim_amd.h): glim_amd_ba_auto_radius with the same arguments and
 * result, plus one entry per evaluation in `entries` (1 + GLIM_AMD_BA_MAX_TRIALS of them; *num_entries are filled): entry 0 is r0, entry i
 * the i-th trial.  An entry whose decision is GLIM_AMD_BA_TRACE_RANGE was not evaluated: its count is -1 and its eigenvalues are NaN. */
enum {
  GLIM_AMD_BA_TRACE_INITIAL = 0,    /* r0: always kept */
  GLIM_AMD_BA_TRACE_TAKEN = 1,      /* the trial became the current radius */
  GLIM_AMD_BA_TRACE_RANGE = 2,      /* outside [min_radius, max_radius]: the search stopped */
  GLIM_AMD_BA_TRACE_FEW_POINTS = 3, /* fewer than 10 points: stopped */
  GLIM_AMD_BA_TRACE_PLANE_EPS = 4   /* larger than r0 and lambda_0 / lambda_2 > plane_eps: stopped */
};
typedef struct {
  double radius;
  int64_t count;
  double eigenvalues[3];
  int32_t decision;
  int32_t reserved;
} glim_amd_ba_trace_entry;
int glim_amd_debug_ba_auto_radius_trace(const glim_amd_cloud* const* clouds, int32_t num_clouds, const double* T_world_submap12,
                                        const double* center3, double radius0, const glim_amd_ba_params* params,
                                        glim_amd_ba_radius_result* out, glim_amd_ba_trace_entry* entries, int32_t* num_entries);
/* the eigen-solver of the plane bundle-adjustment statistics and factors (csrc/eig3_direct.hpp) run by one device thread per matrix:
 * m9: count x 9 row-major symmetric; evals: count x 3 ascending; evecs: count x 9, evecs[3 k + r] = component r of eigenvector k */
int glim_amd_debug_ba_eigen3(glim_amd_ctx* ctx, int32_t count, const double* m9, double* evals, double* evecs);
/* the SE(3) maps and pose-graph terms every on-device optimiser is built from (csrc/ct_se3.hpp), one routine at a time, one device thread per
 * case (blocks of 64): in: count x IN doubles, out: count x OUT doubles.  Poses are row-major 3 x 4, tangents (omega, v), 6 x 6 row-major.
 *   op 0 exp              IN  6 xi              OUT 12 T
 *   op 1 log              IN 12 T               OUT  6 xi
 *   op 2 jr               IN  6 xi              OUT 36 J_r(xi)
 *   op 3 jr_inv           IN  6 xi              OUT 36 J_r(xi)^-1
 *   op 4 ad               IN 12 T               OUT 36 Ad(T)
 *   op 5 prior_residual   IN 24 P | X           OUT 42 r = Log(P^-1 X) | d r / d X (6 x 6)
 *   op 6 between_residual IN 36 D | X | Y       OUT 78 r = Log(D^-1 X^-1 Y) | [d r / d X | d r / d Y] (6 x 12)
 *   op 7 ct_pose_bucket   IN 25 X | Y | t_k     OUT 84 T_k | D0_k | D1_k
 * GLIM_AMD_ERR_INVALID: a NULL context or array, count < 0, any other op.  count == 0: GLIM_AMD_OK, nothing is launched. */
int glim_amd_debug_se3_eval(glim_amd_ctx* ctx, int32_t op, int32_t count, const double* in, double* out);
/* test window of the map editor's min-cut segmentation (glim_amd.h): the graph glim_amd_edit_min_cut builds from the same inputs, before any
 * flow.  pairs: the candidates, pair_capacity x 2; source_cap / sink_cap: pair_capacity entries, the terminal capacity of every candidate (0:
 * not tied); edges: edge_capacity x 2 candidate indices (i < j) in ascending key order; edge_cap: edge_capacity capacities.  At most the
 * capacities are written, the first entries; out: the true counts and the status (EMPTY / FEW_POINTS / NO_SEED as for the call, else OK);
 * count, flow, rounds and looks are 0.  Any array may be NULL with its capacity 0. */
int glim_amd_diag_edit_min_cut_graph(const glim_amd_cloud* const* clouds, int32_t num_clouds, const double* T_world_submap12,
                                     const glim_amd_edit_window* window, const glim_amd_edit_min_cut_params* params, int64_t pair_capacity,
                                     int32_t* pairs, int32_t* source_cap, int32_t* sink_cap, int64_t edge_capacity, int32_t* edges,
                                     int32_t* edge_cap, glim_amd_edit_min_cut_result* out);
/* the solver of the min-cut segmentation (csrc/min_cut.hip) alone, on a caller's graph of n nodes: num_edges undirected edges (i, j), i != j,
 * both in [0, n), parallel edges allowed, with capacities edge_cap >= 0 in both directions; source_cap / sink_cap >= 0 per node.  member: n
 * flags, 1 iff the node is reachable from the source in the residual graph of a maximum flow.  max_rounds 0 = the default.  status:
 * GLIM_AMD_EDIT_OK or GLIM_AMD_EDIT_ROUND_LIMIT (every flag 0, flow 0).  GLIM_AMD_ERR_INVALID: a NULL context or output, n < 0 or num_edges < 0
 * or either above 2^30, an endpoint out of range, a loop, a negative capacity, max_rounds < 0. */
int glim_amd_diag_max_flow(glim_amd_ctx* ctx, int32_t n, int64_t num_edges, const int32_t* edges, const int32_t* edge_cap,
                           const int32_t* source_cap, const int32_t* sink_cap, int32_t max_rounds, int32_t* member, int64_t* flow,
                           int32_t* rounds, int32_t* looks, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* GLIM_AMD_DIAG_H */
