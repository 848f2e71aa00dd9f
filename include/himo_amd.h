/*
 * himo_amd.h -- C ABI of libhimo_amd.so: the MI355X (gfx950) motion-compensation hot path
 * of KTH-RPL/HiMo.
 *
 * The reference has no native layer: its per-frame path is numpy code
 * inside two Python loops.  This ABI is what a maintainer of the reference would bind with
 * ctypes to replace that arithmetic (binding shown in INTEGRATION.md).  Each entry point
 * cites the reference lines it replaces (paths relative to /root/reference).
 *
 * Conventions
 *   - plain C types only; every `d_*` pointer is DEVICE memory (HBM), every `h_*` pointer is
 *     HOST memory; the caller owns all buffers, the library never allocates or frees;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); every call is
 *     asynchronous on that stream unless stated, re-entrant per stream, and holds no global
 *     state;
 *   - row-major arrays; point rows are `pc_stride` floats apart (3 = xyz, 4 = xyzi as the
 *     reference's `pc0`); 16-byte aligned base pointers take the vectorised path;
 *   - every function returns a himo_status; HIMO_OK == 0.  The Python host layer turns a
 *     non-zero status into the exception the reference would raise (ValueError / KeyError).
 */
#ifndef HIMO_AMD_H
#define HIMO_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIMO_ABI_VERSION 1

typedef enum himo_status {
    HIMO_OK = 0,
    HIMO_ERR_INVALID_ARGUMENT = 1, /* NULL where data is required, negative sizes, bad stride */
    HIMO_ERR_EMPTY_FRAME = 2,      /* reference: `max()` of an empty lidar_dt raises ValueError (save_zip.py:120) */
    HIMO_ERR_WORKSPACE = 3,        /* workspace smaller than himo_*_workspace_bytes() */
    HIMO_ERR_SINGULAR_POSE = 4,    /* reference: np.linalg.inv raises LinAlgError (save_zip.py:115) */
    HIMO_ERR_HIP = 5,              /* a HIP runtime call failed; see himo_last_hip_error() */
    HIMO_ERR_UNSUPPORTED = 6
} himo_status;

/* flags for the comp_dis entry points */
#define HIMO_FLAG_F32_CHAIN 0x1u /* do the arithmetic in float32: what numpy does when the poses are
                                    float32 (dataprocess/extract_sca.py:232); default is the float64
                                    chain numpy runs for float64 poses, rounded to f32 at the end
                                    exactly where save_zip.py:70-72 casts */
#define HIMO_FLAG_RAW 0x2u       /* res_name == "raw": est_flow = zeros (save_zip.py:117) */
#define HIMO_FLAG_SCANIA 0x4u    /* eval mask also requires flow_is_valid (eval.py:293-294) */
#define HIMO_FLAG_POSE_IS_EGO 0x8u /* `pose0` already holds ego_pose = inv(pose1) @ pose0 (save_zip.py:115,
                                    computed by the caller, e.g. with numpy); `pose1` is ignored / may be NULL */

int himo_abi_version(void);
/* sizeof(struct) for "himo_conv_desc" | "himo_op" | "himo_sweep" | "himo_instance_record" (0 for an unknown name): lets
 * a binding verify its mirror of the structs that cross the boundary by address */
size_t himo_abi_sizeof(const char* struct_name);
const char* himo_status_string(int status);
/* text of the last HIP error seen by this thread (empty string if none) */
const char* himo_last_hip_error(void);

/* Optional per-kernel timing (used by bench.py for the roofline figure): while enabled, every
 * kernel launch of this library is bracketed by two HIP events on its own stream.
 * himo_prof_summary waits for the recorded launches and writes one line per kernel name:
 * "<name> <count> <total_ms> <min_ms> <max_ms>\n"; returns the bytes needed (incl. NUL). */
void himo_prof_enable(int on);
/* time only kernels whose name contains `substr` (NULL or "" = all): keeps the event records out of the other launches */
void himo_prof_filter(const char* substr);
void himo_prof_reset(void);
size_t himo_prof_summary(char* buf, size_t cap);
/* Diagnostic: the matrix-instruction rate the device sustains on its own -- independent v_mfma chains from registers on every
 * SIMD, no memory traffic, for about `min_seconds` (half of it untimed, to reach the power-managed clock).  kind 0: fp16
 * 32x32x16, 1: bf16 32x32x16, 2: float32 32x32x2; `zero_operands` != 0 feeds all-zero operands (the clock, hence the rate,
 * depends on the operand bits).  Synchronous.  Writes TFLOP/s to *tflops. */
int himo_mfma_sustained_tflops(int kind, int zero_operands, double min_seconds, double* tflops, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a1-a4 (+a5/a6): flow -> per-point de-distortion offsets, batched over ragged frames.
 *
 * Replaces, per frame f with rows [offsets[f], offsets[f+1]):
 *     ego_pose  = inv(pose1) @ pose0                                   save_zip.py:115  eval.py:284
 *     pose_flow = pc0[:, :3] @ ego_pose[:3,:3].T + ego_pose[:3,3] - pc0[:, :3]    save_zip.py:116
 *     est_flow  = flow - pose_flow            (zeros when RAW)          save_zip.py:117
 *     dt0       = max(lidar_dt) - lidar_dt                             save_zip.py:120
 *     comp_dis  = est_flow / sensor_dt * dt0[:, None]    utils/__init__.py:43, save_zip.py:121
 *     refined   = pc0[:, :3] + comp_dis                  utils/__init__.py:46     (optional)
 *     eval_mask = |pc0.xy| <= close_distance & ~gm0 & ego_pts_mask(pc0) [& flow_is_valid]
 *                                                         eval.py:288-296         (optional)
 *
 * d_offsets   int64[n_frames+1], non-decreasing, offsets[0] == 0, offsets[n_frames] == total_points
 * d_pose0/1   double[n_frames][16], row-major 4x4 (`pose0`, `pose1` of the frame dict)
 * d_pc0       float[total_points][pc_stride]; d_flow float[total_points][3] (ignored when RAW);
 * d_lidar_dt  float[total_points]
 * d_comp_dis  float[total_points][3]  (out)
 * d_refined   float[total_points][3]  (out, may be NULL)
 * d_eval_mask uint8[total_points]     (out, may be NULL; then the four arguments below are unused)
 * d_gm0, d_flow_is_valid  uint8/bool[total_points]  (d_flow_is_valid may be NULL unless SCANIA)
 * mask_bounds float[6] HOST: ego box min xyz, max xyz (utils/__init__.py:26; eval.py:296)
 * d_workspace at least himo_compdis_workspace_bytes(n_frames) bytes, 16-byte aligned.
 *
 * Frames with zero points are skipped (the single-frame wrapper reports HIMO_ERR_EMPTY_FRAME).
 * NaN entries of lidar_dt are ignored by the max.  A singular pose1 yields NaN outputs for that
 * frame (the single-frame wrapper reports HIMO_ERR_SINGULAR_POSE instead).
 */
size_t himo_compdis_workspace_bytes(int n_frames);

int himo_compdis_batch(int n_frames, int64_t total_points,
                       const int64_t* d_offsets, const double* d_pose0, const double* d_pose1,
                       const float* d_pc0, int pc_stride, const float* d_flow, const float* d_lidar_dt,
                       double sensor_dt, unsigned flags,
                       float* d_comp_dis, float* d_refined,
                       uint8_t* d_eval_mask, const uint8_t* d_gm0, const uint8_t* d_flow_is_valid,
                       const float* h_mask_bounds, float close_distance,
                       void* d_workspace, size_t workspace_bytes, void* stream);

/* One frame with host-side scalars: the body of the loop at save_zip.py:112-121.  Uploads the two
 * poses into the workspace (a small blocking copy), then runs the batch path with n_frames = 1. */
int himo_compdis_frame(int64_t n_points, const double* h_pose0, const double* h_pose1,
                       const float* d_pc0, int pc_stride, const float* d_flow, const float* d_lidar_dt,
                       double sensor_dt, unsigned flags,
                       float* d_comp_dis, float* d_refined,
                       void* d_workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Ground-truth sweeps (tools/test/save_zip_gt.py:141-178): the same chain with est_flow = `flow` - pose_flow, written as
 * the BODY of one Arrow record batch per sweep -- the sweep's Feather file is head + body + tail with the framing a function
 * of the schema and the row count alone.  Columns, in file order, each starting at a multiple of 8 bytes with zero pad bytes
 * and no validity buffers:
 *     comp_dis_x_m, comp_dis_y_m, comp_dis_z_m  float32     gt_flow / sensor_dt * dt0
 *     eval_mask                                 uint8       as himo_compdis_batch
 *     flow_category_indices                     uint8       copied   (HIMO_GT_HAS_CATEGORY)
 *     flow_instance_id                          uint32      copied   (HIMO_GT_HAS_INSTANCE)
 *     gt_flow_norm                              float32     ||gt_flow||_2 in the chain's dtype, rounded once
 *     pc0_x, pc0_y, pc0_z                       float32     copied
 * `columns` = HIMO_GT_HAS_* bits: a column without its bit is absent from the layout (its pointer may be NULL).
 */
#define HIMO_GT_HAS_CATEGORY 0x1u
#define HIMO_GT_HAS_INSTANCE 0x2u
#define HIMO_GT_MAX_COLUMNS 10

/* bytes of one sweep's body (a multiple of 8; 0 for an empty sweep) */
size_t himo_gt_body_bytes(int64_t n_points, unsigned columns);
/* h_starts[HIMO_GT_MAX_COLUMNS]: byte offset of every column inside the body in the order above, -1 for an absent one
 * (host arithmetic only: the function the kernel places its stores with); returns the body's bytes */
size_t himo_gt_column_starts(int64_t n_points, unsigned columns, int64_t* h_starts);

/* d_body_offsets int64[n_frames+1]: byte offset of every sweep's body in d_body, each a multiple of 8, with
 * offsets[f+1] - offsets[f] >= himo_gt_body_bytes(points of f, columns); d_body 8-byte aligned.  Every byte of a sweep's
 * body is written.  d_category uint8[T] / d_instance uint32[T] are read when their HIMO_GT_HAS_* bit is set.  flags:
 * F32_CHAIN, SCANIA, POSE_IS_EGO as in himo_compdis_batch (RAW is refused: the ground truth needs `flow`).  Workspace as
 * himo_compdis_workspace_bytes(n_frames). */
int himo_compdis_gt_batch(int n_frames, int64_t total_points,
                          const int64_t* d_offsets, const double* d_pose0, const double* d_pose1,
                          const float* d_pc0, int pc_stride, const float* d_flow, const float* d_lidar_dt,
                          double sensor_dt, unsigned flags,
                          const uint8_t* d_gm0, const uint8_t* d_flow_is_valid,
                          const uint8_t* d_category, const uint32_t* d_instance, unsigned columns,
                          const float* h_mask_bounds, float close_distance,
                          const int64_t* d_body_offsets, uint8_t* d_body,
                          void* d_workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The three functions of utils/__init__.py as stand-alone element-wise operators.
 * `dtype_is_f64` selects float64 flow/out arrays (numpy's result for float64 poses).
 */
/* utils/__init__.py:36-43  out = flow / sensor_dt * dt0[:, None];  flow,out: [n][3]; dt0: [n]
 * dtype_flags bit 0: flow and out are float64 (else float32); bit 1: dt0 is float64 (needs bit 0,
 * numpy's promotion rule) */
int himo_flow2compdis(int64_t n, const void* d_flow, const void* d_dt0, double sensor_dt,
                      int dtype_flags, void* d_out, void* stream);
/* utils/__init__.py:45-47  out = pc[:, :3] + ds;  pc float[n][pc_stride]; ds,out [n][3] */
int himo_refine_pts(int64_t n, const float* d_pc, int pc_stride, const void* d_ds,
                    int dtype_is_f64, void* d_out, void* stream);
/* utils/__init__.py:26-34  out[i] = 1 when point i is OUTSIDE the open box (min,max) */
int himo_ego_pts_mask(int64_t n, const float* d_pts, int pc_stride, const float* h_bounds,
                      uint8_t* d_out, void* stream);
/* save_zip.py:120 / eval.py:299  dt0 = max(lidar_dt) - lidar_dt  (one frame; d_workspace >= 32 bytes, 16-byte aligned) */
int himo_dt0(int64_t n, const float* d_lidar_dt, float* d_dt0, void* d_workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a8: exact k = 1 nearest neighbour (both halves of the Chamfer distance), brute force through LDS.
 * Replaces the cKDTree build + query pairs of eval.py:56-59 / tools/test/score.py:186-189 and is the
 * correspondence search of the self-supervised Chamfer loss.
 * Queries in rows [q_offsets[s], q_offsets[s+1]) search the references in rows
 * [r_offsets[s], r_offsets[s+1]) (segments = sweeps of a batch, or instances).  d_q, d_r: [n][3]
 * float32, or float64 when dtype_is_f64.  d_dist2: [nq] SQUARED distance in the same dtype (+inf for
 * an empty reference range); d_idx: [nq] int32 global reference row or -1 (may be NULL).
 * float64 mode is bit-comparable with cKDTree ((dx*dx + dy*dy) + dz*dz, then sqrt by the caller);
 * float32 mode forms fmaf(dz, dz, fmaf(dy, dy, dx * dx)): within 6 * 2^-24 of the exact minimum.
 * Among equally distant references the LOWEST row wins, in both dtypes.  A candidate wins only while
 * its distance is < the best so far, starting from +inf: a reference with a NaN coordinate is never
 * matched, and a query with a NaN coordinate (or whose candidates are all at +inf) gets +inf and -1,
 * like an empty range.  The offsets are not validated: they must be ascending, q_offsets[n_segments]
 * == nq and r_offsets[n_segments] <= nr.  nq == 0 returns HIMO_OK and writes nothing. */
int himo_nn_search(int n_segments, const int64_t* d_q_offsets, const int64_t* d_r_offsets,
                   int64_t nq, int64_t nr, const void* d_q, const void* d_r, int dtype_is_f64,
                   void* d_dist2, int32_t* d_idx, void* stream);
/* squared distances -> distances, in place (the sqrt cKDTree applies to the winning squared distance) */
int himo_sqrt_inplace(int64_t n, void* d_values, int dtype_is_f64, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a7 + a8: per-instance refinement metrics for a ragged batch of sweeps.
 * Replaces the per-category / per-instance loops of InstanceMetrics.step_eval (eval.py:64-114) and
 * ScoreMetrics.step (tools/test/score.py:223-321) up to, but not including, the bucket bookkeeping
 * (eval.py:99-147), which needs a few dozen records per sweep and stays on the host.
 * One record per (frame, class group, instance id) among the points with eval_mask != 0 and
 * (class_lut[category] & 3) != 0, in no particular order (sort on the host).
 * Only the low two bits of a class_lut byte are read: `group` is class_lut[category] & 3, so a byte of 3 opens a third
 * group, 5 joins group 1, and 4 evaluates nothing.  Only the low 32 bits of an instance id are read: ids that agree
 * modulo 2^32 (-1 and 2^32 - 1, say) are ONE instance, and `instance` reports the id modulo 2^32 (0 .. 2^32 - 1).
 * The four means are sums in a fixed order (tests/test_eval_conformance_gpu.py holds them to equal bits of
 * oracle/eval_oracle.py): a call repeated gives the same bits. */
typedef struct himo_instance_record {
    int32_t frame;     /* index of the sweep in the batch */
    int32_t group;     /* class_lut value: 1 = CAR, 2 = OTHER_VEHICLES */
    int64_t instance;  /* flow_instance_id */
    int64_t num_pts;   /* eval.py:90 */
    double vel;        /* mean |gt_flow| / sensor_dt                         eval.py:91 */
    double dis;        /* mean |pc0 row| (all columns, float32 norm)         eval.py:94 */
    double mpe;        /* mean |gt_refined - est_refined|                    eval.py:95 */
    double cham;       /* (mean NN(gt->est) + mean NN(est->gt)) / 2          eval.py:50-62, :96 */
} himo_instance_record;

#define HIMO_EVAL_FLOW 0     /* d_est = estimated flow incl. ego motion (EVAL_FLAG 2, eval.py:301-305) */
#define HIMO_EVAL_COMPDIS 1  /* d_est = float32 comp_dis read from a zip (EVAL_FLAG 1, eval.py:306-310) */
#define HIMO_EVAL_RAW 2      /* est_flow = zeros (res_name == "raw") */
#define HIMO_EVAL_SCORE 3    /* leaderboard scorer: d_gt = GT comp_dis, d_est = predicted comp_dis (both float32),
                                d_pc0 = pc0 xyz or NULL, d_lidar_dt = gt_flow_norm or NULL; poses unused
                                (tools/test/score.py:299-306) */

#define HIMO_EVAL_DIRECT 4   /* step_eval's own arguments (eval.py:64): d_pc0 = masked points, d_gt = float64 [T][3]
                                ego-motion-free GT flow, d_lidar_dt = dt0 (already max - dt), d_est = float64 [T][3]
                                ego-motion-free estimated flow, or float32 comp_dis with HIMO_EVAL_DIRECT_EST_IS_DIS;
                                poses unused */
#define HIMO_EVAL_DIRECT_EST_IS_DIS 0x100u

size_t himo_eval_workspace_bytes(int n_frames, int64_t total_points, int64_t max_records);

/* d_gt: GT flow incl. ego motion [T][3] (data['flow']); d_category uint8[T]; d_instance int64[T] (ids must fit
 * 32 bits); d_eval_mask uint8[T] (e.g. from himo_compdis_batch); h_class_lut: HOST uint8[256].
 * d_records: himo_instance_record[max_records]; d_counts: int64[2] = {selected points, records found}.
 * flags: HIMO_FLAG_POSE_IS_EGO.  Always the float64 chain.  Synchronises the stream once internally.
 * d_counts[1] is the number of records FOUND; when it exceeds max_records only max_records of them (any) were
 * written, each complete: call again with room for all.  total_points == 0 zeroes d_counts and writes nothing
 * else; with nothing selected d_counts is {0, 0} and no record is written.
 * sensor_dt: +0.0 and -0.0 are refused (HIMO_ERR_INVALID_ARGUMENT); a NaN is NOT -- it is divided by like any
 * other value, so vel and mpe come back NaN and cham +inf (points that are all NaN match nothing). */
int himo_eval_instances(int n_frames, int64_t total_points,
                        const int64_t* d_offsets, const double* d_pose0, const double* d_pose1,
                        const float* d_pc0, int pc_stride, const void* d_gt, const void* d_est,
                        const float* d_lidar_dt, const uint8_t* d_category, const int64_t* d_instance,
                        const uint8_t* d_eval_mask, const uint8_t* h_class_lut,
                        double sensor_dt, int mode, unsigned flags,
                        himo_instance_record* d_records, int64_t max_records, int64_t* d_counts,
                        void* d_workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Downstream segmentation evaluator: the confusion matrices of downstream/eval_seg.py (iouEval.addBatch, :113-134, fed
 * by the loop at :248-265) for a packed batch of sweeps, one launch, one pass over the bytes.
 * d_gt: uint8[T] flow_category_indices; h_pred: HOST array of n_results (1..HIMO_SEG_MAX_RESULTS) DEVICE pointers, each
 * uint8[T] predicted category indices; d_seg_valid: uint8[T] (non-zero = set) or NULL; h_class_lut: HOST uint8[256],
 * values 0..2 (eval_seg.py:255-257 as one table).
 * d_conf: int64[n_results][2][3][3], ADDED to (zero it first): [r][0] counts every point, [r][1] the points with
 * seg_valid set (nothing when d_seg_valid is NULL); rows = predicted class, columns = ground-truth class.
 * total_points < 2^31.  16-byte aligned base pointers take the vectorised path. */
#define HIMO_SEG_MAX_RESULTS 8
int himo_seg_confusion(int64_t total_points, const uint8_t* d_gt, const uint8_t* const* h_pred, int n_results,
                       const uint8_t* d_seg_valid, const uint8_t* h_class_lut, int64_t* d_conf, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Scene-flow evaluator ("flow metrics, v1", himo_amd/eval_flow.py; csrc/flowmetrics.hip): three-way and bucketed end-point
 * error of up to HIMO_FLOWM_MAX_RESULTS estimated flows against the ground-truth flow of a packed batch of sweeps, one
 * launch after the per-sweep transform prep.  PARITY UNPINNED: the reference does this in its absent OpenSceneFlow
 * submodule; this is the package's own written rule and makes no claim about the reference's numbers.
 * d_offsets int64[F+1]; d_pose0 / d_pose1 double[F][4][4] (with HIMO_FLAG_POSE_IS_EGO d_pose0 holds inv(pose1) @ pose0 and
 * d_pose1 may be NULL); d_pc0 float[T][pc_stride]; d_gt float[T][3] (data['flow'], ego motion included); h_est: HOST array of
 * n_results DEVICE pointers to float[T][3], NULL = "raw" (no estimate: ego motion only); d_category / d_ground uint8[T];
 * d_valid uint8[T], read only with HIMO_FLAG_SCANIA (which also selects the Scania ego box); h_class_lut: HOST uint8[256],
 * values 0..4 = BACKGROUND, CAR, OTHER_VEHICLES, PEDESTRIAN, WHEELED_VRU, 5 = other foreground (in no bucket).
 * A point is counted where the evaluation mask of himo_compdis_batch holds (range 35 m).  Units: 2^-24 m.
 * d_buckets int64[R][5][51][3] = count, sum q(epe), sum q(speed) per class and speed bucket (bucket b = #{k in 1..50:
 * speed >= k * 0.4 sensor_dt}); d_threeway int64[F][R][3][2] = count, sum q(epe) per sweep for FD, FS, BS (dynamic: speed >
 * 0.5 sensor_dt); d_rejected int64[R] = counted points with a non-finite estimate or an error of 1024 m or more, which
 * enter nothing else.  All three are ADDED to (the caller zeroes them).  d_workspace: 16-byte aligned,
 * himo_flow_metrics_workspace_bytes(F) bytes.  total_points < 2^31; zero points returns HIMO_OK.  Never synchronises. */
#define HIMO_FLOWM_MAX_RESULTS 8
#define HIMO_FLOWM_CLASSES 5
#define HIMO_FLOWM_BUCKETS 51
size_t himo_flow_metrics_workspace_bytes(int n_frames);
int himo_flow_metrics_batch(int n_frames, int64_t total_points, const int64_t* d_offsets,
                            const double* d_pose0, const double* d_pose1, const float* d_pc0, int pc_stride,
                            const float* d_gt, const float* const* h_est, int n_results,
                            const uint8_t* d_category, const uint8_t* d_ground, const uint8_t* d_valid,
                            const uint8_t* h_class_lut, double sensor_dt, unsigned flags,
                            int64_t* d_buckets, int64_t* d_threeway, int64_t* d_rejected,
                            void* d_workspace, void* stream);
/* The same call with two additions to the rule (both PARITY UNPINNED: the package's own rule).  est_stride: floats per row of
 * every estimate, >= 3 (rows of a wider buffer are read in place).  HIMO_FLAG_EST_RESIDUAL in flags: every non-NULL estimate is
 * the ego-motion-free part of a result (a network's own output rows, before the pose flow is added): its error is
 * (double)res - (gt - pose_flow); an all-zero residual is the "raw" result.  d_accuracy int64[R][4][3] = count, strict, relaxed
 * of the groups ALL, FD, FS, BS over the counted, non-rejected points, ADDED to (strict: epe < 0.05 || epe < 0.05 |gt|;
 * relaxed: 0.1 likewise; |gt| of the stored ground truth); NULL: the table is not computed.  est_stride < 3 is
 * HIMO_ERR_INVALID_ARGUMENT and nothing is written.  himo_flow_metrics_batch is this call with est_stride 3, no flag, NULL. */
#define HIMO_FLAG_EST_RESIDUAL 0x10u
int himo_flow_metrics_batch_ex(int n_frames, int64_t total_points, const int64_t* d_offsets,
                               const double* d_pose0, const double* d_pose1, const float* d_pc0, int pc_stride,
                               const float* d_gt, const float* const* h_est, int n_results, int est_stride,
                               const uint8_t* d_category, const uint8_t* d_ground, const uint8_t* d_valid,
                               const uint8_t* h_class_lut, double sensor_dt, unsigned flags,
                               int64_t* d_buckets, int64_t* d_threeway, int64_t* d_rejected, int64_t* d_accuracy,
                               void* d_workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Scania extractor: the labelling of dataprocess/extract_sca.py:95-145 (compute_flow) for a packed batch of sweeps, one
 * launch.  Replaces the pose flow of extract_sca.py:97, the `mmcv.ops.points_in_boxes_part` call of extract_sca.py:117 on double
 * tensors, the object flow and validity of :120-134 and the class / instance columns of :137-140.
 * h_offsets / d_offsets: int64[F+1], the same values on the host (validated here) and on the device (read by the kernel);
 * d_ego1_SE3_ego0: double[F][3][4], the top rows of inv(pose1) @ pose0 computed by the caller; d_pc: float[T][4].
 * h_box_offsets / d_box_offsets: int32[F+1] into the box table, whose rows the caller prepares (:104-114 and the op's own
 * constants): d_box_geom double[B][8] = cx, cy, cz_centre, dx/2, dy/2, dz/2, cos(-rz), sin(-rz); d_box_flow float[B][3] =
 * (hstack(vel, 0) * 0.1).astype(float32), zero where the velocity is infinite; d_box_class uint8[B]; d_box_vel_finite uint8[B].
 * background_class: the byte of 'none'.  Outputs: d_flow float[T][3], d_flow_is_valid uint8[T], d_category uint8[T],
 * d_instance uint32[T] (box index within the sweep + 1; 0 = background; the first containing box in list order wins).
 * Refuses (HIMO_ERR_INVALID_ARGUMENT, outputs untouched) negative or decreasing offsets, offsets that do not start at 0 and
 * end at total_points / n_boxes, and NULL where data is required.  16-byte aligned d_pc / d_flow / d_instance and 4-byte
 * aligned byte columns take the vectorised path.  Asynchronous on `stream`. */
int himo_box_label_batch(int n_frames, int64_t total_points, const int64_t* h_offsets, const int64_t* d_offsets,
                         const double* d_ego1_SE3_ego0, const float* d_pc, int n_boxes, const int* h_box_offsets,
                         const int* d_box_offsets, const double* d_box_geom, const float* d_box_flow,
                         const uint8_t* d_box_class, const uint8_t* d_box_vel_finite, int background_class,
                         float* d_flow, uint8_t* d_flow_is_valid, uint8_t* d_category, uint32_t* d_instance, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Ground segmenter: the per-point `ground_mask` every program of the package consumes, for a packed batch of sweeps.
 * The reference takes the mask from a ground-segmentation pass in its absent submodule, so this stage follows the build's own
 * written rule, "ray ground filter, v1" (the module docstring of himo_amd/ground_seg.py is normative): PARITY UNPINNED.
 *   bin      a point's cell = (range bin, one of 8K segments equal in tangent), float32, no transcendental; the cell's
 *            prototype = its point of lowest z (ties: lowest index), one 64-bit atomicMin per (wave, cell)
 *   walk     per (sweep, segment) over the bins in ascending order, float64 on float32 inputs: a prototype (r, z) is accepted
 *            iff fabs(z - g_prev) <= max_slope * (r - r_prev) + step_tol; the cell's ground height G is z if accepted, else
 *            the height carried so far (also for a cell without points)
 *   classify a binned point is ground iff z - G[cell] <= ground_thresh (float32)
 * h_offsets / d_offsets: int64[F+1], the same values on the host (validated here) and on the device (read by the kernels);
 * d_xyz: float[T][pitch], pitch 3 or 4 (x, y, z first); d_mask: uint8[T], 1 = ground; d_cell_ground: float[F][n_bins][8K] or
 * NULL -- the rows of a sweep WITHOUT points are left as the caller had them (nothing is launched for such a sweep, nor for
 * total_points == 0, which returns HIMO_OK).  d_workspace: 16-byte aligned, himo_ground_seg_workspace_bytes() bytes
 * (HIMO_ERR_WORKSPACE when shorter; the function returns 0 for parameters the batch call refuses).
 * Refuses (HIMO_ERR_INVALID_ARGUMENT, nothing launched) a pitch other than 3 or 4, offsets that are negative, decreasing, do
 * not start at 0 or end at total_points, NULL where data is required, and parameters outside: r_min > 0, bin_size > 0,
 * 1 <= n_bins <= 4096, 1 <= K <= 512, every float finite.  total_points > 0x7fffffff: HIMO_ERR_UNSUPPORTED (the prototype key
 * holds a 32-bit point index).  Asynchronous on `stream`; the same inputs give the same bytes on every run. */
typedef struct himo_ground_params {
    float sensor_height;   /* the ground is expected at z = -sensor_height under the vehicle */
    float r_min;           /* points nearer than this (in the x-y plane) are never ground */
    float bin_size;        /* radial size of a cell */
    int32_t n_bins;
    int32_t K;             /* segments per octant: 8K segments */
    float max_slope;
    float step_tol;
    float ground_thresh;
} himo_ground_params;

size_t himo_ground_seg_workspace_bytes(int n_frames, const himo_ground_params* params);
int himo_ground_seg_batch(int n_frames, int64_t total_points, const int64_t* h_offsets, const int64_t* d_offsets,
                          const float* d_xyz, int pitch, const himo_ground_params* params, uint8_t* d_mask,
                          float* d_cell_ground, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Free-space labeller: which points of a target sweep sit where OTHER sweeps saw through (himo_amd/csrc/raymap.hip).  The
 * reference's label generator is in its absent submodule, so this stage follows the build's own written rule, "free-space ray
 * map, v1" (the module docstring of himo_amd/raymap.py is normative): PARITY UNPINNED.
 *   quantise  f = (c - min) * scale (float32, two operations), scale = (float)(256.0 / voxel); a point is unusable when an f is
 *             not finite or |f| >= 2^22; u = (int)floorf(f) in 1/256 voxel, voxel index u >> 8
 *   carve     every ray walks the voxels from its origin's to its end point's in exact integer arithmetic (the next boundary
 *             crossing by 64-bit cross-multiplication, ties to the lowest axis); a visited voxel in the grid whose Chebyshev index
 *             distance to the end voxel is > guard gets FREE bit `slot`, the end voxel (never visited) HIT bit 16 + slot.
 *             Marks are OR-ed into the caller's map (uint32 [nz][ny][nx], cleared by the caller): calls accumulate.
 *   query     w = the word of a point's voxel, fv = popcount((w & 0xFFFF) & ~(w >> 16)), hv = popcount(w >> 16); the point is
 *             DYNAMIC iff it is not skipped, usable, in the grid, fv >= min_votes and fv > hv
 * d_pts: float[n][pitch], pitch 3 or 4 (x, y, z first) in the map's frame; d_slot: one byte per ray, 0..15 = the sweep the ray
 * belongs to (its origin is d_origins[slot]), 255 = the ray takes no part; d_origins: float[16][3]; d_skip: uint8[n] or NULL,
 * non-zero = the point is never DYNAMIC; d_free_votes / d_hit_votes / d_dynamic: uint8[n], each may be NULL (fv and hv are 0 for
 * a skipped, unusable or out-of-grid point).
 * Refused with HIMO_ERR_INVALID_ARGUMENT, nothing launched and nothing written: n < 0, a pitch other than 3 or 4, NULL where data
 * is required, d_pts / d_origins / d_map not 4-byte aligned, and parameters outside: every float finite, voxel > 0, scale ==
 * (float)(256.0 / voxel) and finite, 1 <= nx, ny <= 1024, 1 <= nz <= 64, nx*ny*nz <= 2^24, 0 <= guard <= 8, 1 <= min_votes <= 16
 * (himo_raymap_map_bytes returns 0 for them).  n > 2^31 - 1: HIMO_ERR_UNSUPPORTED.  n == 0: HIMO_OK without a launch.
 * A slot byte in 16..254 makes the WHOLE carve call a refused one, found on the device: a first kernel reads every slot byte, the
 * carving kernel behind it on the stream then marks nothing, and the refusal is recorded in a flag word of the device.  Both calls
 * are asynchronous on `stream`, so himo_raymap_carve itself still returns HIMO_OK for such a call; himo_raymap_status(stream) waits
 * for `stream`, returns HIMO_ERR_INVALID_ARGUMENT when a carve call on the current device was refused in this way since the last
 * himo_raymap_status, and clears the flag.  The map after equal calls is the same bytes on every run (OR is order-independent). */
typedef struct himo_raymap_params {
    float x0, y0, z0;      /* grid minimum */
    float voxel;           /* voxel edge, m */
    float scale;           /* (float)(256.0 / voxel), the division in double */
    int32_t nx, ny, nz;
    int32_t guard;         /* voxels in front of a return (Chebyshev) that its ray does not carve */
    int32_t min_votes;     /* sweeps that must have seen through a voxel */
} himo_raymap_params;

size_t himo_raymap_map_bytes(const himo_raymap_params* params);        /* 4*nx*ny*nz; 0 = parameters refused */
int himo_raymap_carve(int64_t n_rays, const float* d_pts, int pitch, const unsigned char* d_slot, const float* d_origins,
                      const himo_raymap_params* params, uint32_t* d_map, void* stream);
int himo_raymap_query(int64_t n, const float* d_pts, int pitch, const unsigned char* d_skip, const himo_raymap_params* params,
                      const uint32_t* d_map, unsigned char* d_free_votes, unsigned char* d_hit_votes, unsigned char* d_dynamic,
                      void* stream);
int himo_raymap_status(void* stream);

/* ---------------------------------------------------------------------------------------------
 * Whole-drive free-space map: one map carved from EVERY sweep of a scene, each walked once, that labels points and names the voxels
 * that are reliably static (himo_amd/csrc/drivemap.hip).  The reference has no such stage: this one follows the build's own written
 * rule, "free-space drive map, v1" (the module docstring of himo_amd/drivemap.py is normative): PARITY UNPINNED.
 *   quantise, rays, walk   rules A-C of "free-space ray map, v1" above, unchanged; the origin of ray i is d_origins[d_src[i]]
 *   carve     sweep s marks a voxel FREE if one of its rays visits it in the grid at Chebyshev index distance > guard from that ray's
 *             end voxel, and HIT if one of its rays ends in it.  hit_n counts the sweeps that marked the voxel HIT, free_n those that
 *             marked it FREE and not HIT.  One uint64 per voxel, [nz][ny][nx], cleared by the caller:
 *             stamp (s + 1) in bits 63..48 | HIT bit 33 | FREE bit 32 | free_n in bits 31..16 | hit_n in bits 15..0,
 *             the state bits being what the sweep of the stamp did (HIT replaces FREE).  The word after a sweep depends on the set of
 *             that sweep's marks only: not on ray order, on how its rays are split over calls, or on carving rays twice.
 *             PRECONDITION: the sweep numbers of the calls on one map do not decrease (a sweep that comes back after another has
 *             stamped a voxel is counted again there); 0 <= sweep <= 65534.
 *   query     fv = free_n, hv = hit_n of a point's voxel, both 0 for a skipped, unusable or out-of-grid point; the point is DYNAMIC
 *             iff it is not skipped, fv >= min_votes and fv > hv
 *   emit      a voxel is STATIC iff hit_n >= min_hits and not (free_n >= min_votes and free_n > hit_n).  One row per STATIC voxel in
 *             ascending linear index (vz*ny + vy)*nx + vx: float[4] = {x, y, z, 0} with x = ((float)vx + 0.5f) * voxel + x0 (every
 *             operation rounding on its own), beside it hit_n and free_n as int32.  Count, scan, write: no atomic orders the rows.
 *             *d_count receives the number of STATIC voxels whatever `capacity` is; rows at and beyond `capacity` are not written
 *             (capacity 0: the count alone, the row pointers may be NULL).
 * d_pts: float[n][pitch], pitch 3 or 4, in the map's frame; d_src: one byte per ray, 0..15 = the row of d_origins (float[16][3]) the
 * ray starts from, 255 = the ray takes no part; d_skip: uint8[n] or NULL; d_free_n / d_hit_n: uint16[n], d_dynamic: uint8[n], each
 * may be NULL.  The workspace of emit: himo_drivemap_emit_workspace_bytes(params) bytes, 4-byte aligned.
 * Refused with HIMO_ERR_INVALID_ARGUMENT, nothing launched and nothing written: n < 0, a pitch other than 3 or 4, a sweep outside
 * 0..65534, a capacity < 0, NULL where data is required, d_pts / d_origins / row outputs / the workspace not 4-byte aligned, the map
 * or d_count not 8-byte aligned, d_free_n / d_hit_n not 2-byte aligned, and parameters outside: every float finite, voxel > 0, scale ==
 * (float)(256.0 / voxel), 1 <= nx, ny <= 16384, 1 <= nz <= 256, nx*ny*nz <= 2^29, 0 <= guard <= 8, 1 <= min_votes <= 65535,
 * 1 <= min_hits <= 65535 (himo_drivemap_bytes and himo_drivemap_emit_workspace_bytes return 0 for them).  A workspace that is too
 * small: HIMO_ERR_WORKSPACE.  n > 2^31 - 1: HIMO_ERR_UNSUPPORTED.  n == 0: HIMO_OK without a launch.
 * A src byte in 16..254 makes the WHOLE carve call a refused one, found on the device exactly as himo_raymap_carve finds a slot byte:
 * the call marks nothing, himo_drivemap_carve itself still returns HIMO_OK, and himo_drivemap_status(stream) waits for `stream`,
 * returns HIMO_ERR_INVALID_ARGUMENT when a carve call on the current device was refused in this way since the last
 * himo_drivemap_status, and clears the flag.  Every call is asynchronous on `stream` but that one; only 32- and 64-bit integer atomics
 * touch the map, and the map after equal calls is the same bytes on every run. */
typedef struct himo_drivemap_params {
    float x0, y0, z0;      /* grid minimum */
    float voxel;           /* voxel edge, m */
    float scale;           /* (float)(256.0 / voxel), the division in double */
    int32_t nx, ny, nz;
    int32_t guard;         /* voxels in front of a return (Chebyshev) that its ray does not carve */
    int32_t min_votes;     /* sweeps that must have seen through a voxel and not returned from it */
    int32_t min_hits;      /* sweeps that must have returned from a voxel of the static map */
} himo_drivemap_params;

size_t himo_drivemap_bytes(const himo_drivemap_params* params);          /* 8*nx*ny*nz; 0 = parameters refused */
int himo_drivemap_carve(int64_t n_rays, const float* d_pts, int pitch, const unsigned char* d_src, const float* d_origins, int sweep,
                        const himo_drivemap_params* params, uint64_t* d_map, void* stream);
int himo_drivemap_query(int64_t n, const float* d_pts, int pitch, const unsigned char* d_skip, const himo_drivemap_params* params,
                        const uint64_t* d_map, uint16_t* d_free_n, uint16_t* d_hit_n, unsigned char* d_dynamic, void* stream);
size_t himo_drivemap_emit_workspace_bytes(const himo_drivemap_params* params);
int himo_drivemap_emit(const himo_drivemap_params* params, const uint64_t* d_map, int64_t capacity, float* d_rows4, int32_t* d_hits,
                       int32_t* d_free_n, int64_t* d_count, void* d_workspace, size_t workspace_bytes, void* stream);
int himo_drivemap_status(void* stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-sweep accumulation: several compensated sweeps moved into one target frame and reduced to one centroid per occupied voxel,
 * each with the least time lag of its rows (himo_amd/csrc/accumulate.hip).  The reference has no such program in its tree, so this
 * stage follows the build's own written rule, "sweep accumulation, v1" (the module docstring of himo_amd/accumulate.py is
 * normative): PARITY UNPINNED.
 *   rows      a source row takes part iff its skip byte is 0, its x, y, z are finite and it is not strictly inside the ego box
 *             (six strict inequalities on the row as given)
 *   move      q = R p + t, the arithmetic of himo_rigid_transform (csrc/rigid_math.h), with the transform passed by value
 *   quantise  f = (c - min) * scale (float32, two operations), scale = (float)(256.0 / voxel); unusable when an f is not finite or
 *             |f| >= 2^22; u = (int)floorf(f), voxel index u >> 8, sub-voxel offset u & 255; a voxel outside [0, n) is dropped
 *   reduce    per occupied voxel, key (iz << 24) | (iy << 12) | ix: count, the integer sums Sx, Sy, Sz of the offsets, the least
 *             lag.  Insert calls accumulate until the table is cleared; at most 2^24 rows between two clears (the caller counts)
 *   emit      x = (float)((double)x0 + (((double)(256 * ix) + 0.5) + (double)Sx / (double)count) * ((double)voxel / 256.0)), every
 *             operation rounding on its own; beside it lag (uint8), count (int32) and the key (uint32); rows in ANY order
 * The table is an open-addressing hash table in device memory that the caller owns: himo_accum_table_bytes(capacity) bytes,
 * 16-byte aligned, capacity a power of two in 2^4 .. 2^26.  Only 32-bit integer atomics touch it, so the rows emitted after
 * equal calls, sorted by key, are the same bytes on every run (which slot a key sits in is not fixed).  The probe loop is bounded by the capacity: a row that finds every slot taken by other
 * keys is left out and recorded in a flag word of the device; himo_accum_status(stream) waits for `stream`, returns
 * HIMO_ERR_INVALID_ARGUMENT when an insert on the current device found the table full since the last himo_accum_status, and
 * clears the flag (the insert itself is asynchronous and returns HIMO_OK).
 * d_pts: float[n][pitch], pitch 3 or 4 (x, y, z first) in the source's frame; d_skip: uint8[n] or NULL; h_transform: 16 HOST
 * floats, row-major 4x4, source frame -> target frame; lag: 0..255.  himo_accum_emit writes min(rows, max_rows) rows to d_keys
 * uint32[max_rows], d_xyz float[max_rows][3], d_lag uint8[max_rows], d_count int32[max_rows], and the full number of occupied
 * voxels to d_n_rows (int32[1]) even when it exceeds max_rows.
 * Refused with HIMO_ERR_INVALID_ARGUMENT, nothing launched and nothing written: n < 0, a pitch other than 3 or 4, lag outside
 * 0..255, max_rows < 0, NULL where data is required, d_pts / d_n_rows / d_keys / d_xyz / d_count not 4-byte or the table not 16-byte
 * aligned, a refused capacity (himo_accum_table_bytes returns 0 for it) and parameters outside: every float finite, voxel > 0,
 * scale == (float)(256.0 / voxel) and finite, 1 <= nx, ny <= 4096, 1 <= nz <= 256.  n > 2^31 - 1: HIMO_ERR_UNSUPPORTED.  n == 0:
 * HIMO_OK without a launch. */
typedef struct himo_accum_params {
    float x0, y0, z0;      /* grid minimum */
    float voxel;           /* voxel edge, m */
    float scale;           /* (float)(256.0 / voxel), the division in double */
    int32_t nx, ny, nz;
    float ego_min[3];      /* rows strictly inside (ego_min, ego_max) take no part */
    float ego_max[3];
} himo_accum_params;

size_t himo_accum_table_bytes(int64_t capacity);                       /* 32 * (capacity + 1); 0 = capacity refused */
int himo_accum_clear(void* d_table, int64_t capacity, void* stream);
int himo_accum_insert(int64_t n, const float* d_pts, int pitch, const unsigned char* d_skip, const float* h_transform, int lag,
                      const himo_accum_params* params, void* d_table, int64_t capacity, void* stream);
int himo_accum_emit(const void* d_table, int64_t capacity, const himo_accum_params* params, int64_t max_rows, int32_t* d_n_rows,
                    uint32_t* d_keys, float* d_xyz, unsigned char* d_lag, int32_t* d_count, void* stream);
int himo_accum_status(void* stream);

/* "sweep accumulation, v2": opt-in additions to v1, PARITY UNPINNED as v1 is (the same docstring is normative; the numpy restatement
 * is tests/accumulate2_ref.py).  The table, its size, its hash and every v1 result are unchanged: words 6 and 7 of a 32-byte slot,
 * unused and cleared to 0 in v1, hold Sa and the greatest tag.  The v1 entry points above launch the same kernels with v2 compiled out.
 *   advect    (himo_accum_insert_ex, d_motion float[n][3] not NULL) after the row test and before the move: a row with a non-finite
 *             motion component takes no part; s = (mx*mx + my*my) + mz*mz, each operation rounded; iff s >= motion_min2 the row is
 *             moved, x' = fmaf((float)lag, mx, x), likewise y and z.  The ego-box test stays on the row as given.
 *   attribute (d_attr not NULL; row i's value is d_attr[i * attr_stride], so column 3 of float[n][4] rows is read in place with
 *             stride 4) g = v * attr_scale; q = 0 if !(g > 0), 255 if g >= 255, else (uint)floorf(g + 0.5f); Sa += q
 *   label     (d_label int32[n] not NULL) lab = label if 0 < label < 2^24 else 0; tag = ((255 - lag) << 24) | lab; the slot keeps
 *             the greatest tag: the label of the freshest row, the largest among ties, whatever the order of arrival
 *             A call without d_attr (d_label), v1's insert included, leaves Sa (the tag) alone: its rows count as intensity 0 and
 *             carry no label.
 *   emit      (himo_accum_emit_ex) beside v1's columns, where the pointer is not NULL:
 *             d_intensity[row] = (float)(((double)Sa / (double)count) / (double)attr_scale), d_label[row] = tag & 0xFFFFFF (int32)
 *   motion    (himo_accum_motion) a stored flow less its sweep pair's ego motion: q = E p with the arithmetic of
 *             himo_rigid_transform, d = q - p, m = flow - d, three rounded subtractions a row after the shared move; h_ego: 16 HOST
 *             floats, row-major, E = inv(pose1) @ pose0; d_pts float[n][pitch], d_flow and d_motion float[n][3]
 * Refused with HIMO_ERR_INVALID_ARGUMENT, nothing launched and nothing written: everything v1 refuses; attr_scale not finite or
 * not > 0 beside a d_attr (insert) or a d_intensity (emit); attr_stride < 1; motion_min2 not finite or negative (both whether or not
 * their pointer is NULL); d_motion, d_attr, d_label or d_intensity not 4-byte aligned.  Any of the v2 pointers may be NULL. */
int himo_accum_insert_ex(int64_t n, const float* d_pts, int pitch, const unsigned char* d_skip, const float* h_transform, int lag,
                         const himo_accum_params* params, void* d_table, int64_t capacity, const float* d_motion, float motion_min2,
                         const float* d_attr, int attr_stride, float attr_scale, const int32_t* d_label, void* stream);
int himo_accum_emit_ex(const void* d_table, int64_t capacity, const himo_accum_params* params, int64_t max_rows, int32_t* d_n_rows,
                       uint32_t* d_keys, float* d_xyz, unsigned char* d_lag, int32_t* d_count, float attr_scale, float* d_intensity,
                       int32_t* d_label, void* stream);
int himo_accum_motion(int64_t n, const float* d_pts, int pitch, const float* d_flow, const float* h_ego, float* d_motion, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The headless viewer's renderer ("point splat, v1"; csrc/render.hip; the rule is the module docstring of himo_amd/view.py and is
 * this build's own: no claim is made about the pixels of any other viewer).
 *
 * The visibility buffer is one uint64 per pixel, [height][width]: ~0 = empty, else (zq << 32) | point index, zq the 24-bit depth.
 * himo_render_clear fills it with ~0.  himo_render_splat adds n points (float32 rows of `pitch` >= 3 floats; d_offset, nullable,
 * float32 [n][3], is added per component first; d_skip, nullable, non-zero = not drawn): p -> camera coordinates
 * ((m0 x + m1 y) + m2 z) + m3 per row of the 3x4 matrix `m` (the camera looks along +z; x right, y down), dropped when a
 * coordinate is not finite or zc is outside [znear, zfar]; u = fx (xc / zc) + cx, v = fy (yc / zc) + cy (ortho: without the
 * divide), dropped when not finite or outside [-(radius + 1), extent + radius + 1); pixel (floor u, floor v);
 * zq = min(2^24 - 1, floor((zc - znear) * inv_range * 2^24)); then a 64-bit atomic minimum of (zq << 32) | (index_base + i) into
 * every pixel (px + dx, py + dy), dx^2 + dy^2 <= radius^2, that lies inside the image.  The nearest point wins, the lowest index
 * among equal zq; calls accumulate, in any order and any split, to the same bits.  Every float operation rounds on its own.
 * himo_render_resolve writes uint8 RGB [height][width][3]: an empty pixel takes `background`; a hit takes the colour of the
 * attribute at the key's low 32 bits (an index >= n_attr: `neutral`) -- mode 0: rgba[idx] (r | g << 8 | b << 16); mode 1:
 * lut[clamp(floor((scalar[idx] - lo) * scale), 0, 255)], a non-finite scalar: `neutral`; mode 2: palette[ids[idx] % palette_n], a
 * negative id: `neutral` -- shaded, when edl_strength > 0, by exp2(-edl_strength * resp), resp = the mean over the four
 * neighbours at +-edl_px of max(0, L_c - L_nb), L = log2(1 + zq), an empty neighbour L = 24, one outside the image L_c; a channel
 * becomes floor(c * shade + 0.5).  All pointers of himo_shade are device pointers; lut holds 256 entries.
 *
 * All three are asynchronous on `stream`.  Refused with HIMO_ERR_INVALID_ARGUMENT, nothing launched and nothing written: radius
 * outside 0..8, pitch < 3, n < 0, a non-positive width or height, a NULL or misaligned buffer, camera or shade, NULL points with
 * n > 0, znear / zfar / inv_range not finite or zfar <= znear or inv_range <= 0, a mode outside 0..2, the mode's attribute array NULL
 * with n_attr > 0, a NULL lut (mode 1) or palette (mode 2), palette_n <= 0 in mode 2, lo / scale not finite in mode 1, an
 * edl_strength that is negative or not finite, edl_px < 1 with edl_strength > 0.  HIMO_ERR_UNSUPPORTED: a side above 16384,
 * n > 2^31 - 1, index_base + n > 2^32.  n == 0: HIMO_OK without a launch. */
typedef struct himo_camera {
    float m[12];           /* world -> camera, 3 rows of 4 */
    int32_t ortho;         /* 0 = perspective */
    float fx, fy, cx, cy;
    float znear, zfar;
    float inv_range;       /* (float)1 / (zfar - znear), computed in float32 on the host */
    int32_t width, height;
} himo_camera;

typedef struct himo_shade {
    int32_t mode;          /* 0 = rgba, 1 = scalar through lut, 2 = ids through palette */
    int32_t palette_n;
    const uint32_t* rgba;
    const float* scalar;
    const int32_t* ids;
    const uint32_t* lut;
    const uint32_t* palette;
    int64_t n_attr;        /* entries behind the mode's attribute array */
    float lo, scale;
    uint32_t background, neutral;
    float edl_strength;
    int32_t edl_px;
} himo_shade;

int himo_render_clear(uint64_t* d_vis, int width, int height, void* stream);
int himo_render_splat(int64_t n, const float* d_pts, int pitch, const float* d_offset, const unsigned char* d_skip,
                      const himo_camera* cam, int radius, uint32_t index_base, uint64_t* d_vis, void* stream);
int himo_render_resolve(const uint64_t* d_vis, int width, int height, const himo_shade* shade, unsigned char* d_rgb, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The viewer's line overlay ("line overlay, v1"; csrc/renderlines.hip; the rule is the module docstring of himo_amd/view.py, this
 * build's own: PARITY UNPINNED, the reference has no such stage).
 *
 * The overlay has its own buffer, d_lines, one uint64 per pixel [height][width]: ~0 = empty, else (zq << 32) | segment index;
 * himo_render_clear clears it.  himo_render_lines adds n segments (float32 [n][6] = x0, y0, z0, x1, y1, z1): both ends to camera
 * coordinates as himo_render_splat does (dropped when one of the six is not finite); dropped when both zc < znear or both
 * zc > zfar, else an end outside [znear, zfar] moves along the ORIGINAL segment onto the plane it passed
 * (t = (plane - z) / (z_other - z), x' = x + t * (x_other - x), y' likewise, z' = plane); both ends projected as a point is,
 * dropped when a screen coordinate is not finite or |.| >= 2^20; end pixels (floor u, floor v), end depths zq as for a point.  Then
 * integers: dx = X1 - X0, dy = Y1 - Y0, steps = max(|dx|, |dy|); for k = 0..steps (floor division)
 * x_k = X0 + (2 k dx + steps) / (2 steps), y_k likewise, zq_k = zq0 + k (zq1 - zq0) / steps (steps = 0: the one pixel); the 64-bit
 * minimum of (zq_k << 32) | (index_base + i) into every pixel (x_k + ddx, y_k + ddy), ddx^2 + ddy^2 <= half_px^2, inside the image.
 * Depth is linear along the SCREEN segment: no perspective-correct depth is claimed.  Calls accumulate, in any order and split, to
 * the same bits.  himo_render_composite, per pixel of an RGB image himo_render_resolve has written: an empty d_lines word leaves the
 * pixel alone; with d_vis (nullable: no depth test) a non-empty point word of SMALLER zq leaves it alone too (a tie shows the line);
 * otherwise the pixel takes d_colors[idx] (r | g << 8 | b << 16), `neutral` when idx >= n_colors.
 *
 * Both are asynchronous on `stream`.  Refused with HIMO_ERR_INVALID_ARGUMENT, nothing launched and nothing written: n < 0, half_px
 * outside 0..3, a non-positive width or height, a NULL camera, a NULL or misaligned d_lines, NULL segments with n > 0, misaligned
 * segments, d_vis or d_colors, a NULL d_rgb, znear / zfar / inv_range as for himo_render_splat, n_colors < 0, NULL d_colors with
 * n_colors > 0.  HIMO_ERR_UNSUPPORTED: a side above 16384, n > 2^31 - 1, index_base + n > 2^32.  n == 0: HIMO_OK without a launch. */
int himo_render_lines(int64_t n, const float* d_seg, const himo_camera* cam, int half_px, uint32_t index_base, uint64_t* d_lines,
                      void* stream);
int himo_render_composite(const uint64_t* d_lines, const uint64_t* d_vis /* NULL = no depth test */, int width, int height,
                          const uint32_t* d_colors, int64_t n_colors, uint32_t neutral, unsigned char* d_rgb, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ICP-Flow baseline (`save --model icpflow`, result key `icpflow`): clusters of the non-ground points of pc0, one rigid fit
 * (yaw + 3-D translation) per cluster against pc1, flow = fitted motion.  The reference's ICP-Flow code is in its absent
 * submodule (only the key name is in its tree, tools/view_instance.py:155-156), so this stage follows the build's own written
 * rule, "cluster-rigid ICP, v1" (the module docstring of himo_amd/icpflow.py is normative): PARITY UNPINNED.
 *
 * The clustered points are passed SORTED BY LABEL: cluster k (label k + 1) owns the rows offsets[k] .. offsets[k + 1] of
 * d_pts / d_moved; h_offsets / d_offsets: int64[n_clusters + 1], the same values on the host (validated here) and on the device
 * (read by the kernels).  A cluster may be empty (a label without points).  A label >= n_clusters + 1 among the sorted rows is
 * rows beyond offsets[n_clusters]: offsets that do not end at n are refused.
 * State per cluster: d_transform double[C][5] = c, s, tx, ty, tz (R = [[c, -s], [s, c]] about z); d_status int32[C][4] =
 * HIMO_ICP_ACCEPTED / FAILED / REJECTED, the inlier count of the cluster's last pass, the vote peak kx, ky.
 *   himo_icp_vote   rule 2: the target sweep (d_target float[n_target][3]) is binned on the BEV cell grid of himo_nn_grid
 *                   (1 m cells from (-52, -52), 104 x 104; points outside go to the border cells); every clustered point votes with
 *                   the target points near it.  d_counts int32[C][(2 half + 1)^2] (bin (ky + half) * (2 half + 1) + kx + half),
 *                   d_peak int32[C][2] = kx, ky; starts d_transform at (1, 0, kx bin, ky bin, 0) and d_status at ACCEPTED.
 *   himo_icp_step   one iteration of rule 3 given the search result of the moved points (d_moved float[n][3]; d_nn_idx /
 *                   d_nn_dist2 from himo_nn_grid(n, d_moved, n_target, d_target)): inliers, float64 sums in a fixed reduction
 *                   shape (no floating-point atomics), closed form, composition; a cluster with fewer than min_inliers stops as
 *                   FAILED.  final_pass != 0 is rule 4 instead: count the inliers, ACCEPTED iff inliers / size >= min_ratio, else
 *                   REJECTED (FAILED stays).  d_inlier: uint8[n] or NULL.
 *   himo_icp_apply  rows in ANY order with their labels (d_labels int32[n]; 0 and any value outside 1 .. n_clusters: identity).
 *                   HIMO_ICP_MOVED: d_out float[n][3] = float32(R a + t), evaluated in float64; HIMO_ICP_FLOW: the same for the
 *                   ACCEPTED clusters only (every other row keeps a), minus d_base (float[n][base_pitch], float32 subtraction).
 * Refuse (HIMO_ERR_INVALID_ARGUMENT, nothing launched): a pitch other than 3 or 4, a negative count, offsets that are negative,
 * decreasing, do not start at 0 or end at n, NULL or misaligned where data is required, and parameters that are not finite and
 * positive or have half > 64.  A short, NULL or misaligned (16 bytes) workspace: HIMO_ERR_WORKSPACE (himo_icp_workspace_bytes
 * returns 0 for counts it refuses).  n == 0 or n_clusters == 0: HIMO_OK, nothing launched.  Asynchronous on `stream`; the same
 * inputs give the same bytes on every run. */
typedef struct himo_icp_params {
    float bin;             /* metres per vote bin */
    int32_t half;          /* the vote covers |kx|, |ky| <= half */
    float z_gate;          /* a pair votes iff |dz| <= z_gate */
    float max_dist;        /* inlier iff squared distance <= max_dist^2 */
    int32_t min_inliers;
    float min_ratio;       /* accepted iff inliers / cluster size >= min_ratio */
    int32_t iters;         /* read by the host: the kernels run one pass per call */
} himo_icp_params;

#define HIMO_ICP_ACCEPTED 0
#define HIMO_ICP_FAILED 1
#define HIMO_ICP_REJECTED 2
#define HIMO_ICP_MOVED 0
#define HIMO_ICP_FLOW 1

size_t himo_icp_workspace_bytes(int64_t n_target, int n_clusters);
int himo_icp_vote(int64_t n, const float* d_pts, int pitch, int n_clusters, const int64_t* h_offsets, const int64_t* d_offsets,
                  int64_t n_target, const float* d_target, const himo_icp_params* params, int32_t* d_counts, int32_t* d_peak,
                  double* d_transform, int32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream);
int himo_icp_step(int64_t n, const float* d_moved, int n_clusters, const int64_t* h_offsets, const int64_t* d_offsets,
                  int64_t n_target, const float* d_target, const int32_t* d_nn_idx, const float* d_nn_dist2,
                  const himo_icp_params* params, int final_pass, double* d_transform, int32_t* d_status, uint8_t* d_inlier,
                  void* d_workspace, size_t workspace_bytes, void* stream);
int himo_icp_apply(int64_t n, const float* d_pts, int pitch, const int32_t* d_labels, int n_clusters, const double* d_transform,
                   const int32_t* d_status, int mode, const float* d_base, int base_pitch, float* d_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sweep odometry (`python -m himo_amd.odometry`, stored key `pose_odom`): whole-sweep, 6-DoF scan-to-map ICP.  The reference has no
 * such stage: this one follows the build's own written rule, "sweep odometry, v1" (the module docstring of himo_amd/odometry.py is
 * normative): PARITY UNPINNED.
 *
 * d_src float[n][pitch] (pitch 3 or 4: x, y, z first) the source rows; d_map float[n_map][3] the map rows, finite (the centroids of
 * himo_accum_emit in ascending key order).  The state is ONE himo_odom_state in device memory: T, the first three rows of the
 * row-major transform source -> map frame, the status and what the last pass left.
 *   himo_odom_init      writes a fresh RUNNING state: T = h_transform (12 doubles on the HOST, NULL = the identity; passed by value, no
 *                       copy is enqueued); with d_vote (the double[5] transform himo_icp_vote wrote for ONE cluster) the translation x, y
 *                       is taken from d_vote[2], d_vote[3] on the device.
 *   himo_odom_map       bins the map on the BEV cell grid of the parameters (cell edge max_dist, gw x gh cells from (x0, y0); rows
 *                       outside go to the border cells) into the workspace: once per sweep.
 *   himo_odom_step      one iteration of rule 3 on the binned map: m = float32(T p) in float64, the nearest map row among the 3 x 3
 *                       cells around m's cell (float32 d2, ties keep the lowest row), inliers d2 <= max_dist^2, Geman-McClure weights,
 *                       the 28 float64 sums in a fixed reduction shape (no floating-point atomics), unpivoted Cholesky, Cayley update,
 *                       status.  d_nn_idx int32[n] / d_nn_d2 float[n], each or NULL: the neighbour row and d2 of every source row
 *                       (-1 and +inf without a candidate or for a non-finite m).  A state that is not RUNNING: nothing is written,
 *                       the per-row outputs included.  The workspace must hold what himo_odom_map left for the same map.
 *   himo_odom_register  himo_odom_map, then `iters` steps, enqueued with no host wait; nothing allocates or synchronises.
 * n == 0 and n_map == 0 are defined outcomes (the first step ends FAILED_PAIRS), not errors; d_src / d_map may then be NULL.
 * Refuse (HIMO_ERR_INVALID_ARGUMENT, nothing launched, nothing written): a pitch other than 3 or 4, a negative count, NULL or
 * misaligned (4 bytes; the state 8) where data is required, parameters that are NULL, not finite, max_dist / gm_scale / eps_t2 /
 * eps_r2 not > 0, gw / gh / min_pairs < 1 or iters outside 1 .. 1024, a non-finite h_transform.  gw * gh > 2^20 or a count above
 * 2^31 - 1: HIMO_ERR_UNSUPPORTED.  A short, NULL or misaligned (16 bytes) workspace: HIMO_ERR_WORKSPACE (himo_odom_workspace_bytes
 * returns 0 for what it refuses).  Asynchronous on `stream`; the same inputs give the same bytes on every run. */
typedef struct himo_odom_params {
    float x0, y0;          /* minimum corner of the BEV cell grid */
    float max_dist;        /* cell edge; inlier iff d2 <= max_dist^2 (one float32 product) */
    int32_t gw, gh;        /* cells in x and in y */
    float gm_scale;        /* s of the Geman-McClure weight (s / (s + r.r))^2 */
    int32_t min_pairs;     /* fewer inliers: FAILED_PAIRS */
    int32_t iters;         /* steps of himo_odom_register */
    double eps_t2, eps_r2; /* CONVERGED iff |t_xi|^2 < eps_t2 and |omega|^2 < eps_r2 */
} himo_odom_params;

typedef struct himo_odom_state {
    double T[12];          /* rows of the 3 x 4 transform */
    double cost;           /* sum w r.r of the last pass */
    double xi[6];          /* t_xi, omega of the last solved step */
    double sums[28];       /* the last pass: the 21 upper entries of H (row-major), the 6 of g, the cost */
    int32_t status;        /* HIMO_ODOM_* */
    int32_t iters;         /* passes run on this state */
    int32_t pairs;         /* inliers of the last pass */
    int32_t reserved;
} himo_odom_state;

#define HIMO_ODOM_RUNNING 0
#define HIMO_ODOM_CONVERGED 1
#define HIMO_ODOM_FAILED_PAIRS 2
#define HIMO_ODOM_FAILED_SOLVE 3

size_t himo_odom_workspace_bytes(int64_t n_map, const himo_odom_params* params);
int himo_odom_init(const double* h_transform, const double* d_vote, himo_odom_state* d_state, void* stream);
int himo_odom_map(int64_t n_map, const float* d_map, const himo_odom_params* params, void* d_workspace, size_t workspace_bytes,
                  void* stream);
int himo_odom_step(int64_t n, const float* d_src, int pitch, int64_t n_map, const float* d_map, const himo_odom_params* params,
                   himo_odom_state* d_state, int32_t* d_nn_idx, float* d_nn_d2, void* d_workspace, size_t workspace_bytes, void* stream);
int himo_odom_register(int64_t n, const float* d_src, int pitch, int64_t n_map, const float* d_map, const himo_odom_params* params,
                       himo_odom_state* d_state, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Ego-motion de-skew (`python -m himo_amd.deskew`): every row of a sweep is moved along the sweep's constant body twist from its own
 * capture time to the sweep's reference time.  The reference has no such stage: this one follows the build's own written rule, "ego
 * de-skew, v1" (the module docstring of himo_amd/deskew.py is normative): PARITY UNPINNED.
 *
 * A ragged batch of n_sweeps sweeps in one call: the rows laid end to end, d_pts float[n][in_pitch] and d_lidar_dt float[n]; offsets
 * int64[n_sweeps + 1] on the HOST (validated) and on the device (sweep b owns rows offsets[b] .. offsets[b + 1]); twists
 * double[n_sweeps][8] on the HOST (validated) and on the device: v, w (per `span`, in the sweep's own frame), span [s], one spare.
 *   himo_deskew_tref   d_tref float[n_sweeps]: per sweep the greatest (HIMO_DESKEW_REF_MAX) or least (.._MIN) finite lidar_dt, or 0
 *                      (.._ZERO, and a sweep without a finite lidar_dt).
 *   himo_deskew_rows   p' = Exp(-s xi) p (inverse = 1: Exp(+s xi) p) with s = (t_ref - lidar_dt) / span, in float64, rounded once
 *                      to float32, into d_out float[n][out_pitch].  A row with s == 0, with a non-finite coordinate or lidar_dt, or
 *                      of a sweep whose twist is all zeros passes through with its bytes.  Column 3 is copied (0 when the input has
 *                      none).  d_out == d_pts is the in-place run (equal pitches only).  d_counts int32[n_sweeps][2]: rows moved,
 *                      rows passed through; d_max_disp float[n_sweeps]: the greatest |p' - p| of the moved rows (float64, rounded
 *                      once; an integer atomic max on the bits of a non-negative float).
 * n_sweeps == 0 and sweeps without rows are defined outcomes, not errors.  Refuse (HIMO_ERR_INVALID_ARGUMENT, nothing launched,
 * nothing written): a pitch other than 3 or 4, a negative count, offsets that do not start at 0, decrease or do not end at n, NULL or
 * misaligned (4 bytes; offsets and twists 8) where data is required, a twist or span that is not finite, a span not > 0, an unknown
 * mode or `inverse`, d_pts and d_out that overlap other than as one buffer of one pitch.  n above 2^31 - 1: HIMO_ERR_UNSUPPORTED.
 * Both calls are asynchronous on `stream`, allocate nothing and wait for nothing; no floating-point atomics: the same inputs give the
 * same bytes on every run. */
#define HIMO_DESKEW_REF_MAX 0
#define HIMO_DESKEW_REF_MIN 1
#define HIMO_DESKEW_REF_ZERO 2

int himo_deskew_tref(int n_sweeps, int64_t n, const int64_t* h_offsets, const int64_t* d_offsets, const float* d_lidar_dt, int mode,
                     float* d_tref, void* stream);
int himo_deskew_rows(int n_sweeps, int64_t n, const int64_t* h_offsets, const int64_t* d_offsets, const float* d_pts, int in_pitch,
                     const float* d_lidar_dt, const double* h_twists, const double* d_twists, const float* d_tref, int inverse,
                     float* d_out, int out_pitch, int32_t* d_counts, float* d_max_disp, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Cluster-rigid flow refinement (`python -m himo_amd.rigid_refine`, result key `<res_name>_rigid`): a stored flow is projected
 * onto at most `models` rigid motions (yaw + 3-D translation) per cluster of the non-ground points of pc0; a motion that moves no
 * claimed point by static_disp becomes the identity, i.e. the ego-motion flow.  The reference has no such stage: this one follows
 * the build's own written rule, "cluster-rigid refinement, v1" (the module docstring of himo_amd/rigid_refine.py is normative):
 * PARITY UNPINNED.
 *
 * One call runs rule 2 (every round of every cluster) and rules 2e / 3 (the flow of ALL n rows) on `stream`.
 *   d_pc0 float[n][pitch] the sweep; d_flow float[n][3] the stored flow; d_moved float[n][3] the sweep in pc1's frame
 *   (himo_rigid_transform); d_labels int32[n], 0 = no cluster (read for claimed rows only).
 *   The clustered rows SORTED BY LABEL, as for himo_icp_*: d_rows int64[n_clustered] the sweep row of every sorted row; cluster k
 *   (label k + 1) owns the sorted rows offsets[k] .. offsets[k + 1], given on the host (validation) and on the device; offsets that
 *   do not end at n_clustered are refused.  Every row that is clustered takes part in the rule: the caller labels no ground row, no
 *   row outside the range and no row whose flow is not finite.
 * Outputs: d_status int32[C][models][4] = state, the inlier count of the round's last pass (its claim count when it claimed), the
 * vote peak kx, ky; d_transform double[C][models][5] = c, s, tx, ty, tz (identity for a STATIC round and for a round not run);
 * d_claim int8[n] = 0 or the round 1 .. models that claimed the row; d_out float[n][3] = float32(R a + t) - pc0 for a claimed row,
 * the BYTES of d_flow for every other row.
 * Refuse (HIMO_ERR_INVALID_ARGUMENT, nothing launched): a pitch other than 3 or 4, a negative count, n_clustered > n, clustered
 * rows without clusters, offsets that are negative, decreasing, do not start at 0 or end at n_clustered, NULL or misaligned where
 * data is required, parameters that are not finite and positive, half > 64, models > HIMO_RIGID_MAX_MODELS.  A short, NULL or
 * misaligned (16 bytes) workspace: HIMO_ERR_WORKSPACE (himo_rigid_refine_workspace_bytes returns 0 for what it refuses).  n == 0:
 * HIMO_OK, nothing launched; n_clusters == 0: d_out is the copy of d_flow.  The number of launches does not depend on the clusters;
 * float64 sums take a fixed shape (no floating-point atomics): the same inputs give the same bytes on every run. */
typedef struct himo_rigid_params {
    float bin;             /* metres per vote bin */
    int32_t half;          /* the vote covers |kx|, |ky| <= half */
    float tol;             /* inlier radius, metres */
    int32_t iters;         /* refit passes per round */
    int32_t min_inliers;
    float min_ratio;       /* a round is accepted iff inliers / cluster size >= min_ratio */
    float static_disp;     /* a round whose claim moves by less than this everywhere is static */
    int32_t models;        /* rounds per cluster */
} himo_rigid_params;

#define HIMO_RIGID_ACCEPTED 0
#define HIMO_RIGID_FAILED 1
#define HIMO_RIGID_REJECTED 2
#define HIMO_RIGID_STATIC 3
#define HIMO_RIGID_NOT_RUN 4
#define HIMO_RIGID_MAX_MODELS 4

size_t himo_rigid_refine_workspace_bytes(int64_t n_clustered, int n_clusters, int half, int models);
int himo_rigid_refine(int64_t n, const float* d_pc0, int pitch, const float* d_flow, const float* d_moved, const int32_t* d_labels,
                      int64_t n_clustered, const int64_t* d_rows, int n_clusters, const int64_t* h_offsets, const int64_t* d_offsets,
                      const himo_rigid_params* params, int32_t* d_status, double* d_transform, int8_t* d_claim, float* d_out,
                      void* d_workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Cluster boxes (`python -m himo_amd.box_fit`, dataset `boxes_<name>`): one oriented box per cluster of labelled points by the
 * search-based L-shape fit -- every heading of a fixed integer table is tried, the one with the most edge inliers is kept, ties go
 * to the smaller area, then to the lower table index (himo_amd/csrc/boxfit.hip).  The reference has no such stage: this one follows
 * the build's own written rule, "cluster boxes, v1" (the module docstring of himo_amd/box_fit.py is normative): PARITY UNPINNED.
 * Timed on a synthetic sweep only (profiles/box_fit.txt); nothing has been tried on field data.
 *
 *   d_pts float[n][pitch], pitch >= 3 (x, y, z first), raw or compensated as the caller decides; d_labels int32[n], 0 = none.
 *   The labelled rows SORTED BY LABEL, as for himo_rigid_refine: d_rows int64[n_clustered] the sweep row of every sorted row; cluster
 *   k (label k + 1) owns the sorted rows offsets[k] .. offsets[k + 1], given on the host (validation) and on the device.
 *   d_motion float[n][3] or NULL: a displacement per sweep period.  h_dirs: int32[n_dirs][2] on the HOST, read before the call
 *   returns: 1 <= n_dirs <= HIMO_BOXFIT_MAX_DIRS, every |a|, |b| <= 4096, a*a + b*b > 0.
 *   quantise  a row is USABLE iff its label > 0, x, y, z are finite and |x*scale|, |y*scale| (one float32 product each) are below
 *             4194304; X = (int)floorf(x*scale), Y likewise; n = the cluster's usable rows
 *   state     TOO_FEW iff n < min_points; else TOO_LARGE iff n > max_points or Xmax - Xmin >= 16384 or Ymax - Ymin >= 16384; else
 *             FITTED.  A cluster that is not FITTED writes its state and n, and zeros elsewhere
 *   fit       per direction (a, b): u = a X' + b Y', v = -b X' + a Y' over X' = X - Xmin, Y' = Y - Ymin; a row is an edge inlier iff
 *             min(u - umin, umax - u, v - vmin, vmax - v) <= tol_q << 12; S = the inlier count, A = (umax - umin)(vmax - vmin) in
 *             int64; the chosen k has the largest S, then the smallest A, then the lowest k.  All integers: order-independent
 *   box       float64, every operation rounding on its own: n2 = a a + b b, r = sqrt(n2), su = (umin + umax) / 2, sv likewise,
 *             px = (a su - b sv) / n2, py = (b su + a sv) / n2, cx = ((Xmin + px) + 0.5) / scale, eu = (umax - umin) / (r scale),
 *             cz = (zmin + zmax) / 2, h = zmax - zmin (the float32 extremes, -0 below +0); the float64 mean of the usable rows'
 *             motion, rows with a non-finite value left out of sum and count (a fixed summation shape: the same bytes every run)
 * Outputs: d_info int32[C][12] = state, n, k, S, Xmin, Ymin, umin, umax, vmin, vmax, motion row count, 0; d_box double[C][10] = cx,
 * cy, cz, eu, ev, h, mx, my, mz, 0.
 * Refused with HIMO_ERR_INVALID_ARGUMENT, nothing launched and nothing written: a negative count, pitch < 3, n_clustered > n,
 * clustered rows without clusters, offsets that are negative, decreasing, do not start at 0 or end at n_clustered, NULL or misaligned
 * where data is required, a refused table, and parameters outside: scale finite and > 0, 0 <= tol_q <= 1024, min_points >= 1,
 * min_points <= max_points <= 2^20.  n > 2^31 - 1: HIMO_ERR_UNSUPPORTED.  A short, NULL or misaligned (16 bytes) workspace:
 * HIMO_ERR_WORKSPACE (himo_boxfit_workspace_bytes returns 0 for what it refuses).  n_clusters == 0: HIMO_OK, nothing launched.
 * One launch, asynchronous on `stream`, whatever the clusters. */
typedef struct himo_boxfit_params {
    float scale;           /* sub-units per metre */
    int32_t tol_q;         /* edge-inlier tolerance, sub-units */
    int32_t min_points;    /* fewer usable rows: TOO_FEW */
    int32_t max_points;    /* more usable rows: TOO_LARGE */
} himo_boxfit_params;

#define HIMO_BOXFIT_FITTED 0
#define HIMO_BOXFIT_TOO_FEW 1
#define HIMO_BOXFIT_TOO_LARGE 2
#define HIMO_BOXFIT_MAX_DIRS 128
#define HIMO_BOXFIT_CHUNK 1024     /* points the kernel stages in LDS at a time (a size its tests straddle) */

size_t himo_boxfit_workspace_bytes(int64_t n_clustered, int n_clusters, int n_dirs);
int himo_boxfit(int64_t n, const float* d_pts, int pitch, const int32_t* d_labels, int64_t n_clustered, const int64_t* d_rows,
                int n_clusters, const int64_t* h_offsets, const int64_t* d_offsets, const float* d_motion, const int32_t* h_dirs,
                int n_dirs, const himo_boxfit_params* params, int32_t* d_info, double* d_box, void* d_workspace,
                size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Cross-sensor consistency (`python -m himo_amd.eval_xsensor`): inside every cluster of labelled points, the distance from each point
 * to the nearest point ANOTHER SENSOR recorded -- large where the sensors' copies of a moving object are displaced, the sampling spacing
 * where they lie on top of one another; a score that needs no ground truth (himo_amd/csrc/xsensor.hip).  The reference has no such
 * stage: this one follows the build's own written rule, "cross-sensor consistency, v1" (the module docstring of
 * himo_amd/eval_xsensor.py is normative): PARITY UNPINNED.  Timed on synthetic sweeps only (profiles/xsensor.txt); nothing has been
 * tried on field data.
 *
 *   d_pts float[n][pitch], pitch >= 3 (x, y, z first), raw or compensated as the caller decides; d_labels int32[n], 0 = none, else
 *   1..n_clusters; d_group uint8[n], the sensor id; d_dt float[n] or NULL, the capture time; d_motion float[n][3] or NULL, a
 *   displacement per sweep period.  The labelled rows SORTED BY LABEL, as for himo_boxfit: d_rows int64[n_clustered] the buffer row of
 *   every sorted row; cluster k owns the sorted rows offsets[k] .. offsets[k + 1], given on the host (validation) and on the device.
 *   The clusters of several sweeps and results may be laid end to end in one call: more segments over one point buffer.
 *   usable    a row is USABLE iff its label is in 1..n_clusters, x, y, z are finite, group <= 7 and, with d_dt, dt is finite;
 *             n = the cluster's usable rows, n_g those of group g
 *   state     TOO_FEW iff n < min_points; else TOO_LARGE iff n > max_points; else group g is LIVE iff n_g >= min_group and the
 *             cluster is ONE_SENSOR iff fewer than two groups are live; else SCORED.  A cluster that is not SCORED writes its state, n
 *             and the n_g, and zeros elsewhere
 *   search    a QUERY is a usable row of a live group; its candidates are the usable rows of the same cluster in ANOTHER live group;
 *             float32, every operation rounding on its own: dx = x_i - x_j, ..., d2 = (dx*dx + dy*dy) + dz*dz; m_i = the minimum
 *             over the candidates (order-free: defined bit for bit; no index is reported)
 *   terms     float64: d_i = sqrt(m_i); c_i = d_i < trunc ? d_i : trunc (+inf clips); NEAR iff d_i <= near; q(x) = llrint(x * 2^24);
 *             every sum is an int64 sum, so no order is part of the rule
 * Outputs: d_info int32[C][4] = state, n, live-group bit mask, query rows; d_rec int64[C][8][4], per group = n_g, the sum of q(dt) over
 * the group's usable rows (dt clipped to +-1024 s; 0 without d_dt), the sum of q(c_i) over its query rows, its NEAR count; d_mot
 * int64[C][2] = the usable rows with a finite motion and the sum of q(s_i) over them, s_i = sqrt((mx*mx + my*my) + mz*mz) in float64
 * clipped at 1024 m (zeros without d_motion); d_min_d2 float[n_clustered] or NULL: m_i per sorted row, +inf for a row that is no query.
 * All three are written whole: they need no clearing.
 * Refused with HIMO_ERR_INVALID_ARGUMENT, nothing launched and nothing written: a negative count, pitch < 3, n_clustered > n,
 * clustered rows without clusters, offsets that are negative, decreasing, do not start at 0 or end at n_clustered, NULL or misaligned
 * where data is required, and parameters outside: trunc finite, > 0 and <= 1024, near finite and >= 0, min_group >= 1, min_points
 * >= 2, min_points <= max_points <= 2^20.  n > 2^31 - 1: HIMO_ERR_UNSUPPORTED.  A short, NULL or misaligned (16 bytes) workspace:
 * HIMO_ERR_WORKSPACE (himo_xsensor_workspace_bytes returns 0 for what it refuses).  n_clusters == 0: HIMO_OK, nothing launched.
 * One clear and three launches (count, search, reduce), asynchronous on `stream`, whatever the clusters; no float atomics. */
typedef struct himo_xsensor_params {
    float trunc;           /* the distance a row's term is clipped at, metres */
    float near;            /* a row at most this far from another sensor's point is NEAR, metres */
    int32_t min_group;     /* fewer usable rows of a sensor in a cluster: that sensor is not live there */
    int32_t min_points;    /* fewer usable rows: TOO_FEW */
    int32_t max_points;    /* more usable rows: TOO_LARGE */
} himo_xsensor_params;

#define HIMO_XSENSOR_SCORED 0
#define HIMO_XSENSOR_TOO_FEW 1
#define HIMO_XSENSOR_ONE_SENSOR 2
#define HIMO_XSENSOR_TOO_LARGE 3
#define HIMO_XSENSOR_GROUPS 8
#define HIMO_XSENSOR_CHUNK 1024    /* rows the search stages in LDS at a time (a size its tests straddle) */

size_t himo_xsensor_workspace_bytes(int64_t n_clustered, int n_clusters);
int himo_xsensor(int64_t n, const float* d_pts, int pitch, const int32_t* d_labels, const uint8_t* d_group, const float* d_dt,
                 const float* d_motion, int64_t n_clustered, const int64_t* d_rows, int n_clusters, const int64_t* h_offsets,
                 const int64_t* d_offsets, const himo_xsensor_params* params, int32_t* d_info, int64_t* d_rec, int64_t* d_mot,
                 float* d_min_d2, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Cross-sensor alignment (`python -m himo_amd.xalign`, an ordinary flow key `xalign`): the planar velocity of every cluster from the
 * capture times inside ONE sweep -- the sensors record a moving object at different instants, r_i = P + v tau_i, so the v that lays
 * their copies on top of one another is the object's; no second sweep, no network, no training (himo_amd/csrc/xalign.hip).  The
 * reference names this route ("dynamic segmentation + ICP alignment across LiDARs") and ships no program for it: this one follows the
 * build's own written rule, "cross-sensor alignment, v1" (the module docstring of himo_amd/xalign.py is normative): PARITY UNPINNED.
 * Timed on synthetic sweeps only (profiles/xalign.txt); nothing has been tried on field data.
 *
 *   Inputs as for himo_xsensor; d_tau float[n], the capture time, is REQUIRED.  The labelled rows SORTED BY LABEL, the clusters of
 *   several sweeps laid end to end in one call.
 *   usable    rules A and B of cross-sensor consistency v1, word for word (one header states them for both files): the usable rows,
 *   state     the live groups, and TOO_FEW, TOO_LARGE, ONE_SENSOR in that order; then NO_BASELINE iff max t_g - min t_g < tau_min over
 *             the live groups, t_g = (sum of q24(tau clipped to +-1024 s)) / (2^24 n_g) in float64.  The ROWS below are the usable rows
 *             of live groups.  A cluster that ends in one of these states writes its state, n (and for NO_BASELINE the live mask and
 *             the rows), v = 0 and zeros elsewhere.  A cluster that ends as NO_BASELINE later -- no vote, or A == 0 -- writes v = 0
 *             and zero sums too, but keeps in d_info what it had counted by then: the votes and the winning bin, and after A == 0
 *             the iterations used and the pairs of the last one
 *   vote      every pair of rows (i, j) of live groups with group(i) < group(j), |tau_i - tau_j| >= tau_min and |z_i - z_j| < z_gate
 *             (float32) votes for (dx / dtau, dy / dtau) in float64; bin = floor(v / bin + nb / 2) per axis, nb = 2 ceil(v_max / bin)
 *             + 1; a vote outside the table is dropped; a bin's score is the sum of the counts of its 3 x 3 neighbourhood clipped at
 *             the edge; v_0 is the centre of the bin with the greatest score, ties to the smallest flat index bx nb + by; no vote:
 *             NO_BASELINE
 *   iterate   k = 0 .. iters - 1: moved rows x = r_x - (float)v_x tau, y likewise, z as recorded (float32, every operation rounding on
 *             its own); per row the nearest moved row of another live group by d2 = (dx*dx + dy*dy) + dz*dz, as the minimum of the
 *             64-bit key (bits of d2 << 32 | sorted row) -- ties to the smallest sorted row, a NaN orders as 0x7fc00000, after +inf;
 *             float64: d = sqrt(d2), the pair is kept iff d <= trunc, w = (sigma^2 / (sigma^2 + d^2))^2, dtau = tau_i - tau_j, dp = r_i
 *             - r_j on the RECORDED rows; A = sum q40((w dtau) dtau), b = sum q40((w dtau) dp_{x,y}), every term clipped to +-256 before
 *             q40(x) = llrint(x 2^40), int64 sums: no order is part of the rule; A == 0: NO_BASELINE; v_{k+1} = b / A; the loop ends
 *             after the step in which |v_{k+1} - v_k| < tol
 *   score     X(v) = sum over the rows of q24(min(d, trunc)) (a NaN counts as trunc) at v = 0 (X0) and at the final v (X1)
 *   decide    REJECTED iff |v| > v_max or (double)X1 > (1 - min_gain) (double)X0; else STATIC iff |v| < static_speed; else ALIGNED.
 *             Only ALIGNED clusters carry a non-zero v
 * Outputs, written whole (they need no clearing): d_info int32[C][8] = state, n, live-group bit mask, rows, votes cast, the winning
 * flat bin, iterations used, pairs kept in the last iteration; d_v float[C][4] = v_x, v_y, 0, |v|; d_x int64[C][2] = X0, X1.
 * himo_xalign_apply (rule G) over one point buffer of n_sweeps sweeps laid end to end (sweep s owns the rows pt_off[s] .. pt_off[s + 1];
 * d_E float[n_sweeps][12], the first three rows of inv(pose1) @ pose0): a row whose label is in 1..n_clusters, whose x, y, z are finite
 * and whose cluster is ALIGNED gets (E p - p) + v * sensor_dt -- E p by the arithmetic of himo_rigid_transform, as in
 * himo_trackflow_apply's replace mode; every other row keeps the bytes of d_base, or, with d_base NULL ("raw"), gets E p - p.
 * Refused with HIMO_ERR_INVALID_ARGUMENT, nothing launched and nothing written: what himo_xsensor refuses, d_tau NULL where rows are
 * clustered, and parameters outside: min_group >= 1, min_points >= 2, min_points <= max_points <= HIMO_XALIGN_MAX_POINTS; v_max, bin
 * finite and > 0, v_max <= 1024 and nb * nb <= HIMO_XALIGN_TABLE_CELLS (the vote table lives in LDS); tau_min, sigma, trunc finite, > 0
 * and <= 1024; z_gate finite and > 0; iters 1..HIMO_XALIGN_MAX_ITERS with iters * max_points^2 <= HIMO_XALIGN_MAX_WORK (2^32: one
 * workgroup walks a cluster, so the work of one is bounded); tol, static_speed finite and >= 0; min_gain finite in [0, 1).  n > 2^31 - 1:
 * HIMO_ERR_UNSUPPORTED.  A short, NULL or misaligned (16 bytes) workspace: HIMO_ERR_WORKSPACE (himo_xalign_workspace_bytes returns 0 for
 * what it refuses).  n_clusters == 0: HIMO_OK, nothing launched.  himo_xalign_apply refuses a negative count, pitch < 3, sensor_dt not
 * finite and > 0, rows without sweeps, offsets that do not start at 0, decrease or do not end at n, NULL or misaligned where data is
 * required; n == 0: HIMO_OK.
 * himo_xalign: one clear and two launches (count; one workgroup per cluster for everything else), asynchronous on `stream`, no host
 * wait; no float atomics; the same inputs give the same bytes. */
typedef struct himo_xalign_params {
    int32_t min_group;     /* fewer usable rows of a sensor in a cluster: that sensor is not live there */
    int32_t min_points;    /* fewer usable rows: TOO_FEW */
    int32_t max_points;    /* more usable rows: TOO_LARGE */
    int32_t iters;         /* the most iterations */
    float v_max;           /* the vote covers |v_x|, |v_y| <= v_max, and a faster result is REJECTED, m/s */
    float bin;             /* m/s per vote bin */
    float tau_min;         /* the smallest difference of capture times of a voting pair, and of the live groups' mean times, s */
    float z_gate;          /* a voting pair lies closer than this in z, metres */
    float sigma;           /* the scale of the weight, metres */
    float trunc;           /* a pair farther apart is dropped, and a row's score term is clipped here, metres */
    float tol;             /* the loop ends when v changes by less, m/s */
    float min_gain;        /* REJECTED unless X1 <= (1 - min_gain) X0 */
    float static_speed;    /* slower: STATIC, m/s */
} himo_xalign_params;

#define HIMO_XALIGN_ALIGNED 0
#define HIMO_XALIGN_TOO_FEW 1      /* = HIMO_XSENSOR_TOO_FEW */
#define HIMO_XALIGN_ONE_SENSOR 2   /* = HIMO_XSENSOR_ONE_SENSOR */
#define HIMO_XALIGN_TOO_LARGE 3    /* = HIMO_XSENSOR_TOO_LARGE */
#define HIMO_XALIGN_NO_BASELINE 4
#define HIMO_XALIGN_REJECTED 5
#define HIMO_XALIGN_STATIC 6
#define HIMO_XALIGN_CHUNK 1024           /* moved rows a nearest-neighbour pass stages in LDS at a time (a size its tests straddle) */
#define HIMO_XALIGN_TABLE_CELLS 15360    /* int32 cells of the LDS buffer the vote table must fit: nb <= 123 */
#define HIMO_XALIGN_MAX_POINTS 16384
#define HIMO_XALIGN_MAX_ITERS 100
#define HIMO_XALIGN_MAX_WORK 4294967296LL   /* iters * max_points^2 at the most: what ONE workgroup may be asked to walk */

size_t himo_xalign_workspace_bytes(int64_t n_clustered, int n_clusters);
int himo_xalign(int64_t n, const float* d_pts, int pitch, const int32_t* d_labels, const uint8_t* d_group, const float* d_tau,
                int64_t n_clustered, const int64_t* d_rows, int n_clusters, const int64_t* h_offsets, const int64_t* d_offsets,
                const himo_xalign_params* params, int32_t* d_info, float* d_v, int64_t* d_x, void* d_workspace, size_t workspace_bytes,
                void* stream);
int himo_xalign_apply(int64_t n, const float* d_pts, int pitch, const int32_t* d_labels, int n_clusters, const int32_t* d_info,
                      const float* d_v, int n_sweeps, const int64_t* h_pt_off, const int64_t* d_pt_off, const float* d_E,
                      const float* d_base, float sensor_dt, float* d_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Box evaluation (`python -m himo_amd.eval_box`): the rotated BEV IoU and the 3-D IoU of oriented boxes, and the greedy matching of
 * two sets of boxes per sweep by descending BEV IoU (himo_amd/csrc/boxeval.hip).  The reference has no such stage: this one follows
 * the build's own written rule, "box evaluation, v1" (the module docstring of himo_amd/eval_box.py is normative): PARITY UNPINNED.
 * Timed on synthetic sweeps only (profiles/box_eval.txt).
 *
 *   A rect is double[12]: the four BEV corners x0, y0 .. x3, y3, counter-clockwise; zlo, zhi; area; 0.  The HOST makes rects from box
 *   rows (the library calls no transcendental).  INVALID (IoU 0 with everything, never matched): a value that is not finite, a
 *   negative area, zhi < zlo.
 *   pair      float64, every operation rounding on its own: all corners relative to A's corner 0; disjoint bounds: 0; else A clipped
 *             by B's four edges in order (Sutherland-Hodgman; inside iff ex (vy - py) - ey (vx - px) >= 0; crossing s + (ds / (ds - de))
 *             (e - s)); the shoelace fan about vertex 0 times 0.5, clamped to [0, min(areaA, areaB)]; iou = inter / ((areaA + areaB) -
 *             inter), iou3 from inter times the overlap of the z ranges -- each 0 where its denominator is not > 0
 *   matching  per sweep, greedy: the pairs with iou >= min_iou in the order greater iou, then lower i, then lower j; a pair is kept
 *             iff neither its i nor its j was kept before
 * himo_boxeval_match: n_sweeps sweeps a call; sweep s owns the rects h_off[s] .. h_off[s + 1] of its side's packed table (offsets
 * int64[n_sweeps + 1], on the host for validation and on the device; the device copy is clamped to the host's totals, not read back).
 * Outputs, in the packed order: d_match_a int32[rows of A] = the j within the sweep or -1, d_match_b int32[rows of B] = the i or
 * -1, d_iou_a double[rows of A][2] = iou and iou3 of the kept pair, zeros otherwise.  A sweep with boxes on one side only writes
 * -1 / zeros for it.  The workspace is the dense candidate store: (rows of A in the call) x (the largest sweep of B) x 8 bytes,
 * rounded up to 256 (himo_boxeval_workspace_bytes: 0 for what it refuses).  Two launches, asynchronous on `stream`, no host wait.
 * Refused, nothing launched and nothing written.  HIMO_ERR_INVALID_ARGUMENT: n_sweeps < 0, params NULL or min_iou not finite or
 * outside (0, 1], host offsets that are NULL, do not start at 0 or decrease, device offsets NULL where the host's name boxes, NULL
 * or misaligned tables and outputs where data is required.  HIMO_ERR_UNSUPPORTED: a sweep of more than HIMO_BOXEVAL_MAX_BOXES boxes
 * on a side.  HIMO_ERR_WORKSPACE: a NULL, misaligned (16 bytes) or short workspace.  n_sweeps == 0 or no box at all: HIMO_OK,
 * nothing launched.
 * himo_box_iou_pairs: iou and iou3 of the listed pairs, d_pairs int64[n_pairs][2] = (row of A, row of B), d_iou double[n_pairs][2];
 * an index outside its table gives zeros for that pair.  One launch.  HIMO_ERR_INVALID_ARGUMENT: a negative count, NULL or misaligned
 * where data is required. */
typedef struct himo_boxeval_params {
    double min_iou;        /* the smallest BEV IoU of a candidate pair: finite, 0 < min_iou <= 1 */
    int32_t reserved[2];   /* 0 */
} himo_boxeval_params;

#define HIMO_BOXEVAL_MAX_BOXES 1024
#define HIMO_BOXEVAL_TILE 128      /* rects of B a pair-phase block stages in LDS (a size its tests straddle) */

size_t himo_boxeval_workspace_bytes(int n_sweeps, const int64_t* h_off_a, const int64_t* h_off_b);
int himo_boxeval_match(int n_sweeps, const double* d_rect_a, const int64_t* h_off_a, const int64_t* d_off_a, const double* d_rect_b,
                       const int64_t* h_off_b, const int64_t* d_off_b, const himo_boxeval_params* params, int32_t* d_match_a,
                       int32_t* d_match_b, double* d_iou_a, void* d_workspace, size_t workspace_bytes, void* stream);
int himo_box_iou_pairs(int64_t n_pairs, const double* d_rect_a, int64_t n_a, const double* d_rect_b, int64_t n_b, const int64_t* d_pairs,
                       double* d_iou, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Box tracking (`python -m himo_amd.track`, dataset `tracks_<name>`): identities of oriented boxes over the sweeps of a scene -- a
 * constant-velocity prediction, the rotated BEV IoU and greedy matching of box evaluation v1 between live tracks and a sweep's boxes,
 * an alpha-beta update, births and deaths (himo_amd/csrc/boxtrack.hip).  The reference has no such stage: this one follows the build's
 * own written rule, "box tracking, v1" (the module docstring of himo_amd/track.py is normative): PARITY UNPINNED.  Timed on synthetic
 * scenes only (profiles/box_track.txt); nothing has been tried on field data.
 *
 *   A detection row is double[12]: x, y, z, l, w, h, c, s, vx, vy, 0, 0 in the scene frame, (c, s) the unit heading.  The HOST makes
 *   them from box rows and poses (the library calls no transcendental).  INVALID (never matched, never a track, id -1): a value that
 *   is not finite or a negative extent.
 *   Scene n owns the sweeps h_sweep_off[n] .. h_sweep_off[n + 1] (int64[n_scenes + 1]); sweep k owns the rows h_det_off[k] ..
 *   h_det_off[k + 1] of d_det (int64[n_sweeps + 1]); both on the host for validation and on the device, where the copies are clamped
 *   to the host's totals and to the cap, not read back.  h_dt / d_dt double[n_sweeps]: the time from the sweep before; a scene's first
 *   is not read, every other must be finite and > 0.
 *   step      per live track px = x + vx dt, py likewise; the rects of tracks and detections as in box evaluation v1 with (c, s) given;
 *             BEV IoU with the track the subject; greedy matching at min_iou (greater IoU, then lower track slot, then lower j);
 *             matched: x = px + alpha (dx - px), z, l, w, h, c, s the detection's, vx = vx + beta (dvx - vx) [vel_mode 0] or vx + beta
 *             ((dx - px) / dt) [vel_mode 1], hits + 1, misses 0; unmatched: x = px, misses + 1, dead iff misses > max_age; an unmatched
 *             valid detection starts a track in ascending j with the scene's next id (from 0, never reused) while the table holds
 *             fewer than max_tracks, else id -1 and the scene's overflow count goes up; the table keeps its order, births behind.
 * Outputs, in the packed order: d_track_id int32[rows] (the id or -1), d_age int32[rows] (the track's hits after the step, 0 for -1),
 * d_state double[rows][4] (x, y, vx, vy of the track after the step, zeros for -1), d_iou double[rows] (the matched pair's BEV IoU, 0
 * for births and -1), d_live int32[n_sweeps] (live tracks after the step), d_scene_info int32[n_scenes][2] (ids issued, overflow).
 * The workspace is a slice per scene: the dense candidate matrix max_tracks x (the largest sweep of the call) x 8 bytes, the rects and
 * the track state (himo_boxtrack_workspace_bytes: 0 for what it refuses).  ONE launch (one per 32768 scenes), one 512-thread workgroup
 * per scene, asynchronous on `stream`, no host wait; the same inputs give the same bytes.
 * Refused, nothing launched and nothing written.  HIMO_ERR_INVALID_ARGUMENT: n_scenes < 0, params NULL or outside (min_iou finite in
 * (0, 1]; alpha, beta finite in [0, 1]; max_age 0..255; max_tracks 1..HIMO_BOXTRACK_MAX; vel_mode 0 or 1), host offsets that are NULL,
 * do not start at 0 or decrease, a dt that is read and is not finite and > 0, NULL or misaligned tables and outputs where data is
 * required.  HIMO_ERR_UNSUPPORTED: a sweep of more than HIMO_BOXTRACK_MAX boxes, more than 2^31 - 2 sweeps.  HIMO_ERR_WORKSPACE: a
 * NULL, misaligned (16 bytes) or short workspace.  n_scenes == 0: HIMO_OK, nothing launched.
 * himo_boxtrack_slabbed is himo_boxtrack with the scenes per launch given (>= 1): what the tests use to cross a launch boundary
 * without a large batch. */
typedef struct himo_boxtrack_params {
    double min_iou;        /* the smallest BEV IoU of a candidate pair: finite, 0 < min_iou <= 1 */
    double alpha;          /* position gain, finite, 0..1 */
    double beta;           /* velocity gain, finite, 0..1 */
    int32_t max_age;       /* a track dies after more than this many sweeps without a match, 0..255 */
    int32_t max_tracks;    /* live tracks of a scene, 1..HIMO_BOXTRACK_MAX */
    int32_t vel_mode;      /* 0: the velocity follows the boxes' ("box"); 1: it follows the position residual ("track") */
    int32_t reserved;      /* 0 */
} himo_boxtrack_params;

#define HIMO_BOXTRACK_MAX 512      /* live tracks of a scene and boxes of a sweep */

size_t himo_boxtrack_workspace_bytes(int n_scenes, const int64_t* h_sweep_off, const int64_t* h_det_off, const himo_boxtrack_params* params);
int himo_boxtrack(int n_scenes, const double* d_det, const int64_t* h_sweep_off, const int64_t* d_sweep_off, const int64_t* h_det_off,
                  const int64_t* d_det_off, const double* h_dt, const double* d_dt, const himo_boxtrack_params* params, int32_t* d_track_id,
                  int32_t* d_age, double* d_state, double* d_iou, int32_t* d_live, int32_t* d_scene_info, void* d_workspace,
                  size_t workspace_bytes, void* stream);
int himo_boxtrack_slabbed(int n_scenes, const double* d_det, const int64_t* h_sweep_off, const int64_t* d_sweep_off, const int64_t* h_det_off,
                          const int64_t* d_det_off, const double* h_dt, const double* d_dt, const himo_boxtrack_params* params,
                          int32_t* d_track_id, int32_t* d_age, double* d_state, double* d_iou, int32_t* d_live, int32_t* d_scene_info,
                          void* d_workspace, size_t workspace_bytes, int slab_scenes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Track-consistent flow (`python -m himo_amd.track_flow`, dataset `<name>_track`): the velocity of a box becomes the mean over its track
 * in a window of sweeps, and the points of the box are moved by it (himo_amd/csrc/trackflow.hip).  The reference has no such stage: this
 * one follows the build's own written rule, "track flow, v1" (the module docstring of himo_amd/track_flow.py is normative): PARITY
 * UNPINNED.  Timing (synthetic tables only, profiles/track_flow.txt; nothing has been tried on field data): 16 scenes of 150 sweeps of 300 boxes and
 * 120k points: plan 0.56 ms, apply 3.87 ms in 16 launches (1.96 x himo_accum_motion on the same rows); one 120k-row sweep applied alone 11.2 us.
 *
 *   The box tables are packed in the order of himo_boxtrack: scene n owns the sweeps h_sweep_off[n] .. h_sweep_off[n + 1], sweep k the
 *   rows h_det_off[k] .. h_det_off[k + 1] and scene n the words h_id_off[n] .. h_id_off[n + 1] of the workspace (one per track id of the
 *   scene: ids are 0 .. n_ids - 1); every table on the host for validation and on the device, where the copies are clamped to the host's
 *   totals and to the cap, not read back.  d_id int32[rows] (-1: no track), d_w double[rows][3] (the box velocity in the scene frame, made
 *   by the HOST), d_boxes float[rows][12] (columns 7..9: the float32 velocity in the sensor frame), d_U double[n_sweeps][9] (the rotation
 *   back into the sweep's sensor frame).  A row is USABLE iff 0 <= id < n_ids and w is finite.
 *   plan      L(id) = the USABLE rows of the scene with that id (integer atomics); a USABLE row of sweep k on a track with L >= min_len:
 *             S = 0, m = 0; for j = max(first, k - half) .. min(last, k + half) ascending, if sweep j holds a USABLE row of the id (the
 *             lowest such row) S += w_j, m += 1; wbar = S / m; u = U_k wbar, each component ((U0 x + U1 y) + U2 z); d_s = u sensor_dt;
 *             d_b = (double)v32 sensor_dt; STATIC (2) iff ((d_s.x^2 + d_s.y^2) + d_s.z^2) < motion_min^2, else MOVING (1); every other
 *             row NONE (0) with zeros.  d_state int32[rows], d_m int32[rows], d_shift float[rows][3] = (float)(d_s - d_b), d_disp
 *             float[rows][3] = (float)d_s, d_u double[rows][3].  One workgroup per (scene, sweep).
 *   apply     over the packed point rows of n_sweeps sweeps (h_pt_off int64[n_sweeps + 1] from 0; d_pc0 float[rows][pitch], pitch >= 3;
 *             d_flow float[rows][3]; d_label int32[rows]; d_E float[n_sweeps][12], the first three rows of inv(pose1) pose0); sweep k
 *             owns the plan rows h_box_off[k] .. h_box_off[k + 1] (absolute, at most n_box_rows), d_sorted_id / d_sorted_row int32 aligned
 *             with them: the sweep's label ids ascending (stable) and each one's row inside the sweep.  A row with label > 0 whose label
 *             is among the ids (the lowest row among equals), whose box is not NONE and whose three flow values are finite is rewritten:
 *             STATIC: a - pc0 with a = E pc0 (the arithmetic of himo_rigid_transform); MOVING, mode 0: flow + shift; MOVING, mode 1:
 *             (a - pc0) + disp; float32, every operation rounded.  Every other row keeps the bytes of its flow.  d_out float[rows][3];
 *             d_counts int32[n_sweeps][2]: rows written as MOVING, as STATIC.
 * Asynchronous on `stream`, no host wait; the only atomics are integer adds: the same inputs give the same bytes.
 * Refused, nothing launched and nothing written.  HIMO_ERR_INVALID_ARGUMENT: a negative count, pitch < 3, params NULL or outside (below),
 * host offsets that are NULL, do not start at 0 (h_box_off: are negative or pass n_box_rows) or decrease, NULL or misaligned tables and
 * outputs where data is required.  HIMO_ERR_UNSUPPORTED: a sweep of more than HIMO_BOXTRACK_MAX boxes, more than 2^31 - 2 sweeps or ids.
 * HIMO_ERR_WORKSPACE: a NULL, misaligned (16 bytes) or short workspace (himo_trackflow_workspace_bytes: 0 for what it refuses).
 * n_scenes == 0 / n_sweeps == 0: HIMO_OK, nothing launched. */
typedef struct himo_trackflow_params {
    double sensor_dt;      /* seconds between sweeps: finite, > 0 */
    double motion_min;     /* a box that moves less than this a sweep is STATIC [m]: finite, >= 0 */
    int32_t half;          /* the window is the sweeps k - half .. k + half, 0..8 */
    int32_t min_len;       /* a track with this many USABLE rows is CONFIRMED, >= 1 */
    int32_t mode;          /* MOVING rows: 0 flow + shift ("shift"), 1 the ego-motion flow + disp ("replace") */
    int32_t reserved;      /* 0 */
} himo_trackflow_params;

size_t himo_trackflow_workspace_bytes(int n_scenes, const int64_t* h_sweep_off, const int64_t* h_det_off, const int64_t* h_id_off);
int himo_trackflow_plan(int n_scenes, const int64_t* h_sweep_off, const int64_t* d_sweep_off, const int64_t* h_det_off,
                        const int64_t* d_det_off, const int64_t* h_id_off, const int64_t* d_id_off, const int32_t* d_id, const double* d_w,
                        const float* d_boxes, const double* d_U, const himo_trackflow_params* params, int32_t* d_state, int32_t* d_m,
                        float* d_shift, float* d_disp, double* d_u, void* d_workspace, size_t workspace_bytes, void* stream);
int himo_trackflow_apply(int n_sweeps, const int64_t* h_pt_off, const int64_t* d_pt_off, const float* d_pc0, int pitch, const float* d_flow,
                         const int32_t* d_label, const float* d_E, const int64_t* h_box_off, const int64_t* d_box_off, int64_t n_box_rows,
                         const int32_t* d_sorted_id, const int32_t* d_sorted_row, const int32_t* d_state, const float* d_shift,
                         const float* d_disp, const himo_trackflow_params* params, float* d_out, int32_t* d_counts, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a10: scene-flow network (voxelise -> encoder/decoder -> per-point flow).
 * The reference's implementation is in the absent OpenSceneFlow submodule: these
 * entry points have NO reference lines to cite beyond the call sites README.md:50 (`save.py`) and the
 * hyper-parameters at assets/slurm/ssl-train-av2.sh:32-33; the specification is himo_amd/seflow/spec.py.
 * All feature maps are NHWC float32 addressed as base + n*batch_stride + pixel*pitch + channel.
 */
/* One sweep: rigid transform (h_transform: row-major 4x4 float32), dynamic pillarisation on a
 * grid_w x grid_h grid (h_range = min xyz, h_voxel = cell size, h_centre_offset = voxel/2 + min as
 * float32), pillar feature net Linear(9,32)+BN+ReLU+mean -> 32 floats at d_image[cell * image_pitch] (every cell written;
 * d_image 16-byte aligned, image_pitch a multiple of 4 floats).
 * Also returns the transformed points, each point's cell (-1 = out of range) and its offset to the cell
 * centre.
 * The cell count grid_w * grid_h is taken in 64 bits (65536 x 65536 is 2^32 cells, not 0).  Refusals, in the order they are
 * checked, every one before anything is launched and with no output written:
 *   1. HIMO_ERR_INVALID_ARGUMENT  n < 0, pc_stride < 3, grid_w < 1 or grid_h < 1, a NULL host array, weight, image or
 *                                 workspace, a NULL point array or per-point output with n > 0;
 *   2. HIMO_ERR_UNSUPPORTED       n > 2^31 - 1, image_pitch < 32 or not a multiple of 4, d_image not 16-byte aligned, more
 *                                 than 1024 x 1024 = 1,048,576 cells (whatever workspace was passed);
 *   3. HIMO_ERR_WORKSPACE         a workspace that is not 16-byte aligned or shorter than the call needs
 *                                 (himo_pillar_workspace_bytes(n, ...) always suffices).
 * himo_pillar_workspace_bytes returns 0 for a point count or a grid that steps 1-2 refuse. */
size_t himo_pillar_workspace_bytes(int64_t max_points, int grid_w, int grid_h);
int himo_pillarize(int64_t n, const float* d_pts, int pc_stride, const float* h_transform,
                   const float* h_range, const float* h_voxel, const float* h_centre_offset,
                   int grid_w, int grid_h,
                   const float* d_pfn_weight, const float* d_pfn_scale, const float* d_pfn_shift,
                   float* d_xyz_t, int32_t* d_pid, float* d_offsets, float* d_image, int image_pitch,
                   void* d_workspace, size_t workspace_bytes, void* stream);
/* The sweeps of one sample (history, pc0, pc1) -- or of several samples, up to 12 sweeps -- through the same five launches: the stage's kernels are latency
 * chains on small grids, so sharing launches is worth ~2x on the stage.  Every sweep has its own outputs, image channel
 * group and workspace of `workspace_bytes` (himo_pillar_workspace_bytes of the largest sweep). */
typedef struct himo_sweep {
    int64_t n; const float* d_pts; int pc_stride;
    float transform[16];                                   /* row-major 4x4, sweep -> common frame */
    float* d_xyz_t; int32_t* d_pid; float* d_offsets;      /* per-point outputs as in himo_pillarize */
    float* d_image;                                        /* first of this sweep's 32 image channels */
    void* d_workspace;
    uint64_t* d_occupancy;                                 /* NULL, or grid_w * grid_h / 64 (rounded up) words, 8-byte aligned: bit c of
                                                              word w is set when cell 64 w + c holds a point of THIS pass -- the feature
                                                              kernel's own list of non-empty cells, every word written.  Not the
                                                              incremental-image bits of the workspace (those describe the previous
                                                              pass).  A himo_conv_desc.d_mask for the layers whose output is read at this
                                                              sweep's cells only.  Misaligned: HIMO_ERR_INVALID_ARGUMENT (step 1) */
} himo_sweep;
int himo_pillarize_multi(int n_sweeps, const himo_sweep* h_sweeps, const float* h_range, const float* h_voxel,
                         const float* h_centre_offset, int grid_w, int grid_h, const float* d_pfn_weight,
                         const float* d_pfn_scale, const float* d_pfn_shift, int image_pitch, size_t workspace_bytes,
                         void* stream);
/* image_split bit 0 (HIMO_IMAGE_SPLIT): each sweep's 32 image channels are written in the split activation format
 * (himo_conv_desc.act_layout; image_pitch a multiple of 16 floats, d_image 64-byte aligned); empty cells are zero either way.
 * bit 1 (HIMO_IMAGE_INCREMENTAL): the image persists between calls and only changes are written.  The last bytes of each
 * sweep's workspace (workspace_bytes a multiple of 16, constant per buffer) hold one bit per cell = "non-empty after the
 * previous call"; an empty cell that was empty then is already zero and is skipped -- two thirds of the zero rows of a
 * 120k-point sweep.  Contract: himo_pillar_occupancy_reset() once after allocating the workspace / image (marks every cell
 * dirty), and nobody else writes this sweep's image channels in between.
 * bit 2 (HIMO_PILLAR_NO_LISTS): nobody reads the per-cell ascending point lists of the workspace after this call (the training
 * backward pass and himo_head_scatter do; inference does not), so they need not be left there -- the workspace is still written.
 * With it a sweep may pass d_offsets == NULL and then gets no offsets written, by any kernel; d_xyz_t and d_pid stay required.
 * Without the bit a NULL d_offsets with n > 0 is refused as in himo_pillarize (step 1).  Every other output keeps its bits.
 * bit 3 (HIMO_PILLAR_HALFWAVE_ONLY): every non-empty cell takes the feature kernel's half-wave path (32 lanes = 32 channels per
 * cell) instead of one lane per cell for the cells of few points; same bits either way -- an A/B and test switch.
 * himo_pillarize and himo_pillarize_multi pass 0 for both.
 * Refusals of the multi-sweep forms (himo_pillar_features_multi included), in the order they are checked, nothing launched:
 *   1. HIMO_ERR_INVALID_ARGUMENT  n_sweeps outside [1, 12], h_sweeps NULL (himo_pillar_features_multi: d_scale / d_shift NULL);
 *                                 HIMO_IMAGE_SPLIT with image_pitch not a multiple of 16 or a sweep's d_image not 64-byte
 *                                 aligned; a sweep's d_occupancy not 8-byte aligned; two sweeps naming the same workspace
 *                                 (himo_pillarize_multi*);
 *   2. then sweep by sweep, steps 1-3 of himo_pillarize; with HIMO_IMAGE_INCREMENTAL step 3 (HIMO_ERR_WORKSPACE) also refuses a
 *      workspace_bytes that is not a multiple of 16 or leaves no room for the occupancy words behind the sweep's lists.
 * himo_pillar_occupancy_reset: HIMO_ERR_INVALID_ARGUMENT for a NULL workspace or a grid side < 1, HIMO_ERR_UNSUPPORTED beyond
 * 1,048,576 cells, HIMO_ERR_INVALID_ARGUMENT for a workspace shorter than the occupancy words; in that order. */
#define HIMO_IMAGE_SPLIT 1
#define HIMO_IMAGE_INCREMENTAL 2
#define HIMO_PILLAR_NO_LISTS 4
#define HIMO_PILLAR_HALFWAVE_ONLY 8
int himo_pillar_occupancy_reset(void* d_workspace, size_t workspace_bytes, int grid_w, int grid_h, void* stream);
int himo_pillarize_multi_ex(int n_sweeps, const himo_sweep* h_sweeps, const float* h_range, const float* h_voxel,
                         const float* h_centre_offset, int grid_w, int grid_h, const float* d_pfn_weight,
                         const float* d_pfn_scale, const float* d_pfn_shift, int image_pitch, size_t workspace_bytes, int image_split,
                         void* stream);

/* NHWC float32 convolution (ksize 3 pad 1 stride 1|2, or ksize 1) / row GEMM on v_mfma_f32_32x32x2_f32
 * with a fused epilogue. */
#define HIMO_EPI_BIAS 0          /* y = acc + bias */
#define HIMO_EPI_BIAS_BN_GELU 1  /* y = gelu((acc + bias) * scale + shift) */
#define HIMO_EPI_BIAS_GELU 2     /* y = gelu(acc + bias) */
#define HIMO_EPI_GRU_ZR 3        /* cols [0,C/2): y = sigmoid(.) (z); cols [C/2,C): aux_out = sigmoid(.) * aux_in (r*h) */
#define HIMO_EPI_GRU_Q 4         /* aux_out = (1 - aux_in) * aux_out + aux_in * tanh(acc + bias)   (aux_in = z, aux_out = h) */
#define HIMO_EPI_BIAS_RELU 5     /* y = max(acc + bias, 0) */
#define HIMO_EPI_RELU_MASK 6     /* y = aux_in > 0 ? acc : 0   (bias ignored: pass NULL) */
typedef struct himo_conv_desc {
    const float* x; int64_t x_batch_stride; int x_pitch;   /* input  (device) */
    const float* w;                                        /* [ksize][ksize][cin][cout] (device) */
    const float* bias; const float* scale; const float* shift;   /* [cout] (device; scale/shift for BN) */
    float* y; int64_t y_batch_stride; int y_pitch;         /* output (device) */
    int n, h, w_in, cin, cout, ksize, stride, epilogue;
    const float* aux_in; int aux_in_pitch;                 /* GRU epilogues, [rows][pitch] */
    float* aux_out; int aux_out_pitch;
    const void* w_packed;                                  /* optional: himo_conv_pack_weights[_ex] output; when set the
                                                              split-precision kernels run (stride 1, and 3x3 stride 2):
                                                              float32-class accuracy at a multiple of the float32-MFMA rate */
    int tile_hint;                                         /* 0 = library heuristic.  Every variant of a layer returns the same
                                                              bits; hints exist for callers that time them.  The full table
                                                              (csrc/conv_plan.h decides; `rows` = tile_hint & 15):
      value                 kernel family                     meaning                                 ignored / refused
      (64|128) << 4 | (1|2) LDS-staged weights: float32       channel tile 64|128, pixel tile         ignored (heuristic) when malformed or 128 with
                            (no w_packed; 3x3 stride 2), or   64|128                                  cout not a multiple of 128; 3x3 stride 1 packed
                            split precision on float32 maps                                           with packed_format 2 or a non-zero act_layout:
                            (1x1; pins it for 3x3 stride 1)                                           HIMO_ERR_UNSUPPORTED; on 3x3 stride 2 it selects
                                                                                                      the float32 kernel although w_packed is set
      0x1000 | 4|2|1        weights from L2 (3x3, packed,     image rows per wave (stride 2: 2|1,     a layer this family declines (GRU epilogues, an
                            float32 input map)                4 = heuristic)                          image of 2 GB or more): the LDS-staged kernel
                                                                                                      with its heuristic at stride 1, else refused
      0x1000 | 5|6          same, stride 1, packed_format     64-channel blocks forced (wide layers   packed_format 0, stride 2 or a declined layer:
                            1|2                               too), 1|2 rows per wave                 HIMO_ERR_UNSUPPORTED
      0x1000 | 9|10         same                              32-channel blocks, four pixel groups,   as 5|6
                                                              1|2 rows per wave
      0x1000 | other rows   same                              0, 3: heuristic                         rows > 4 otherwise: HIMO_ERR_UNSUPPORTED
      rows 4|2|1            split-format input                image rows (3x3 stride 1) / 32-pixel    4 on layers of <= 64 channels becomes 2; stride 2
      (any upper bits)      (HIMO_ACT_SPLIT_IN; 3x3 and 1x1)  segments (1x1) per wave                 has one variant per width class: ignored
      rows 8                same, 3x3 stride 1, cout <= 64    two 32-channel column tiles per wave,   ignored (heuristic) on wider layers or when the
                                                              8-row tiles                             output does not admit 16-byte stores
      rows 12               same, 3x3 stride 1, cout > 64     4 rows x 64 channels per wave           ignored (heuristic) likewise
      any value             same with HIMO_ACT_ROW_MASK       one variant (8 x 32 pixels x 64         ignored
                                                              channels, listed pixels only)
      anything else         --                                --                                      the tile is the heuristic's, but a non-zero value
                                                                                                      without 0x1000 still selects the family as the
                                                                                                      first row does (packed 3x3 layers) */
    int packed_format;                                     /* format of w_packed: 0 = three bf16 planes (float32 range,
                                                              6 matrix instructions per product block), 1 = two fp16
                                                              planes, x = h + l with weights packed x 2^6 (|values| < 65504,
                                                              3 matrix instructions): himo_conv_pack_weights_ex */
    int n_outer;                                           /* 0 | 1: `n` images; > 1: n * n_outer images, image i at
                                                              (i % n) * batch_stride + (i / n) * outer_stride -- the n
                                                              frames of a sample (channel groups) x the samples of a batch */
    int64_t x_outer_stride, y_outer_stride;
    int act_layout;                                        /* 0 = float32 activations; HIMO_ACT_SPLIT_IN | HIMO_ACT_SPLIT_OUT:
                                                              x / y in the split activation format (same addressing, every
                                                              16-channel group of a pixel = [16 fp16 high | 16 fp16 low]):
                                                              3x3 layers with packed_format 1, bias or bias+BN+GELU epilogue,
                                                              channel counts and pitches multiples of 16; SPLIT_IN: stride 1 */
    uint32_t* d_range_seen;                                /* HIMO_ACT_SPLIT_OUT only, may be NULL: the launch stores 1 into this
                                                              device word when one of the outputs it samples (one per lane and
                                                              block) has |y| >= 2^-6.  A two-term fp16 split keeps a value to
                                                              max(2^-25 absolute, 2^-23 relative): a layer whose word stays 0
                                                              after a forward pass sits on the absolute floor and the caller
                                                              should redo the pass in the bf16 split (pipeline.HiMoPipeline does) */
    const uint64_t* d_mask;                                /* HIMO_ACT_ROW_MASK: one bit per OUTPUT pixel -- bit c of 64-bit word w is
                                                              pixel 64 w + c of the image, pixels numbered iy * w_in + ix (the order of
                                                              himo_sweep.d_occupancy).  Only pixels whose bit is set are computed and
                                                              written; every other byte of y keeps what it held.  (h * w_in + 63) / 64
                                                              words per image, 8-byte aligned */
    int64_t mask_batch_stride, mask_outer_stride;          /* in 64-bit words: image i's mask starts at d_mask + (i % n) *
                                                              mask_batch_stride + (i / n) * mask_outer_stride, as x and y do */
} himo_conv_desc;
#define HIMO_ACT_SPLIT_IN 1
#define HIMO_ACT_SPLIT_OUT 2
#define HIMO_ACT_ROW_MASK 32    /* with HIMO_ACT_SPLIT_IN and nothing else: d_mask selects the output pixels (csrc/convsg.hip,
                                   conv3_rowmask_kernel; values bit-identical to the unmasked layer's).  Admitted: ksize 3, stride 1,
                                   packed_format HIMO_PACK_F16X2, bias or bias+BN+GELU epilogue, float32 output, cout <= 64, w_in a multiple
                                   of 32.  HIMO_ERR_INVALID_ARGUMENT for a NULL or misaligned d_mask, HIMO_ERR_UNSUPPORTED for every other
                                   descriptor that carries the bit; nothing is written either way */
#define HIMO_ACT_ACCUMULATE 8   /* alone: y += result instead of y = result -- float32 maps, 3x3 stride 1, packed_format HIMO_PACK_BF16X2,
                                   bias epilogue (the training step's stride-2 data gradients add into the decoder's skip gradient in place);
                                   also ksize 1 (row GEMM) with packed weights of either bf16 split and the bias epilogue, output map below
                                   2^30 elements (the decoder's skip gradient added to the pillar-image gradient the head's scatter wrote) */
#define HIMO_ACT_STUFFED_2X 16  /* alone or with HIMO_ACT_ACCUMULATE, same kernel: d_x is a COMPACT [h / 2][w_in / 2] map that the convolution
                                   reads as its zero-stuffed x2 image (x[2 i][2 j] = map[i][j], zeros elsewhere; h, w_in even = the stuffed
                                   size; x_batch_stride / x_pitch describe the compact map) -- the data gradient of a stride-2 convolution
                                   without materialising the stuffed image; matrix work on the all-zero rows is skipped */
/* (split-precision paths: one image -- h * w_in * x_pitch floats -- must stay below 2 GB: 32-bit byte offsets through a buffer resource;
 *  HIMO_ERR_UNSUPPORTED otherwise) */
int himo_conv2d(const himo_conv_desc* h_desc, void* stream);
/* one-time weight preparation for the split-bf16 path: [k][k][cin][cout] float32 -> three bf16 planes */
size_t himo_conv_packed_weight_bytes(int ksize, int cin, int cout);
int himo_conv_pack_weights(const float* d_w, int ksize, int cin, int cout, void* d_packed, void* stream);
#define HIMO_PACK_BF16X3 0
#define HIMO_PACK_F16X2 1
#define HIMO_PACK_BF16X2 2   /* two bf16 planes, x = h + m (16 significant bits, float32 range, three products per block): 3x3 layers and row GEMMs
                                (1x1) with float32 activation maps and the bias epilogue only -- the data gradients of the mixed-precision
                                training step */
int himo_conv_pack_weights_ex(const float* d_w, int ksize, int cin, int cout, int format, void* d_packed, void* stream);

/* bilinear x2 upsampling, align_corners = true; c channels of every pixel, NHWC with pitches */
int himo_upsample2x(const float* d_x, int x_pitch, int h, int w, int c, float* d_y, int y_pitch, void* stream);
int himo_upsample2x_batch(int n, const float* d_x, int64_t x_batch_stride, int x_pitch, int h, int w, int c, float* d_y,
                          int64_t y_batch_stride, int y_pitch, void* stream);
/* out_split != 0: y in the split activation format (himo_conv_desc.act_layout; c, y_pitch multiples of 16, d_y 64-byte aligned) */
int himo_upsample2x_batch_ex(int n, const float* d_x, int64_t x_batch_stride, int x_pitch, int h, int w, int c, float* d_y,
                             int64_t y_batch_stride, int y_pitch, int out_split, void* stream);

/* A prepared operator list (the static part of a forward pass: fixed buffers, shapes, weights) run from one call.
 * With HIMO_OPS_GRAPH the list is captured once into a hipGraph, keyed by the h_ops address and validated by a hash of
 * the list's bytes (a changed list is re-captured), and replayed with one hipGraphLaunch; himo_ops_release(h_ops)
 * frees the cached graph.  The graph path is
 * skipped while the himo_prof_* profiler is on, and falls back to plain launches if capture is not possible. */
#define HIMO_OP_CONV 0
#define HIMO_OP_UPSAMPLE2X 1
#define HIMO_OPS_GRAPH 0x1u
typedef struct himo_op {
    int kind;
    himo_conv_desc conv;                                   /* HIMO_OP_CONV */
    const float* up_x; int up_x_pitch, up_h, up_w, up_c;   /* HIMO_OP_UPSAMPLE2X: the arguments of himo_upsample2x_batch */
    float* up_y; int up_y_pitch;
    int up_n; int64_t up_x_batch_stride, up_y_batch_stride; /* up_n 0 | 1: one image */
    int up_out_split;                                       /* himo_upsample2x_batch_ex's out_split */
} himo_op;
int himo_run_ops(const himo_op* h_ops, int n_ops, unsigned flags, void* stream);
void himo_ops_release(const himo_op* h_ops);

/* The whole per-point head in one kernel (inference, split-bf16): gather -> `iters` GRU iterations -> Linear(192,32)+GELU
 * -> Linear(32,3) -> flow (pose_flow + residual for in-range points, pose_flow otherwise).  Same inputs and result as
 * himo_head_gather + the GRU row-GEMMs of himo_conv2d + himo_head_final; the hidden state never leaves the chip.
 * Fixed widths: hidden 128 (32 + 32 + 64 gathered channels), x 64.  Packed weights =
 * himo_conv_pack_weights_ex(w, 1, 192, cout, packed_format) of zr [192][256] (z | r), q [192][128], dec1 [192][32].  Specification: himo_amd/seflow/spec.py (reference absent). */
int himo_gru_head(int64_t n, const int32_t* d_pid, const float* d_offsets, const float* d_img0, const float* d_img1,
                  int img_pitch, const float* d_dec, int dec_pitch, const float* d_w_off, const float* d_b_off,
                  const void* d_wzr_packed, const float* d_bzr, const void* d_wq_packed, const float* d_bq,
                  const void* d_w1_packed, const float* d_b1, const float* d_w2, const float* d_b2,
                  const float* d_xyz_t, const float* d_pts, int pc_stride, float* d_flow, int iters, int packed_format,
                  void* stream);
/* The same over several samples in ONE launch (a sample's ~1900 blocks are 2.4 rounds on 256 CUs: per-sample launches
 * each end in a half-empty round).  Up to 16 samples; samples with n == 0 are skipped; weights shared.
 * img_split != 0 (packed_format 1 only): d_img0 / d_img1 rows are in the split activation format.  With packed_format 1
 * an image feature enters the head as its two-term fp16 value h + l in either layout, so both give the same bits. */
typedef struct himo_head_sample {
    int64_t n;
    const int32_t* d_pid; const float* d_offsets; const float* d_img0; const float* d_img1; const float* d_dec;
    const float* d_xyz_t; const float* d_pts; int pc_stride; float* d_flow;
} himo_head_sample;
int himo_gru_head_batch(int n_samples, const himo_head_sample* h_samples, int img_pitch, int dec_pitch,
                        const float* d_w_off, const float* d_b_off,
                        const void* d_wzr_packed, const float* d_bzr, const void* d_wq_packed, const float* d_bq,
                        const void* d_w1_packed, const float* d_b1, const float* d_w2, const float* d_b2,
                        int iters, int packed_format, int img_split, void* stream);
/* The same head with the 64 x-columns FOLDED: x = Linear(3,64)(offset) is an affine function of the point's offset o and
 * constant over the GRU iterations, so x W_x = [o, 1] [W_off W_x ; b_off W_x] is a K = 4 product.  The packed weights are
 * himo_conv_pack_weights_ex of [144][cout] matrices -- rows 0..127 the hidden rows of zr | q | dec1, rows 128..130
 * W_off W_x, row 131 b_off W_x, rows 132..143 zero -- and every GEMM of the head runs 9 slabs of 16 instead of 12.  Results
 * equal himo_gru_head_batch's up to float32 rounding of the folded rows. */
int himo_gru_head_batch_folded(int n_samples, const himo_head_sample* h_samples, int img_pitch, int dec_pitch,
                               const void* d_wzr_packed, const float* d_bzr, const void* d_wq_packed, const float* d_bq,
                               const void* d_w1_packed, const float* d_b1, const float* d_w2, const float* d_b2,
                               int iters, int packed_format, int img_split, void* stream);
/* himo_gru_head_batch (d_w_off / d_b_off given) or himo_gru_head_batch_folded (both NULL: folded [144][cout] weights) with the
 * finite-flow guard of the fp16-split arithmetic built into the output stage: *d_nonfinite (device uint32, may be NULL) is
 * OR-ed with 1 when any flow value this launch writes is NaN or infinite.  The caller clears the word (himo_clear_u32) before
 * the launches it wants covered.  Replaces the host framework's isfinite reduction over the flow buffer. */
int himo_gru_head_batch_guarded(int n_samples, const himo_head_sample* h_samples, int img_pitch, int dec_pitch,
                                const float* d_w_off, const float* d_b_off,
                                const void* d_wzr_packed, const float* d_bzr, const void* d_wq_packed, const float* d_bq,
                                const void* d_w1_packed, const float* d_b1, const float* d_w2, const float* d_b2,
                                int iters, int packed_format, int img_split, uint32_t* d_nonfinite, void* stream);
/* The head's TRAINING forward in one launch (BASELINE config 5; csrc/gruhead.hip with its saves enabled): gather -> `iters` (<= 4) GRU
 * iterations -> Linear(192,32) + GELU -> Linear(32,3), the explicit-x form of himo_gru_head_batch, writing the network's RESIDUAL flow
 * d_res [rows][4] (zeros for dropped points and in column 3) and every tensor the backward pass reads.  All saved buffers have
 * h_saved->rows rows per iteration, a multiple of 64 >= ceil(n / 64) * 64 (a caller may keep capacity beyond the current sweep).  d_w2 is [32][w2_pitch], w2_pitch 3 or 4.  Replaces, in the trainer, himo_head_gather + 2 * iters row
 * products (himo_conv2d) + 2 * iters gate kernels (himo_gru_gates_fwd) + the decoder.  Spec: himo_amd/seflow/spec.py steps 5-6
 * (reference model source absent: PARITY UNPINNED). */
typedef struct himo_head_saved {
    int64_t rows;              /* the row count of every buffer below = the stride between the stacked iterations: a multiple of 64,
                                  >= ceil(n / 64) * 64 */
    float* d_hx;               /* [iters + 1][rows][192]  [h_t | x], t = 0 .. iters */
    float* d_rhx;              /* [iters][rows][192]      [r_t h_t | x] */
    float* d_z; float* d_r; float* d_q;               /* [iters][rows][128] */
    float* d_pre1; float* d_y1;                       /* [rows][32] */
    float* d_res;                                     /* [rows][4] */
} himo_head_saved;
int himo_gru_head_train(int64_t n, const int32_t* d_pid, const float* d_offsets, const float* d_img0, const float* d_img1,
                        int img_pitch, const float* d_dec, int dec_pitch, const float* d_w_off, const float* d_b_off,
                        const void* d_wzr_packed, const float* d_bzr, const void* d_wq_packed, const float* d_bq,
                        const void* d_w1_packed, const float* d_b1, const float* d_w2, int w2_pitch, const float* d_b2,
                        int iters, int packed_format, const himo_head_saved* h_saved, uint32_t* d_nonfinite, void* stream);
/* Backpropagation through the head's GRU iterations in one launch (csrc/gruheadbwd.hip): d_dhx_last [rows][192] = d loss / d [h_T | x]
 * (from the decoder's backward) and the states himo_gru_head_train saved -> d_daq [iters][rows][128], d_dazr [iters][rows][256] (the gate
 * pre-activation gradients: the dz operands of the q / z|r weight-gradient products, zero in the padding rows) and d_dhx0 [rows][192] =
 * d loss / d [h_0 | x].  Every buffer has h_saved->rows rows (per iteration); the sweep writes whole 64-row blocks of the n points.  d_wq_t_packed / d_wzr_t_packed =
 * himo_weight_prepare_batch's flipped copies (ksize 1: the transposes) of q [192][128] and zr [192][256], packed_format
 * HIMO_PACK_BF16X3 or HIMO_PACK_BF16X2.  Replaces gru_bwd1/2/3 + two himo_conv2d row products per iteration. */
int himo_gru_head_backward(int64_t n, int iters, const float* d_dhx_last, const himo_head_saved* h_saved,
                           const void* d_wq_t_packed, const void* d_wzr_t_packed, int packed_format, float* d_daq,
                           float* d_dazr, float* d_dhx0, void* stream);
int himo_clear_u32(uint32_t* d_words, int n, void* stream);

/* per-point head glue: hx[i] = [img0[cell], img1[cell], dec[cell], Linear(3,64)(offset)] (192 floats; the 128 gathered
 * columns are zeros for dropped points, the 64 Linear columns are computed from the offset for every point, dropped or
 * not -- as himo_gru_head_train saves them), rhx[i][128:192] = the same Linear output */
int himo_head_gather(int64_t n, const int32_t* d_pid, const float* d_offsets, const float* d_img0,
                     const float* d_img1, int img_pitch, const float* d_dec, int dec_pitch,
                     const float* d_w_off, const float* d_b_off, float* d_hx, float* d_rhx, int pitch, void* stream);
/* flow[i] = (xyz_t[i] - pts[i]) + (cell >= 0 ? y1[i] @ w2 + b2 : 0): the (N,3) flow INCLUDING ego motion that
 * save_zip.py:117 consumes */
int himo_head_final(int64_t n, const float* d_y1, int y1_pitch, const float* d_w2, const float* d_b2,
                    const int32_t* d_pid, const float* d_xyz_t, const float* d_pts, int pc_stride,
                    float* d_flow, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a11: KNN/Chamfer correspondence + the self-supervised loss terms.  The reference's `seflowppLoss` is in the
 * absent OpenSceneFlow submodule; the only in-tree facts are the four term names and unit weights at
 * assets/slurm/ssl-train-av2.sh:33.  Definitions: himo_amd/csrc/sslloss.hip header (this build's own spec).
 */
/* exact k=1 NN between two sweeps through a uniform BEV grid (cell metres, grid_w x grid_h cells from
 * (x0, y0), at most 2^20 cells; points outside are binned into border cells).  float32 [n][3] in, squared distances + int32
 * reference rows out (idx may be NULL; -1 / +inf when nr == 0).  Ties keep the lowest reference row.  BOTH sets are
 * binned (the query side is searched in cell order, 64 neighbouring queries per block): the workspace is sized for
 * n_max = max(nq, nr). */
size_t himo_nn_grid_workspace_bytes(int64_t n_max, int grid_w, int grid_h);
int himo_nn_grid(int64_t nq, const float* d_q, int64_t nr, const float* d_r, float x0, float y0, float cell,
                 int grid_w, int grid_h, float* d_dist2, int32_t* d_idx, void* d_workspace,
                 size_t workspace_bytes, void* stream);
/* loss[0..3] = chamfer_dis, static_flow_loss, dynamic_chamfer_dis, cluster_based_pc0pc1; loss[4] = their sum
 * (float64, device); d_grad_flow [n0][3] = d loss[4] / d flow.  pc0 must already be in pc1's frame; labels:
 * 0 = static, > 0 = dynamic cluster id (< n_labels).  Synchronises the stream once internally. */
size_t himo_ssl_loss_workspace_bytes(int n0, int n1, int n_labels, int grid_w, int grid_h);
int himo_ssl_loss(int n0, int n1, const float* d_pc0, const float* d_pc1, const float* d_flow,
                  const int32_t* d_label0, const int32_t* d_label1, int n_labels,
                  float grid_x0, float grid_y0, float grid_cell, int grid_w, int grid_h,
                  double* d_loss, float* d_grad_flow, void* d_workspace, size_t workspace_bytes, void* stream);
/* ... with the raw correspondences pc0 -> pc1 supplied: d_raw_dist2 [n0] / d_raw_idx [n0] = himo_nn_grid(n0, d_pc0, n1, d_pc1) on the same
 * grid (they depend on the inputs only: a training step computes them beside its forward pass); both NULL = himo_ssl_loss. */
int himo_ssl_loss_ex(int n0, int n1, const float* d_pc0, const float* d_pc1, const float* d_flow,
                     const int32_t* d_label0, const int32_t* d_label1, int n_labels,
                     float grid_x0, float grid_y0, float grid_cell, int grid_w, int grid_h,
                     const float* d_raw_dist2, const int32_t* d_raw_idx,
                     double* d_loss, float* d_grad_flow, void* d_workspace, size_t workspace_bytes, void* stream);
/* ... and without the internal synchronisation: n_dyn0 / n_dyn1 = the number of points with label > 0 in d_label0 / d_label1, which
 * size the dynamic-subset searches (himo_ssl_loss_ex copies them back in the middle of the call -- in a training step that drains the
 * forward pass out of the queue before the backward pass can be enqueued).  himo_ssl_dyn_sizes counts them into d_counts [2] ahead of
 * time (they depend on the labels only; the caller copies them to pinned host memory beside the forward pass).  Sizes that do not
 * match the labels return every loss term as NaN.  (Reference: the loss of assets/slurm/ssl-train-av2.sh:33, source absent.) */
int himo_ssl_dyn_sizes(int n0, const int32_t* d_label0, int n1, const int32_t* d_label1, int32_t* d_counts, void* stream);
int himo_ssl_loss_presized(int n0, int n1, const float* d_pc0, const float* d_pc1, const float* d_flow,
                           const int32_t* d_label0, const int32_t* d_label1, int n_labels,
                           float grid_x0, float grid_y0, float grid_cell, int grid_w, int grid_h,
                           const float* d_raw_dist2, const int32_t* d_raw_idx, int n_dyn0, int n_dyn1,
                           double* d_loss, float* d_grad_flow, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The supervised loss on ground-truth flow: "DeFlow loss, v1" (himo_amd/csrc/deflowloss.hip, himo_amd/deflow_loss.py).
 * PARITY UNPINNED: the reference's `deflowLoss` is in the absent OpenSceneFlow submodule; this is the build's own written
 * rule after the published DeFlow formulation (end-point error averaged inside three speed bands, the bands summed), and no
 * claim is made about the reference's numbers.
 *
 * All arrays have n rows aligned 1:1 with pc0: d_pc0 raw pc0 xyz (float32, row pitch pc0_pitch >= 3 floats), d_moved [n][3]
 * the same points in pc1's frame as the network saw them, d_gt [n][3] the dataset's `flow` (ego motion included), d_est the
 * network's residual flow (row pitch est_pitch >= 3 floats), d_pid int32 or NULL (pid < 0: the row was dropped by the pillar
 * stage), d_valid uint8 or NULL (`flow_is_valid`), sensor_dt > 0 (0.1).  IEEE double on the float32 inputs, every operation
 * rounded on its own:
 *   1. a row is COUNTED when (d_pid is NULL or pid >= 0) and (d_valid is NULL or valid != 0) and gt is finite in all three
 *      components;
 *   2. g = (p + gt) - m, component by component (the ground-truth residual in pc1's frame = gt - pose_flow);
 *   3. s = sqrt((gx gx + gy gy) + gz gz);
 *   4. band 0 when s < 0.4 dt, band 1 when s <= 1.0 dt, band 2 otherwise (both products in double from (double)sensor_dt);
 *   5. d = est - g,  e = sqrt((dx dx + dy dy) + dz dz);
 *   6. term_b = mean of e over the counted rows of band b, 0 when the band is empty;  total = (term_0 + term_1) + term_2;
 *   7. d total / d est_i = (d_i / e_i) / count_band(i) for a counted row with e_i > 0, computed in double and rounded once to
 *      float32; exactly 0 for an uncounted row and for a counted row with e_i = 0.  A non-finite est in a counted row is not
 *      filtered: that row's gradient and the loss come out non-finite, other rows' gradients are unaffected.
 * d_loss [4] = the three terms and the total (float64, device), d_counts [3] = counted rows per band (int64, device), d_grad
 * [n][3] float32.  Sums are fixed-order trees and there are no atomics: loss and gradient are bit-identical from run to run.
 * Never synchronises, keeps nothing between calls.  n == 0: HIMO_OK, zero loss and zero counts, nothing else is touched.
 * HIMO_ERR_INVALID_ARGUMENT: n < 0, a pitch < 3, a NULL required array, sensor_dt not positive and finite; HIMO_ERR_UNSUPPORTED:
 * n > 2^31 - 1; HIMO_ERR_WORKSPACE: a NULL, misaligned (16 bytes) or short workspace (himo_deflow_loss_workspace_bytes(n)). */
size_t himo_deflow_loss_workspace_bytes(int64_t n);
int himo_deflow_loss(int64_t n, const float* d_pc0, int pc0_pitch, const float* d_moved, const float* d_gt,
                     const float* d_est, int est_pitch, const int32_t* d_pid /* nullable */,
                     const uint8_t* d_valid /* nullable */, float sensor_dt, double* d_loss /* [4]: three terms, total */,
                     int64_t* d_counts /* [3] */, float* d_grad /* [n][3] */, void* d_workspace, size_t workspace_bytes,
                     void* stream);

/* ---------------------------------------------------------------------------------------------
 * a12: optimisation-based scene flow ("fastnsf", README.md:53).  Reference implementation absent (OpenSceneFlow
 * submodule); specification in himo_amd/fastnsf.py.  The MLP forward / input-gradient products use himo_conv2d
 * (ksize 1) with HIMO_EPI_BIAS_RELU / HIMO_EPI_RELU_MASK; these are the fitting-specific pieces.
 */
/* dW[cin][cout] = X^T dZ and (optionally) db[cout] = column sums of dZ over n rows; cin, cout <= 128 */
size_t himo_wgrad_workspace_bytes(int64_t n_rows);
int himo_linear_wgrad(int64_t n, const float* d_x, int x_pitch, int cin, const float* d_dz, int z_pitch, int cout,
                      float* d_dw, float* d_db, void* d_workspace, size_t workspace_bytes, void* stream);
/* the same for any cin / cout (tiled 128 x 128); flags bit 0: accumulate into d_dw / d_db (BPTT over GRU iterations); bit 1 (2):
 * multiply split-bf16 operands (x = h + m, 16 significant bits, float32 sums) on the 16-bit matrix instructions */
size_t himo_wgrad_workspace_bytes_ex(int64_t n_rows, int cin, int cout);
int himo_linear_wgrad_ex(int64_t n, const float* d_x, int x_pitch, int cin, const float* d_dz, int z_pitch, int cout,
                         float* d_dw, float* d_db, unsigned flags, void* d_workspace, size_t workspace_bytes, void* stream);
int himo_transpose(const float* d_w, int rows, int cols, float* d_wt, void* stream);
/* torch.optim.Adam semantics (no weight decay, no amsgrad); step counts from 1 */
int himo_adam_step(int64_t n, float* d_param, const float* d_grad, float* d_m, float* d_v, float lr, float beta1,
                   float beta2, float eps, int step, void* stream);
/* loss = mean_i [d_a_i <= trunc^2] d_a_i + mean_j [d_b_j <= trunc^2] d_b_j on squared NN distances (from himo_nn_grid),
 * and d loss / d moved (correspondences constant).  The distances and indices are used as given: a term is kept iff d <= t2 with
 * t2 = trunc_dist * trunc_dist in float32 (NaN and +inf distances are dropped, and the index of a dropped term is not read); the
 * pc1 -> moved half is summed in 2^-40 fixed point, so the result does not depend on the order.  trunc_dist is only ever squared: a
 * negative one acts as its magnitude, a NaN one drops every term (himo_nsfp_objective refuses both).  n0 == 0 or n1 == 0: loss 0 and
 * a zero gradient; no correspondence is read and none need be passed.  A short workspace: HIMO_ERR_WORKSPACE. */
size_t himo_chamfer_trunc_workspace_bytes(int n0, int n1);
int himo_chamfer_trunc(int n0, int n1, const float* d_moved, const float* d_pc1, const float* d_dist_a,
                       const int32_t* d_idx_a, const float* d_dist_b, const int32_t* d_idx_b, float trunc_dist,
                       double* d_loss, float* d_grad_moved, void* d_workspace, size_t workspace_bytes, void* stream);
/* y[i][c] = a[i][c] + b_scale * b[i][c] for c < cols (b may be NULL); zero_tail clears y's columns cols..y_pitch-1 */
int himo_rows_add(int64_t n, int cols, const float* d_a, int a_pitch, const float* d_b, int b_pitch, float b_scale,
                  float* d_y, int y_pitch, int zero_tail, void* stream);
/* out[i][0:3] = R p_i + t with d_transform a DEVICE row-major 4x4 float32; the rest of each out row (out_pitch floats) is
 * zeroed.  Per row one rounded product, two fused multiply-adds and one rounded sum, in the order written in csrc/rigid_math.h
 * (the sequence this entry point has always computed; himo_accum_insert moves its rows with the same function) */
int himo_rigid_transform(int64_t n, const float* d_pts, int pc_stride, const float* d_transform, float* d_out,
                         int out_pitch, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a11, training side: element-wise pieces of the network's backward pass (csrc/train.hip).  The reference trains through
 * the absent OpenSceneFlow/train.py (assets/slurm/ssl-train-av2.sh:31); conventions in himo_amd/seflow/train.py.
 * Matrix products use himo_conv2d (row GEMM) and himo_linear_wgrad_ex.
 */
/* GRU cell, training forward.  which = 1: pre = [az | ar] (n x 256), hx = [h | x] (n x 192) -> z, r (n x 128),
 * out = [r * h | x].  which = 2: pre = aq (n x 128), z_in, hx -> q (n x 128), out = [(1 - z) h + z q | x]. */
int himo_gru_gates_fwd(int64_t n, int which, const float* d_pre, const float* d_z_in, const float* d_hx,
                       float* d_z, float* d_r, float* d_q, float* d_out, void* stream);
/* GRU cell, backward (three element-wise stages around the two transposed GEMMs; see csrc/train.hip) */
int himo_gru_bwd1(int64_t n, const float* d_dh_next, const float* d_z, const float* d_q, const float* d_hx,
                  float* d_daq, float* d_dz, float* d_dhp, void* stream);
int himo_gru_bwd2(int64_t n, const float* d_d_rhx, const float* d_hx, const float* d_z, const float* d_r,
                  const float* d_dz, float* d_dhp, float* d_dazr, float* d_dx, void* stream);
int himo_gru_bwd3(int64_t n, const float* d_d_hx, const float* d_dhp, float* d_dh, float* d_dx, void* stream);
/* pre = x * scale[c] + shift[c] (scale/shift NULL: identity), y = gelu(pre); and dx = dy * gelu'(pre) * scale[c] */
int himo_affine_gelu_fwd(int64_t rows, int ch, const float* d_x, int x_pitch, const float* d_scale, const float* d_shift,
                         float* d_pre, int pre_pitch, float* d_y, int y_pitch, void* stream);
int himo_affine_gelu_bwd(int64_t rows, int ch, const float* d_dy, int dy_pitch, const float* d_pre, int pre_pitch,
                         const float* d_scale, float* d_dx, int dx_pitch, void* stream);
/* zero the rows of v whose cell id is negative */
int himo_mask_rows(int64_t n, int cols, const int32_t* d_pid, float* d_v, int pitch, void* stream);
/* convolution backward: wf[k][k][cout][cin] = w[k][k][cin][cout] with mirrored taps (the data gradient of a stride-1 "same"
 * convolution is himo_conv2d of dY with wf); zero-stuffing of dY for the stride-2 layers; the adjoint of himo_upsample2x;
 * the 3x3 weight gradient of ONE image as a split-K MFMA product (flags bit 0: accumulate) */
int himo_weight_flip(const float* d_w, int ksize, int cin, int cout, float* d_wf, void* stream);
int himo_zero_stuff2x(int n_img, int h, int w, int c, const float* d_dy, int64_t dy_batch_stride, int dy_pitch,
                      float* d_z, int64_t z_batch_stride, int z_pitch, void* stream);
int himo_upsample2x_bwd(const float* d_dy, int dy_pitch, int h, int w, int c, float* d_dx, int dx_pitch, void* stream);
int himo_add2d(int64_t rows, int cols, const float* d_b, int b_pitch, float* d_y, int y_pitch, void* stream);   /* y += b */
/* column sums of a pitched [n][cout] matrix (bias gradients); workspace >= ceil(cout/128)*ceil(n/256)*512 bytes */
int himo_colsum(int64_t n, const float* d_z, int z_pitch, int cout, float* d_out, unsigned flags, void* d_workspace,
                size_t workspace_bytes, void* stream);
/* backward of the pillar stage; d_pillar_workspace = the workspace himo_pillarize(n, ...) of the same sweep left behind.
 * himo_pfn_backward: d loss / d pfn.weight [9][32] from the gradient of the sweep's 32 image channels (flags bit 0:
 * accumulate).  himo_head_scatter: adjoint of himo_head_gather -- per-point rows [d img0 | d img1 | d dec] (128 columns)
 * summed per pillar into channel groups group0 / group1 of d_db0 (other groups and empty cells zeroed) and d_ddec.
 * `n` MUST be the n of the forward call that filled d_pillar_workspace: the cell lists are located inside the workspace from
 * n (and the grid), so another n reads them from the wrong place.  The same holds for every h_n[i] of the himo_pfn_bn_stats* and
 * himo_pfn_backward_bn* forms below.  Nothing can check this; it is the caller's contract.
 * Refusals, in the order they are checked, nothing launched and no output written:
 *   himo_pfn_backward  1. HIMO_ERR_INVALID_ARGUMENT  n < 0, a grid side < 1, image_pitch < 32, a NULL argument (d_xyz_t may be
 *                                                    NULL when n == 0);
 *                      2. HIMO_ERR_UNSUPPORTED       n > 2^31 - 1, more than 1,048,576 cells (grid_w * grid_h in 64 bits);
 *                      3. HIMO_ERR_WORKSPACE         workspace_bytes < himo_pfn_backward_workspace_bytes().
 *   himo_head_scatter  1. HIMO_ERR_INVALID_ARGUMENT  n < 0, a grid side < 1, NULL d_pillar_workspace / d_db0 / d_ddec (d_dhx with
 *                                                    n > 0), dhx_pitch < 128, n_groups < 1, b0_pitch < 32 n_groups,
 *                                                    dec_pitch < 64; then group0 or group1 outside [0, n_groups), or
 *                                                    group0 == group1 (either would drop a sum silently; hence n_groups >= 2);
 *                      2. HIMO_ERR_UNSUPPORTED       n > 2^31 - 1, more than 1,048,576 cells. */
size_t himo_pfn_backward_workspace_bytes(void);
int himo_pfn_backward(int64_t n, const float* h_voxel, const float* h_centre_offset, int grid_w, int grid_h,
                      const float* d_pfn_weight, const float* d_pfn_scale, const float* d_pfn_shift,
                      const float* d_xyz_t, const void* d_pillar_workspace, const float* d_dimage, int image_pitch,
                      float* d_dweight, unsigned flags, void* d_workspace, size_t workspace_bytes, void* stream);
int himo_head_scatter(int64_t n, int grid_w, int grid_h, const void* d_pillar_workspace, const float* d_dhx, int dhx_pitch,
                      float* d_db0, int b0_pitch, int group0, int group1, int n_groups, float* d_ddec, int dec_pitch,
                      void* stream);

/* Every packed weight copy of a training step in ONE launch.  A job = himo_conv_pack_weights_ex(w, ksize, cin, cout, format) into
 * `packed`; with flip != 0 the copy is of the layer's DATA-GRADIENT weights instead -- taps mirrored and the channel roles swapped,
 * i.e. pack(wf, ksize, cout, cin) with wf[t][co][ci] = w[k*k-1-t][ci][co] (for ksize 1: the transpose).  The job table lives in DEVICE
 * memory (the caller uploads it once; the tensors it names are updated in place by the optimiser); first_block = the running sum
 * of himo_weight_job_blocks over the jobs before it, total_blocks the sum over all.  Spec: himo_amd/seflow/train.py (reference
 * absent: its training loop packs nothing). */
typedef struct himo_weight_job {
    const float* w;           /* [k][k][cin][cout] float32 */
    void* packed;             /* himo_conv_packed_weight_bytes(ksize, cin, cout) bytes (the same for the flipped form) */
    int ksize, cin, cout;
    int format;               /* HIMO_PACK_* */
    int flip;
    int first_block;
} himo_weight_job;
int himo_weight_job_blocks(int ksize, int cin, int cout, int flip);
int himo_weight_prepare_batch(const himo_weight_job* d_jobs, int n_jobs, int total_blocks, void* stream);

/* FastNSF's MLP after an optimiser step, ONE launch for all layers: every W [cin][cout] -> its fp16-split copy (format 1, forward
 * products) and the two-term bf16 copy of its transpose (format 2, input-gradient products); either destination may be NULL. */
int himo_mlp_repack(int n_layers, const float* const* h_w, const int* h_cin, const int* h_cout, void* const* h_fwd_packed,
                    void* const* h_bwd_packed, void* stream);

/* Self-supervised cluster labels (`+ssl_label=seflow_auto`, assets/slurm/ssl-train-av2.sh:32; the reference's generator is in the
 * absent OpenSceneFlow submodule: PARITY UNPINNED, specification himo_amd/seflow/ssl_label.py, oracle sklearn.cluster.DBSCAN):
 * DBSCAN(eps, min_pts) over 3-D points on the GPU (csrc/dbscan.hip).  d_xyz [n][pitch >= 3] float32; d_skip [n] bytes or NULL
 * (non-zero, a NaN or an infinite coordinate: the point takes no part); BEV cell grid of `cell` >= eps metres from (x0, y0), grid_w and
 * grid_h at most 32768 each and grid_w * grid_h at most 2^26; eps * eps must be a normal finite float; d_labels [n] int32: 0 = noise /
 * skipped, 1 .. K = clusters in the order of their lowest CORE point index (a border point joins the neighbouring cluster of lowest such
 * index): a pure function of the input.  d_n_clusters: K (or NULL).  HIMO_ERR_INVALID_ARGUMENT for arguments outside that,
 * HIMO_ERR_WORKSPACE for a workspace that is NULL, smaller than the query's size or not 16-byte aligned; n = 0 writes *d_n_clusters = 0. */
size_t himo_dbscan_workspace_bytes(int n, int grid_w, int grid_h);
int himo_dbscan(int n, const float* d_xyz, int pitch, const unsigned char* d_skip, float eps, int min_pts, float x0, float y0, float cell,
                int grid_w, int grid_h, int32_t* d_labels, int32_t* d_n_clusters, void* d_workspace, size_t workspace_bytes, void* stream);

/* HDBSCAN beside DBSCAN ("HDBSCAN, v1": this build's own rule, PARITY UNPINNED like its neighbours; the rule is written out in
 * csrc/hdbscan.hip and himo_amd/seflow/ssl_label.py, its restatement is tests/hdbscan_ref.py).  Two phases:
 *   himo_hdbscan_mst   (device, asynchronous, never synchronises) the minimum spanning tree of the mutual-reachability graph of the
 *                      participating points P under the strict edge order (w, lo, hi).  d_xyz [n][pitch >= 3] float32; d_skip [n] bytes or
 *                      NULL (non-zero, or a NaN coordinate: the point takes no part); 1 <= min_samples <= 32.  Writes d_counts [4] int32:
 *                      {|P|, edges emitted, Boruvka rounds taken, 0}; d_index [n] int32: the original indices of P, ascending, in its
 *                      first |P| entries; d_core2 [n] float32 or NULL: the squared core distance by ORIGINAL index, +inf for a point that
 *                      takes no part or has fewer than min_samples points around; d_edges [n - 1][3] uint32: {bits of the float32 weight
 *                      w, lo, hi} with lo < hi original indices, |P| - 1 of them in no particular order (none when |P| < max(min_samples,
 *                      2)).  The cost is quadratic in |P| per round, ceil(log2 n) rounds at most; core2 is a brute-force k-select.
 *   himo_hdbscan_tree  (host, plain C++, no HIP call) dendrogram, condensed tree, stabilities, excess-of-mass selection and labels from
 *                      HOST copies of d_index and d_edges: h_labels [n] int32: 0 = noise / no part, 1 .. K = clusters in the order of their
 *                      lowest point index; h_n_clusters: K (or NULL).  An edge list that is not a spanning tree of the n_part points
 *                      (wrong count, an index that is out of range or takes no part, lo >= hi, a weight that is no non-negative float, a
 *                      cycle) is refused with HIMO_ERR_INVALID_ARGUMENT; n_part < max(min_samples, 2) wants n_edges == 0 and labels all 0.
 * himo_hdbscan_workspace_bytes: grid_w, grid_h >= 1 are the BEV cell grid of a core-distance search that is not built (the brute-force
 * form keeps no cell table); 0 for arguments it refuses.  Errors as himo_dbscan: HIMO_ERR_INVALID_ARGUMENT, HIMO_ERR_WORKSPACE. */
size_t himo_hdbscan_workspace_bytes(int n, int grid_w, int grid_h);
int himo_hdbscan_mst(int n, const float* d_xyz, int pitch, const unsigned char* d_skip, int min_samples, int32_t* d_counts, int32_t* d_index,
                     float* d_core2, uint32_t* d_edges, void* d_workspace, size_t workspace_bytes, void* stream);
int himo_hdbscan_tree(int n, int n_part, const int32_t* h_index, int n_edges, const uint32_t* h_edges, int min_cluster_size, int min_samples,
                      int32_t* h_labels, int32_t* h_n_clusters);

/* FastNSF (README.md:53 `model=fastnsf`; specification himo_amd/fastnsf.py, PARITY UNPINNED) -- one optimiser iteration of the
 * coordinate MLP as THREE launches (csrc/nsffused.hip):
 *   himo_nsf_forward   the MLP over all points (activations spilled as two-term bf16 matrix fragments + ReLU mask bits for the backward
 *                      pass) and, when d_dout is given, the distance-transform objective of the moved points: d loss / d out
 *                      WITHOUT the 1 / (points in the volume) factor, per-tile loss and count sums, and the last layer's own
 *                      gradients per tile (into d_spill's tail);
 *   himo_nsf_backward  the whole chain of input gradients AND the gradient of every parameter, summed over each block of 256
 *                      points: d_partial [himo_nsf_backward_blocks(n)][partial_stride], each row laid out like the flat parameter
 *                      vector (h_off_w[i] / h_off_b[i]: float offsets of layer i's W [cin][cout] / b; i = 0 first (W [4][128]),
 *                      1 .. n_hidden - 1 hidden, n_hidden last (W [128][4]));
 *   himo_nsf_update    fixed-order sum of the block rows / (points in the volume) -> d_grad, one Adam step on d_param / d_m / d_v,
 *                      the packed copies of every hidden W (himo_mlp_repack's two formats), the loss and the count.
 * EVERY [n][.] buffer (d_x0, d_out, d_dout) holds himo_nsf_padded_rows(n) rows (whole blocks of 4 x 64 points, no bounds checks);
 * d_x0's padding rows must be zero.  d_spill: himo_nsf_spill_bytes(n, n_hidden).  2 <= n_hidden <= 12. */
int64_t himo_nsf_padded_rows(int64_t n);
size_t himo_nsf_spill_bytes(int64_t n, int n_hidden);
int himo_nsf_backward_blocks(int64_t n);
int himo_nsf_forward(int64_t n, const float* d_x0, int n_hidden, const float* d_w_first, const float* d_b_first,
                     const void* const* h_w_hidden_packed, const float* const* h_b_hidden, const float* d_w_last, const float* d_b_last,
                     void* d_spill, float* d_out, const float* h_origin, float cell, const int* h_dims, int window, const void* d_volume,
                     float trunc_dist, float* d_dout, double* d_loss_partial, int* d_count_partial, void* stream);
int himo_nsf_backward(int64_t n, const float* d_x0, const float* d_dout, int n_hidden, const void* const* h_wT_hidden_packed,
                      const float* d_w_last, const void* d_spill, const int* h_off_w, const int* h_off_b, int64_t partial_stride,
                      float* d_partial, void* stream);
int himo_nsf_update(int total, int n_partials, int64_t partial_stride, const float* d_partial, int n_fwd_blocks,
                    const double* d_loss_partial, const int* d_count_partial, float* d_param, float* d_grad, float* d_m, float* d_v,
                    float lr, float beta1, float beta2, float eps, int step, int n_hidden, const int* h_off_w, void* const* h_fwd_packed,
                    void* const* h_bwd_packed, double* d_loss, int* d_count, void* stream);

/* ---- NSFP, v1 (result key `nsfp`, tools/view_instance.py:155; the reference's implementation is in the absent OpenSceneFlow
 * submodule: PARITY UNPINNED, specification himo_amd/nsfp.py) -- the truncated-Chamfer objective on the fused MLP kernels above, and
 * the early-stopping / keep-best rule on the device (csrc/nsfp.hip).  An iteration is
 *   himo_nsf_forward_keep -> himo_nsfp_objective -> himo_nsf_last_grad -> himo_nsf_backward -> himo_nsf_update -> himo_nsfp_keep_best.
 * himo_nsf_forward_keep   himo_nsf_forward without an objective, which also leaves H_{L-1} (float32) in d_spill.
 * himo_nsf_last_grad      the per-tile last-layer gradients from that H_{L-1} and d_dout, where himo_nsf_backward reads them.
 * himo_nsfp_prepare       ONCE per sweep pair: d_pc1 [n1][3] binned on the search grid (as himo_nn_grid's: x0, y0, cell, grid_w, grid_h)
 *                         into d_workspace (himo_nsfp_workspace_bytes), which then belongs to the pair until its last objective step.
 * himo_nsfp_objective     moved = d_x0 + d_out (both [himo_nsf_padded_rows(n0)][4]) -> d_moved [n0][3]; both exact nearest-neighbour
 *                         searches (d_dist_a / d_idx_a [n0]: moved -> pc1, d_dist_b / d_idx_b [n1]: pc1 -> moved; squared distances,
 *                         ties to the lowest row); d_dout [padded][4] = n0 * d L / d out (padding rows zero) and
 *                         himo_nsfp_partials(n0, n1) loss / count entries whose sums himo_nsf_update divides: loss = L, gradient = dL.
 *                         The pc1 -> moved half is summed in 2^-40 fixed point: the result does not depend on the order.
 * himo_nsfp_keep_best     step >= 1 of the stop rule on d_state (8 float64: two slots of best, best_iter, stale, stopped_at; slot 0
 *                         starts +inf, 0, 0, 0; the state after step t is slot t & 1) with the loss *d_loss; copies d_out to
 *                         d_best_out (both [padded][4]) when the loss improved by more than min_delta.  patience <= 0 never stops.
 * n0 == 0: nothing is launched.  n1 == 0: loss 0, zero gradient.  Misaligned (16 bytes) buffers: HIMO_ERR_INVALID_ARGUMENT; a short
 * workspace: HIMO_ERR_WORKSPACE. */
int himo_nsf_forward_keep(int64_t n, const float* d_x0, int n_hidden, const float* d_w_first, const float* d_b_first,
                          const void* const* h_w_hidden_packed, const float* const* h_b_hidden, const float* d_w_last,
                          const float* d_b_last, void* d_spill, float* d_out, void* stream);
int himo_nsf_last_grad(int64_t n, int n_hidden, const float* d_dout, void* d_spill, void* stream);
size_t himo_nsfp_workspace_bytes(int64_t n0, int64_t n1, int grid_w, int grid_h);
int64_t himo_nsfp_partials(int64_t n0, int64_t n1);
int himo_nsfp_prepare(int64_t n0, int64_t n1, const float* d_pc1, float x0, float y0, float cell, int grid_w, int grid_h,
                      void* d_workspace, size_t workspace_bytes, void* stream);
int himo_nsfp_objective(int64_t n0, int64_t n1, const float* d_x0, const float* d_out, const float* d_pc1, float x0, float y0,
                        float cell, int grid_w, int grid_h, float trunc_dist, float* d_moved, float* d_dist_a, int32_t* d_idx_a,
                        float* d_dist_b, int32_t* d_idx_b, float* d_dout, double* d_loss_partial, int* d_count_partial,
                        void* d_workspace, size_t workspace_bytes, void* stream);
int himo_nsfp_keep_best(int64_t n, const float* d_out, float* d_best_out, const double* d_loss, double* d_state, int step,
                        int patience, double min_delta, void* stream);

/* FastNSF's coordinate MLP (3 -> 128 x n_hidden, ReLU -> 3; himo_amd/fastnsf.py) over all n points as ONE kernel per direction
 * (csrc/mlpfused.hip): the forward pass writes the post-ReLU activations h_H[k] [n][128] and d_out [n][4]; the backward pass turns
 * d_dout [n][4] into the masked gradients h_dZ[k] [n][128] at every hidden layer's output.  Hidden layer k = 1 .. n_hidden - 1 is
 * given by himo_mlp_repack's copies of W_k (forward: fp16 split) / W_k^T (backward: two-term bf16); entry 0 of those arrays is
 * ignored.  First layer W [4][128] and last layer W [128][4] are float32 (padded with zeros).  Replaces 17 row-GEMM launches.
 * EVERY [n][.] buffer must hold ceil(n / 64) * 64 rows (whole 64-row blocks, no bounds checks; pad d_x0 / d_dout with zeros). */
int himo_mlp_forward_fused(int64_t n, const float* d_x0, int n_hidden, const float* d_w_first, const float* d_b_first,
                           const void* const* h_w_hidden_packed, const float* const* h_b_hidden, const float* d_w_last,
                           const float* d_b_last, float* const* h_H, float* d_out, void* stream);
int himo_mlp_backward_fused(int64_t n, const float* d_dout, int n_hidden, const void* const* h_wT_hidden_packed,
                            const float* d_w_last, float* const* h_H, float* const* h_dZ, void* stream);
/* the same, also yielding the hidden layers' bias gradients h_db[k] [128] (column sums of dZ_k, taken while dZ_k passes through the kernel:
 * one reduction launch for all layers instead of a column-sum pass per layer); the padding rows of d_dout must be zero.
 * himo_mlp_bias_workspace_bytes(n, n_hidden) = max(n_hidden, 1) * ceil(n / 64) * 512 + 64; a workspace that is missing, shorter than
 * that or not 16-byte aligned is refused with HIMO_ERR_INVALID_ARGUMENT (not HIMO_ERR_WORKSPACE), as are n_hidden outside 1 .. 12, a
 * NULL h_H[k] / h_dZ[k] / h_db[k], a packed weight or d_x0 / d_dout / d_w_last off its 16-byte alignment; n == 0 writes nothing.
 * dZ_k is the same bits from either backward entry point. */
size_t himo_mlp_bias_workspace_bytes(int64_t n, int n_hidden);
int himo_mlp_backward_fused_bias(int64_t n, const float* d_dout, int n_hidden, const void* const* h_wT_hidden_packed,
                                 const float* d_w_last, float* const* h_H, float* const* h_dZ, float* const* h_db,
                                 void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- FastNSF's distance-transform objective (BASELINE config 4, `model=fastnsf`, README.md:53; implementation absent from the
 * reference tree: PARITY UNPINNED, specification in csrc/dtloss.hip / himo_amd/fastnsf.py).  himo_dt_build: ONCE per sweep pair, the
 * target sweep d_pc1 [n1][3] -> a volume of squared cell distances to the nearest occupied cell (uint16, x fastest, exact up to
 * `window` cells; h_dims = {nx, ny, nz}); d_volume holds himo_dt_volume_bytes() (two volumes: the passes ping-pong, the result is
 * the first).  himo_dt_loss: per optimiser iteration, loss = (1/n) sum [D <= trunc] D(moved_i) by trilinear lookup and its gradient
 * with respect to the moved points [n][3] -- what replaces the two exact NN searches + himo_chamfer_trunc of the NN objective. */
size_t himo_dt_volume_bytes(const int* h_dims);
int himo_dt_build(int n1, const float* d_pc1, const float* h_origin, float cell, const int* h_dims, int window,
                  void* d_volume, size_t volume_bytes, void* stream);
size_t himo_dt_loss_workspace_bytes(int n);
int himo_dt_loss(int n, const float* d_moved, const float* h_origin, float cell, const int* h_dims, int window,
                 const void* d_volume, float trunc_dist, double* d_loss, float* d_grad_moved, void* d_workspace,
                 size_t workspace_bytes, void* stream);

/* ---- BatchNorm in TRAINING mode (BASELINE config 5).  Replaces: the torch.nn.BatchNorm layers of the model the reference's
 * training job builds from scratch (assets/slurm/ssl-train-av2.sh:31-34: no checkpoint=, 12 epochs, batch_size=8; the model
 * source, OpenSceneFlow/, is absent -- PARITY UNPINNED, semantics = torch's: biased variance normalises, the unbiased one
 * feeds the running estimate, momentum 0.1).  Maps are NHWC float32 views [n_img][rows][ch]: element (i, r, c) at
 * p + i * img_stride + r * pitch + c (16-byte aligned bases, strides multiples of 4 floats, ch % 4 == 0).
 * himo_bn_train_fwd: batch mean / invstd over all n_img * rows rows -> d_mean, d_invstd [ch] (kept for the backward pass);
 *   d_xhat = (x - mean) * invstd (may alias d_x; NULL: not written, see himo_bn_train_bwd_x); d_y = gelu(gamma * xhat + beta); running statistics updated in place when
 *   given.  himo_bn_train_bwd: d_dy = d loss / d y -> d_dx = d loss / d x (the three-term BatchNorm gradient through the
 *   exact-erf GELU; may alias d_dy), d_dgamma / d_dbeta [ch] (flags bit 0: accumulate).  Every reduction is a fixed tree.
 * himo_bn_fold: eval-mode constants scale = gamma / sqrt(var + eps), shift = beta - mean * scale from the running statistics.
 * A single row (n_img * rows == 1), which torch refuses: var = 0, invstd = 1 / sqrt(eps), xhat = 0 and dx = 0, and the running
 *   variance takes var unchanged (there is no unbiased estimate): running_var <- (1 - momentum) running_var.
 * Status: HIMO_ERR_INVALID_ARGUMENT for n_img < 1, rows < 1, ch < 4, ch % 4 != 0, a NULL d_gamma / d_beta / d_mean (fwd, bwd_x) /
 *   d_invstd / d_dgamma / d_dbeta / d_workspace, exactly one of d_running_mean / d_running_var NULL, and for himo_bn_fold ch < 1 or
 *   any NULL pointer; HIMO_ERR_UNSUPPORTED for a map that is NULL (d_xhat of the forward pass excepted) or whose base is not
 *   16-byte aligned, img_stride % 4 != 0, pitch % 4 != 0, pitch < ch, and for n_img * rows * ch / 4 >= 2^31; HIMO_ERR_WORKSPACE
 *   for workspace_bytes < himo_bn_workspace_bytes(n_img * rows, ch) or a workspace that is not 16-byte aligned.  A refused call
 *   writes nothing.  himo_bn_workspace_bytes returns 0 for total_rows < 1 or ch < 1. */
size_t himo_bn_workspace_bytes(int64_t total_rows, int ch);
int himo_bn_train_fwd(int n_img, int64_t rows, int ch, const float* d_x, int64_t x_img_stride, int x_pitch,
                      const float* d_gamma, const float* d_beta, float eps, float momentum, float* d_running_mean,
                      float* d_running_var, float* d_mean, float* d_invstd, float* d_xhat, int64_t xhat_img_stride, int xhat_pitch,
                      float* d_y, int64_t y_img_stride, int y_pitch, void* d_workspace, size_t workspace_bytes, void* stream);
int himo_bn_train_bwd(int n_img, int64_t rows, int ch, const float* d_dy, int64_t dy_img_stride, int dy_pitch,
                      const float* d_xhat, int64_t xhat_img_stride, int xhat_pitch, const float* d_gamma, const float* d_beta,
                      const float* d_invstd, float* d_dx, int64_t dx_img_stride, int dx_pitch, float* d_dgamma, float* d_dbeta,
                      unsigned flags, void* d_workspace, size_t workspace_bytes, void* stream);
/* himo_bn_train_bwd from the layer's INPUT x (+ d_mean) instead of xhat: himo_bn_train_fwd may then be called with d_xhat = NULL and
 * writes 4 B per activation less; xhat is re-formed as the forward pass formed it (same results bit for bit). */
int himo_bn_train_bwd_x(int n_img, int64_t rows, int ch, const float* d_dy, int64_t dy_img_stride, int dy_pitch,
                        const float* d_x, int64_t x_img_stride, int x_pitch, const float* d_gamma, const float* d_beta,
                        const float* d_mean, const float* d_invstd, float* d_dx, int64_t dx_img_stride, int dx_pitch,
                        float* d_dgamma, float* d_dbeta, unsigned flags, void* d_workspace, size_t workspace_bytes, void* stream);
int himo_bn_fold(int ch, const float* d_gamma, const float* d_beta, const float* d_mean, const float* d_var, float eps,
                 float* d_scale, float* d_shift, void* stream);
/* The same for the pillar feature net's BatchNorm1d (statistics over the in-range points of ONE sweep; y = feats W):
 * himo_pfn_bn_stats reads the cell lists himo_pillarize* left in d_pillar_workspace and yields the sweep's constants
 *   d_scale = gamma invstd, d_shift = beta - mean gamma invstd [32] (+ d_mean, d_invstd for the backward pass; running
 *   statistics updated in place when given);
 * himo_pillar_features_multi re-runs ONLY the feature kernel of himo_pillarize_multi_ex with per-sweep constants
 *   (d_scale / d_shift: [n_sweeps][32]);
 * himo_pfn_backward_bn = himo_pfn_backward through the batch statistics, also yielding d gamma / d beta [32]. */
size_t himo_pfn_bn_workspace_bytes(void);
/* the same for the n_sweeps (<= 12) sweeps of a sample in one call: host arrays of per-sweep point counts, d_xyz_t and pillar
 * workspaces (and, backward, image-gradient bases); d_scale / d_shift / d_mean / d_invstd are [n_sweeps][32]; the running statistics
 * (forward) and d_dweight / d_dgamma / d_dbeta (backward) are updated sweep after sweep, so the results have the bits of n_sweeps single
 * calls.  Workspace: n_sweeps * himo_pfn_bn_workspace_bytes(). */
/* ... and for the sweeps of a per-process BATCH (the reference launcher's batch_size=8 on one process, assets/slurm/ssl-train-av2.sh:32-34):
 * sweep i belongs to GROUP i % n_groups, and a group shares ONE set of statistics -- with the sweeps ordered sample-major, frame-minor
 * and n_groups = the frames per sample, group f is frame slot f of every sample: what one call of the pillar net on a batch of sweeps
 * normalises over (torch.nn.BatchNorm1d on the concatenated points).  d_scale / d_shift / d_mean / d_invstd are [n_groups][32]; up to 16
 * sweeps per group; the _multi forms are these with every sweep its own group.  Workspace: n_sweeps * himo_pfn_bn_workspace_bytes().
 * An empty group (no in-range point in any member): constants from the running statistics (mean 0, variance 1 when not tracked),
 * d_mean = d_invstd = 0, running statistics untouched.  h_n[i] is the n of sweep i's forward call (see himo_pfn_backward).
 * Refusals, in the order they are checked, nothing launched and no output written:
 *   1. HIMO_ERR_INVALID_ARGUMENT  n_sweeps < 1, n_groups < 1, n_sweeps % n_groups != 0, more than 16 sweeps per group (the _multi
 *                                 forms: n_sweeps > 12; the backward form: n_sweeps > 192), a NULL host array or output, exactly one
 *                                 of d_running_mean / d_running_var NULL, image_pitch < 32 (backward), a grid side < 1;
 *   2. HIMO_ERR_UNSUPPORTED       more than 1,048,576 cells (grid_w * grid_h in 64 bits), more than 192 groups;
 *   3. HIMO_ERR_WORKSPACE         workspace_bytes < n_sweeps * himo_pfn_bn_workspace_bytes();
 *   4. then sweep by sweep: HIMO_ERR_INVALID_ARGUMENT for h_n[i] < 0, a NULL weight, pillar workspace, workspace (image gradient,
 *      backward) or d_xyz_t with h_n[i] > 0; HIMO_ERR_UNSUPPORTED for h_n[i] > 2^31 - 1; HIMO_ERR_WORKSPACE for a d_workspace that
 *      is not 16-byte aligned. */
int himo_pfn_bn_stats_groups(int n_sweeps, int n_groups, const int64_t* h_n, const float* const* h_xyz_t,
                             const void* const* h_pillar_workspace, const float* h_voxel, const float* h_centre_offset, int grid_w,
                             int grid_h, const float* d_pfn_weight, const float* d_gamma, const float* d_beta, float eps, float momentum,
                             float* d_running_mean, float* d_running_var, float* d_scale, float* d_shift, float* d_mean, float* d_invstd,
                             void* d_workspace, size_t workspace_bytes, void* stream);
int himo_pfn_backward_bn_groups(int n_sweeps, int n_groups, const int64_t* h_n, const float* const* h_xyz_t,
                                const void* const* h_pillar_workspace, const float* const* h_dimage, int image_pitch, const float* h_voxel,
                                const float* h_centre_offset, int grid_w, int grid_h, const float* d_pfn_weight, const float* d_scale,
                                const float* d_shift, const float* d_mean, const float* d_invstd, float* d_dweight, float* d_dgamma,
                                float* d_dbeta, unsigned flags, void* d_workspace, size_t workspace_bytes, void* stream);
int himo_pfn_bn_stats_multi(int n_sweeps, const int64_t* h_n, const float* const* h_xyz_t, const void* const* h_pillar_workspace,
                            const float* h_voxel, const float* h_centre_offset, int grid_w, int grid_h,
                            const float* d_pfn_weight, const float* d_gamma, const float* d_beta, float eps, float momentum,
                            float* d_running_mean, float* d_running_var, float* d_scale, float* d_shift, float* d_mean,
                            float* d_invstd, void* d_workspace, size_t workspace_bytes, void* stream);
int himo_pfn_backward_bn_multi(int n_sweeps, const int64_t* h_n, const float* const* h_xyz_t, const void* const* h_pillar_workspace,
                               const float* const* h_dimage, int image_pitch, const float* h_voxel, const float* h_centre_offset,
                               int grid_w, int grid_h, const float* d_pfn_weight, const float* d_scale, const float* d_shift,
                               const float* d_mean, const float* d_invstd, float* d_dweight, float* d_dgamma, float* d_dbeta,
                               unsigned flags, void* d_workspace, size_t workspace_bytes, void* stream);
int himo_pfn_bn_stats(int64_t n, const float* h_voxel, const float* h_centre_offset, int grid_w, int grid_h,
                      const float* d_pfn_weight, const float* d_xyz_t, const void* d_pillar_workspace, const float* d_gamma,
                      const float* d_beta, float eps, float momentum, float* d_running_mean, float* d_running_var,
                      float* d_scale, float* d_shift, float* d_mean, float* d_invstd, void* d_workspace, size_t workspace_bytes,
                      void* stream);
int himo_pillar_features_multi(int n_sweeps, const himo_sweep* h_sweeps, const float* h_range, const float* h_voxel,
                               const float* h_centre_offset, int grid_w, int grid_h, const float* d_pfn_weight,
                               const float* d_scale, const float* d_shift, int image_pitch, size_t workspace_bytes,
                               int image_split, void* stream);
int himo_pfn_backward_bn(int64_t n, const float* h_voxel, const float* h_centre_offset, int grid_w, int grid_h,
                         const float* d_pfn_weight, const float* d_scale, const float* d_shift, const float* d_mean,
                         const float* d_invstd, const float* d_xyz_t, const void* d_pillar_workspace, const float* d_dimage,
                         int image_pitch, float* d_dweight, float* d_dgamma, float* d_dbeta, unsigned flags, void* d_workspace,
                         size_t workspace_bytes, void* stream);
/* the 3x3 weight gradient over a batch of images, LDS-tiled (dY tile + X halo staged once, all 9 taps read them);
 * h, w = INPUT image size.  stride 1: h even, w % 32 == 0, cin % 64 == 0; stride 2: h even, w % 64 == 0, cin == 32 or
 * cin % 64 == 0; cout % 64 == 0 -- HIMO_ERR_UNSUPPORTED otherwise (workspace_bytes returns 0).
 * flags bit 0: accumulate into d_dw; bit 1 (2): stride-1 layers multiply split-bf16 operands (x = h + m, 16 significant bits,
 * float32 accumulation) on the 16-bit matrix instructions instead of float32 ones; bit 2 (4): the launch runs BESIDE another stream's
 * kernels -- one block per CU instead of two, so that the other stream's blocks find registers and LDS on every CU (results differ
 * from the two-block launch only in the summation order of the pixel chunks) */
size_t himo_conv_wgrad_batch_workspace_bytes(int n_img, int h, int w, int cin, int cout, int stride);
int himo_conv3x3_wgrad_batch(int n_img, const float* d_x, int64_t x_batch_stride, int x_pitch, int h, int w, int cin,
                             const float* d_dy, int64_t dy_batch_stride, int dy_pitch, int cout, int stride, float* d_dw,
                             unsigned flags, void* d_workspace, size_t workspace_bytes, void* stream);
/* the same with the layer's BIAS gradient d_db [cout] (column sums of dY) from the same pass over dY: stride 1 with flags bit 1 only
 * (HIMO_ERR_UNSUPPORTED otherwise; himo_colsum is the stand-alone form); flags bit 0 accumulates into both.  Same workspace. */
int himo_conv3x3_wgrad_batch_bias(int n_img, const float* d_x, int64_t x_batch_stride, int x_pitch, int h, int w, int cin,
                                  const float* d_dy, int64_t dy_batch_stride, int dy_pitch, int cout, int stride, float* d_dw,
                                  float* d_db, unsigned flags, void* d_workspace, size_t workspace_bytes, void* stream);
size_t himo_conv_wgrad_workspace_bytes(int ho, int wo, int cin, int cout);
int himo_conv3x3_wgrad(const float* d_x, int x_pitch, int h, int w, int cin, const float* d_dy, int dy_pitch, int cout,
                       int stride, float* d_dw, unsigned flags, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a9 helper (host memory, no GPU): LZ4-frame decoder for the compressed buffers of Feather V2 files as pandas /
 * pyarrow write them (save_zip.py:81 `to_feather`).  Returns the decompressed size, or -1. */
int64_t himo_lz4_frame_decompress(const void* h_src, int64_t n, void* h_dst, int64_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* HIMO_AMD_H */
