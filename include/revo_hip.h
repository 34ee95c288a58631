/*
 * revo_hip.h -- C ABI of the MI355X-native REVO hot path (librevo_hip.so).
 *
 * The reference (fabianschenk/REVO) has no FFI/plugin layer: its hot path is a
 * set of C++ classes (ImgPyramidRGBD, TrackerNew, Optimizer) linked into one
 * executable.  This header is the drop-in boundary for that method surface:
 * plain pointers and sizes, POD structs, no Eigen / cv / torch types.  Every
 * entry point cites the reference interface it replaces (paths relative to the
 * reference tree).  The header-only C++ adapters in revo_amd/cpp/ re-create the
 * reference class names on top of it.
 *
 * Conventions
 *   - return value 0 = REVO_OK, negative = error; revo_last_error() gives text
 *     (thread-local).  The reference has no error codes (log + exit(0) /
 *     assert / Sophus abort()); the adapters translate.
 *   - R is a 3x3 rotation in COLUMN-major order (Eigen::Matrix3f storage),
 *     T a 3-vector; together they map CURRENT-frame points into the
 *     KEYFRAME (tracker.cpp:286-288, optimizer.cpp:93).
 *   - 4x4 poses are column-major (Eigen::Matrix4f storage).
 *   - images are row-major with a byte stride (cv::Mat layout).
 *   - level 0 = full resolution (PYR_MAX_LVL), level PYR_MIN_LVL = coarsest.
 *   - every call does hipSetDevice(ctx device) itself; a pyramid may be created
 *     on one host thread and consumed on another (iowrapperRGBD.cpp:279 vs
 *     system.cpp:188), but one handle must not be used concurrently.
 */
#ifndef REVO_HIP_H
#define REVO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* librevo_hip.so is built with hidden visibility: what this header declares is all it exports */
#pragma GCC visibility push(default)

#define REVO_MAX_LEVELS 6 /* optimizer.h:37 PYRAMID_LEVELS */

/* ---- error codes ------------------------------------------------------- */
enum {
  REVO_OK = 0,
  REVO_ERR_INVALID_ARG = -1,
  REVO_ERR_HIP = -2,          /* a HIP runtime call failed / no device        */
  REVO_ERR_NOT_KEYFRAME = -3, /* imgpyramidrgbd.h:113-116 "optimizationStructure not built" */
  REVO_ERR_NOT_ORTHOGONAL = -4, /* Sophus SO3(R) ENSURE, so3.hpp:419-424       */
  REVO_ERR_CAPACITY = -5,
  REVO_ERR_LEVEL = -6,        /* assert(lvl < size) in imgpyramidrgbd.h:59-94  */
  REVO_ERR_UNSUPPORTED = -7,  /* a valid PNG the device decoder does not handle (revo_png_*) */
  REVO_ERR_CORRUPT = -8       /* a malformed PNG / zlib stream (revo_png_*)     */
};

/* TrackerNew::TrackerStatus, tracker.h:61-66 */
enum {
  REVO_TRACKER_STATE_OK = 0,
  REVO_TRACKER_STATE_LOST = 1,
  REVO_TRACKER_STATE_NEW_KF = 2,
  REVO_TRACKER_STATE_UNKNOWN = 3
};

/* ---- settings (POD mirrors of the reference's settings classes) -------- */

/* ImgPyramidSettings, camerapyr.h:27-89 (+ Camera, camerapyr.h:90-111). */
typedef struct revo_pyr_settings {
  int32_t width, height;             /* camerapyr.h:49-52 (640x480)          */
  float fx, fy, cx, cy;              /* camerapyr.h:54-61 (level-0 K)        */
  int32_t pyr_min_lvl;               /* coarsest level, camerapyr.h:45 (2)   */
  int32_t pyr_max_lvl;               /* finest level,   camerapyr.h:46 (0); must be 0 */
  int32_t canny_threshold1;          /* camerapyr.h:40 (150)                 */
  int32_t canny_threshold2;          /* camerapyr.h:41 (100)                 */
  float depth_min, depth_max;        /* camerapyr.h:43-44 (0.1, 5.2)         */
  int32_t use_edge_hist;             /* camerapyr.h:62 (1)                   */
  float n_percentage;                /* camerapyr.h:63 (0.3)                 */
  /* distPatchSizes, imgpyramidrgbd.cpp:50: {20,10,5}.  The reference indexes
   * this 3-entry vector with the level, so levels >= 3 are undefined there;
   * here 0 means "no histogram / no fill-in at this level". */
  int32_t hist_patch[REVO_MAX_LEVELS];
} revo_pyr_settings;
/* Geometry accepted by revo_ctx_create (anything else is REVO_ERR_INVALID_ARG with a message): width a
 * multiple of 4*2^(levels-1) and <= 2048, height a multiple of 2^(levels-1) and <= 2048, at most 2048 tiles of 32 x 32
 * pixels (1920x1080 and 1280x1024 fit), at most REVO_MAX_LEVELS levels, every level a multiple of 16 pixels (640x480: up to
 * 5 levels, 1280x960: 6), hist_patch[l] dividing into <= 128 tiles per row.  The reference itself truncates any size
 * (camerapyr.h:98-103). */

/* OptimizerSettings, optimizer.h:42-112 (only the fields the hot path reads). */
typedef struct revo_opt_settings {
  float lambda_success_fac;                  /* optimizer.h:53 (0.5)  */
  float lambda_fail_fac;                     /* optimizer.h:54 (2.0)  */
  float lambda_initial[REVO_MAX_LEVELS];     /* optimizer.h:63 (0)    */
  float step_size_min[REVO_MAX_LEVELS];      /* optimizer.h:55 (1e-16)*/
  float convergence_eps[REVO_MAX_LEVELS];    /* optimizer.h:65 (0.999)*/
  int32_t max_its_per_lvl[REVO_MAX_LEVELS];  /* optimizer.h:56 (100)  */
  float edge_distance_lvl[REVO_MAX_LEVELS];  /* optimizer.h:59 {30,20,10,5,5,5} */
  float huber_edge;                          /* optimizer.h:75 (0.3)  */
  int32_t use_edge_filter;                   /* tracker.h:46 (1)      */
} revo_opt_settings;

/* TrackerSettings, tracker.h:31-55 (+ TrackerNew::histogramLevel, tracker.cpp:229). */
typedef struct revo_tracker_settings {
  int32_t check_tracking_results;   /* tracker.h:45 (1) */
  int32_t check_init_values;        /* tracker.h:43 (1) */
  int32_t n_frames_hist_voting;     /* tracker.h:47 (3); the vote uses min(n, past clouds, 3) clouds, the oldest first:
                                       values above 3 vote like 3 (the reference would throw std::out_of_range from
                                       histWeights.at(4), tracker.cpp:179); below 3 it never asks for a new keyframe
                                       (hsize < 4, tracker.cpp:184) */
  int32_t histogram_level;          /* tracker.cpp:229 (2) */
} revo_tracker_settings;

/* Optimizer::ResidualInfo, optimizer.h:118-140. */
typedef struct revo_residual_info {
  int32_t good_pts_edges;
  int32_t bad_pts_edges;
  float sum_error_unweighted;
  float sum_error_weighted;
} revo_residual_info;

/* Values of config/dataset_tum1.yaml + config/revo_settings.yaml +
 * OptimizerSettings() defaults. */
void revo_pyr_settings_default(revo_pyr_settings* s);
void revo_opt_settings_default(revo_opt_settings* s);
void revo_tracker_settings_default(revo_tracker_settings* s);

/* ---- handles ------------------------------------------------------------ */
typedef struct revo_ctx revo_ctx;     /* CameraPyr + TrackerNew + Optimizer state */
typedef struct revo_pyr revo_pyr;     /* one ImgPyramidRGBD                       */
typedef struct revo_batch revo_batch; /* B independent frame-pairs, device resident */

const char* revo_last_error(void);
/* "x.y.z gfx950" */
const char* revo_version(void);

/* REVO::REVO -> new CameraPyr(settingsPyr) (camerapyr.h:117-164), new
 * TrackerNew(settingsTracker, settingsPyr) (tracker.cpp:225-235) which owns the
 * Optimizer (optimizer.cpp:44-61).  device = HIP device ordinal. */
int revo_ctx_create(int device, const revo_pyr_settings* pyr,
                    const revo_opt_settings* opt,
                    const revo_tracker_settings* trk, revo_ctx** out);
void revo_ctx_destroy(revo_ctx* ctx);
/* TrackerNew(const TrackerSettings&, const ImgPyramidSettings&) (tracker.cpp:225-235)
 * is constructed AFTER CameraPyr and the IO thread in the reference
 * (system.cpp:96,107): applies tracker/optimizer settings to an existing ctx and, like the
 * reference's constructor, starts with empty past lists (the clouds of an earlier tracker are dropped). */
int revo_ctx_set_tracker(revo_ctx* ctx, const revo_opt_settings* opt,
                         const revo_tracker_settings* trk);

/* TrackerNew::histogramLevel (tracker.h:67, tracker.cpp:229). */
int revo_ctx_histogram_level(const revo_ctx* ctx);

/* Exact-sums mode (off by default).  On: the tracker forms the reference's own per-point float terms
 * (calculateWarpUpdate, LGS6::update) and every sum it compares or solves with -- the 27 entries of the
 * normal equations, the error sums of every LM candidate, the init-check costs -- is the float nearest
 * the exact sum of those terms, whatever the cluster size, batch size, speculation depth or stream count
 * (DESIGN 4.1 states the guarantee).  Poses, evaluation counts and keyframe decisions then depend on the
 * inputs alone.  The flag is read by each tracker launch: it applies from the next single-pair call,
 * batch, pipeline step or revo_vo frame of this context; a revo_vo_multi handle keeps the value it had
 * when it was created.  Returns REVO_OK / the flag (0 or 1), or an error / -1 for a null context. */
int revo_ctx_set_exact_sums(revo_ctx* ctx, int on);
int revo_ctx_exact_sums(const revo_ctx* ctx);

/* Camera(fx,fy,cx,cy,w,h,scale) for level lvl, camerapyr.h:98-103,139-144:
 * out6 = {fx,fy,cx,cy,width,height}. */
int revo_ctx_camera(const revo_ctx* ctx, int lvl, float out6[6]);

/* ---- ImgPyramidRGBD ------------------------------------------------------ */

/* ImgPyramidRGBD(settings, camPyr, fullResRgb [BGR8], fullResDepth [f32 metres],
 * timestamp), imgpyramidrgbd.cpp:43-96.  Inputs are copied before returning
 * (the reference clones them, cpp:51,54), so the caller may reuse its buffers.
 * Strides in bytes. */
int revo_pyramid_create(revo_ctx* ctx, const uint8_t* bgr, size_t bgr_stride,
                        const float* depth_m, size_t depth_stride,
                        double timestamp, revo_pyr** out);
/* Same, fusing iowrapperRGBD.cpp:326-327: depth = u16 * (float)(1/scale). */
int revo_pyramid_create_u16(revo_ctx* ctx, const uint8_t* bgr, size_t bgr_stride,
                            const uint16_t* depth_raw, size_t depth_stride,
                            double depth_scale_factor, double timestamp,
                            revo_pyr** out);
/* ~ImgPyramidRGBD, imgpyramidrgbd.cpp:32-41 */
void revo_pyramid_destroy(revo_pyr* pyr);
/* ImgPyramidRGBD::makeKeyframe, imgpyramidrgbd.cpp:231-252: exact Euclidean
 * distance transform + (-dDT/dx, -dDT/dy, DT, 0) float4 table per level. */
int revo_pyramid_make_keyframe(revo_pyr* pyr);
int revo_pyramid_is_keyframe(const revo_pyr* pyr);
double revo_pyramid_timestamp(const revo_pyr* pyr); /* imgpyramidrgbd.h:97-100 */

/* Accessor planes (imgpyramidrgbd.h:45-117). */
typedef enum revo_plane {
  REVO_PLANE_GRAY = 0,       /* returnGray(lvl)            u8  W*H            */
  REVO_PLANE_DEPTH = 1,      /* returnDepth(lvl)           f32 W*H            */
  REVO_PLANE_EDGES = 2,      /* returnEdges(lvl)           u8  W*H {0,255}    */
  REVO_PLANE_EDGES_ORIG = 3, /* returnOrigEdges(lvl)       u8  W*H {0,255}    */
  REVO_PLANE_DT = 4,         /* returnDistTransform(lvl)   f32 W*H (keyframe) */
  REVO_PLANE_GRADTABLE = 5,  /* returnOptimizationStructure(lvl) f32 4*W*H    */
  REVO_PLANE_EDGES3D = 6,    /* return3DEdges(lvl)         f32 4*N col-major  */
  REVO_PLANE_HIST = 7,       /* histPyr[lvl]               u8  (H/P)*(W/P)    */
  REVO_PLANE_EDGES3D_TILED = 8 /* the same N points as EDGES3D in the order the tracker reads them (32x32-pixel tiles in raster
                                  order, row-major inside a tile): what the per-frame build writes; EDGES3D is derived on demand */
} revo_plane;

/* Lazy device->host read of one accessor plane.  cap_bytes = size of host_dst;
 * *count = number of ELEMENTS written (pixels; 3-D points for EDGES3D).
 * host_dst may be NULL to query *count only. */
int revo_pyramid_read(revo_pyr* pyr, revo_plane what, int lvl, void* host_dst,
                      size_t cap_bytes, size_t* count);

/* ImgPyramidRGBD::generateColoredPcl(lvl, clrPcl, densePcl) (imgpyramidrgbd.cpp:279-327), the
 * cloud REVO::start hands to the viewer / PLY export per keyframe (system.cpp:165,235):
 * 8 floats per point (X,Y,Z,1, r,g,b,1 with colours in [0,1]), x-outer / y-inner order;
 * dense != 0: every pixel with a usable depth, else edge pixels only.  dst8 == NULL only
 * counts.  Single-frame pyramids only (batch views keep no colour image). */
int revo_pyramid_colored_pcl(revo_pyr* p, int lvl, int dense, float* dst8, size_t cap_points, size_t* count);

/* ---- Optimizer ------------------------------------------------------------ */

/* float Optimizer::trackFrames(ref, curr, R, T, lvl, resInfo),
 * optimizer.cpp:235-311: the LM loop of ONE pyramid level, run on the device.
 * R,T in/out; *err = last accepted mean weighted residual. */
int revo_optimizer_track_level(revo_ctx* ctx, const revo_pyr* ref,
                               const revo_pyr* curr, float R_colmajor[9],
                               float T[3], int lvl, revo_residual_info* info,
                               float* err);

/* Optimizer::calcErrorAndBuffers + calculateWarpUpdate at a fixed pose
 * (optimizer.cpp:74-234), exposed for parity tests: A (6x6 row==col major,
 * symmetric), b (6) and error are the LGS6 members after finish()
 * (LGSX.h:320-326). */
int revo_optimizer_eval(revo_ctx* ctx, const revo_pyr* ref, const revo_pyr* curr,
                        const float R_colmajor[9], const float T[3], int lvl,
                        revo_residual_info* info, float* err, float A[36],
                        float b[6]);

/* Eigen::Matrix<float,6,1> inc = A.ldlt().solve(b) after A(i,i) *= 1 + LM_lambda (optimizer.cpp:258-262), as the
 * tracker kernel computes it (float LDL^T pivoted on the largest |diagonal|, pseudo-inverse of D), for n systems:
 * in = n x 43 floats {A[36] symmetric, b[6], lambda}, x6 = n x 6.  Exposed for the parity tests of the solver. */
int revo_optimizer_solve6(revo_ctx* ctx, int n, const float* A36_b6_lambda, float* x6);

/* ---- TrackerNew ------------------------------------------------------------ */

/* TrackerStatus TrackerNew::trackFrames(R, T, error, refFrame, currFrame),
 * tracker.cpp:294-353: init check (265-283, 357-393) + coarse-to-fine loop.
 * iters_per_lvl (may be NULL) receives the number of residual evaluations
 * (calls of calcErrorAndBuffers) per level -- the E_l of SURVEY 8(d). */
int revo_tracker_track_frames(revo_ctx* ctx, const revo_pyr* ref,
                              const revo_pyr* curr, float R_colmajor[9],
                              float T[3], float* err, int* status,
                              revo_residual_info* info,
                              int32_t iters_per_lvl[REVO_MAX_LEVELS]);

/* TrackerStatus TrackerNew::assessTrackingQuality(estimatedPose, currFrame),
 * tracker.cpp:118-201.  hist4/overlaps4 (may be NULL) receive the counts. */
int revo_tracker_assess_quality(revo_ctx* ctx, const float T_w_curr_colmajor[16],
                                const revo_pyr* curr, int* status,
                                int32_t hist4[4], int32_t overlaps4[4]);
/* void TrackerNew::addOldPclAndPose(pcl, worldPose, timeStamp),
 * tracker.cpp:209-223: pcl = src->return3DEdges(lvl) (kept on the device). */
int revo_tracker_add_old_pcl(revo_ctx* ctx, const revo_pyr* src, int lvl,
                             const float T_w_colmajor[16], double timestamp);
/* The same with the cloud in HOST memory, exactly the reference's signature
 * addOldPclAndPose(const Eigen::MatrixXf& pcl, ...): pcl = 4 x n column-major floats (X,Y,Z,1 per point), copied
 * (the reference copies the matrix, tracker.cpp:219). */
int revo_tracker_add_old_pcl_host(revo_ctx* ctx, const float* pcl_4xn_colmajor, size_t n,
                                  const float T_w_colmajor[16], double timestamp);
/* void TrackerNew::clearUpPastLists(), tracker.cpp:248-257 */
int revo_tracker_clear_past(revo_ctx* ctx);
int revo_tracker_past_size(const revo_ctx* ctx);

/* ---- batched independent frame-pairs (new) -------------------- */

/* One record per pair, 96 bytes. */
typedef struct revo_pair_result {
  float R[9];       /* column-major, curr -> ref */
  float T[3];
  float err;        /* last level's mean weighted residual */
  int32_t good, bad;
  int32_t status;   /* tracker.cpp:351-352 */
  int32_t evals[REVO_MAX_LEVELS]; /* residual evaluations per level */
  int32_t flags;    /* bit0: init pose reset to identity (tracker.cpp:277-282);
                       bit1: non-orthogonal input R (the single-pair calls return REVO_ERR_NOT_ORTHOGONAL);
                       bit2: evaluation cap hit (6000 residual evaluations; the reference's bound is 100 outer
                             iterations x unbounded retries) -- pose is the last accepted one;
                       bit3: the workgroups of this pair could not exchange their partial sums in time (not
                             co-resident, e.g. the device is shared): R, T are NOT valid (the single-pair
                             calls return REVO_ERR_HIP) */
  int32_t n_pts0;   /* N_0 of the current frame */
} revo_pair_result;

/* A batch owns device storage for 2*n_pairs pyramids (ref, curr). */
int revo_batch_create(revo_ctx* ctx, int n_pairs, revo_batch** out);
void revo_batch_destroy(revo_batch* b);
/* Device-resident inputs: d_bgr [2*n_pairs][H][W][3] u8, d_depth
 * [2*n_pairs][H][W] f32 metres; frame 2*i = reference (keyframe) of pair i,
 * frame 2*i+1 = current.  h_init_RT: n_pairs x 12 floats (R col-major, T) on
 * the HOST or NULL for identity.  d_results: n_pairs revo_pair_result records
 * in DEVICE memory.  stream: hipStream_t (NULL = the batch's own stream).
 * Enqueues: pyramid build of all frames, keyframe promotion of the refs,
 * TrackerNew::trackFrames of every pair.  Asynchronous. */
int revo_batch_track(revo_batch* b, const uint8_t* d_bgr, const float* d_depth,
                     const float* h_init_RT, revo_pair_result* d_results,
                     void* stream);
/* Stage-wise variants used by bench.py for per-kernel timing.
 * What a build leaves to later (default; REVO_DEFER=0 or REVO_EDT_DEFER=0, read by revo_batch_create, builds everything
 * for every frame at once): the tracker reads a pair's CURRENT frame only through its edge lists and its KEYFRAME only
 * through its distance transforms.  So the depth levels >= 1 and the edge lists of the current frames (odd) and the distance
 * transforms of the keyframes (even) are built by the batch's first consumer (revo_batch_prepare), and the depth levels >= 1,
 * the depth-validity bits and the edge lists of the keyframe-role frames (even) only when somebody asks for them: any
 * accessor or single-pair / vote call on an even view of revo_batch_frame.  The same kernels run on the same inputs
 * either way: every plane, list and record is bit-identical to an eager build's.  That late work reads the edge maps and
 * level 0 of the depth pyramid, so the next revo_batch_build* of the batch is ordered behind it by the library.
 * The BYTE edge planes of such a batch (REVO_PLANE_EDGES, REVO_PLANE_EDGES_ORIG: edgesPyr / edgesOrigPyr) are produced on
 * first access as well: the build ends at the edge bitmaps, which are all the tracker's inputs are made from, and the first
 * accessor, vote, reference-ordered edge list or map call that reads a byte plane through a view of revo_batch_frame expands
 * them for all frames of the batch (one streaming kernel, behind fill-in).  revo_batch_sync does not.  Same bytes as an
 * eager build's. */
int revo_batch_build(revo_batch* b, const uint8_t* d_bgr, const float* d_depth,
                     void* stream);
/* revo_batch_build without the copy of the depth input: level 0 of the depth pyramid IS d_depth (the reference's
 * level 0 is the input image as well, imgpyramidrgbd.cpp:62-64).  d_depth must stay valid and unchanged until the
 * batch is built again or destroyed -- accessors, the tracker's point lists and the keyframe promotion read it, and so
 * does the work an even view triggers on first access (above), whenever that access comes. */
int revo_batch_build_borrow(revo_batch* b, const uint8_t* d_bgr, const float* d_depth,
                            void* stream);
/* revo_batch_build for raw uint16 depth [2*n_pairs][H][W] (depth = raw * (float)(1/scale),
 * iowrapperRGBD.cpp:326-327, fused into the first build kernel). */
int revo_batch_build_u16(revo_batch* b, const uint8_t* d_bgr, const uint16_t* d_depth_raw,
                         double depth_scale_factor, void* stream);
int revo_batch_track_only(revo_batch* b, const float* h_init_RT,
                          revo_pair_result* d_results, void* stream);
/* Runs, on `stream`, whatever part of the last build was left to the batch's first consumer (default: the depth levels >= 1 of the
 * pyramid, imgpyramidrgbd.h:218-249, which only the edge lists read, and the 3-D edge lists, imgpyramidrgbd.cpp:199-226, of the
 * CURRENT frames 1, 3, 5, ...; the distance transforms, imgpyramidrgbd.cpp:231-252, of the keyframes 0, 2, 4, ... -- the build
 * stream is the critical one of a pipelined caller).  It does not build the keyframe-role frames' own edge lists: no tracker
 * grid of the batch reads them (an even view does, on first access).  revo_batch_track_only does this itself on ITS stream; call this first to run that work
 * on another stream (the library orders every later consumer and the next build of the batch behind it) or to keep it outside a
 * timed tracker launch.  On a stream other than the build's it waits for the build.  No-op when nothing is pending. */
int revo_batch_prepare(revo_batch* b, void* stream);
/* Waits for `stream` (NULL = the batch's own), runs whatever the last build still left pending for the tracker (as
 * revo_batch_prepare: not the keyframe-role frames' edge lists), waits for the batch's last
 * tracker grid WHEREVER it ran, and decodes the flags of that grid's records: a record with bit 3 makes the call return
 * REVO_ERR_HIP.  Lifetime contract: the d_results buffer of the last revo_batch_track_only / revo_batch_track must stay
 * valid (not freed, not reused for something else) until this call or the batch's next tracker launch -- the call reads it.
 * A later revo_batch_build* does not end that obligation (a pipelined caller builds step k+1 before it syncs step k). */
int revo_batch_sync(revo_batch* b, void* stream);
/* Pyramid view of frame f of the batch (owned by the batch).  A view of an even frame builds that role's depth levels >= 1
 * and edge lists on its first use after a build (all even frames in one go, on the context's stream, behind the build);
 * what it returns is what a single-frame pyramid of the same input returns. */
int revo_batch_frame(revo_batch* b, int frame, revo_pyr** out);
/* Time one launch of the dominant (tracker) kernel with HIP events on its own
 * stream: returns the mean duration in ms over `reps` launches. */
int revo_batch_time_tracker(revo_batch* b, const float* h_init_RT,
                            revo_pair_result* d_results, void* stream, int reps,
                            float* ms_mean);

/* Measurement aid (bench.py's per-kernel roofline table): every kernel of revo_batch_build_borrow + revo_batch_prepare run
 * ALONE on the batch's own stream with HIP events between the launches; us[i] = mean duration of stage i over `reps` passes
 * (event to event: kernel + a few us of dispatch), name[i] = the kernel ("hysteresis" = k_hyst, or the banded kernels where a
 * level takes that path).  Every launch covers all 2*n_pairs frames (n_pairs keyframes for the distance transforms), whatever
 * a pipelined build would leave for later.  Leaves the batch built, every frame's edge lists included. */
#define REVO_MAX_STAGES 24
typedef struct revo_stage_times {
  int32_t n;
  float us[REVO_MAX_STAGES];
  char name[REVO_MAX_STAGES][32];
} revo_stage_times;
int revo_batch_profile_build(revo_batch* b, const uint8_t* d_bgr, const float* d_depth, int reps, revo_stage_times* out);

/* ---- the information matrix and covariance of tracked poses (new) --------------------------------------
 * What the tracker minimises at a pose (R, T) of one level is sum_i w_i r_i^2 over the GOOD points of the current
 * frame (optimizer.cpp:74-191); its normal equations are H x = -g with H = sum_i w_i v_i v_i^T, g = sum_i v_i (r_i w_i)
 * (calculateWarpUpdate + LGS6::update, optimizer.cpp:192-234, LGSX.h:392-398).  H is the Gauss-Newton information
 * matrix of the relative pose, up to the residual variance; revo_pair_info_covariance turns it into a covariance.
 * Unknown order is LGS6's: translation 0-2, rotation 3-5, the tangent parameters of the increment the LM solves for
 * (optimizer.cpp:258-266): the update is T_new = exp(x) * T_old -- applied on the LEFT, i.e. in the KEYFRAME's frame
 * (se3_exp_mul in revo_amd/csrc/revo_track.hip, called with the accepted pose as its right factor).
 * The per-point terms are exactly those of exact-sums mode (revo_ctx_set_exact_sums): the reference's own
 * float terms (v_a*v_c)*w, v_a*(r*w), (r*r)*w, r*r with v[3], v[4] evaluated in double and rounded once.  Each of the
 * 29 sums is the float nearest the exact sum of its float terms (DESIGN 4.1's midpoint caveat applies) -- whatever
 * the context's exact_sums flag, the batch size, the grid shape or the stream.  Consequence: in exact-sums mode
 * revo_optimizer_eval's A[a][c] equals H/(float)good and its b[a] equals -(g/(float)good), bit for bit. */
typedef struct revo_pair_info {      /* 192 bytes, little-endian, no padding holes */
  float   H[21];    /* upper triangle, row-major (00,01,..,05,11,..,55) of sum_i (v_a*v_c)*w over the good points */
  float   g[6];     /* sum_i v_a*(r*w)   (LGS6's b is minus this, LGSX.h:392-398)                                   */
  float   sum_w;    /* sum_i (r*r)*w                                                                               */
  float   sum_u;    /* sum_i r*r                                                                                   */
  int32_t good, bad;/* Optimizer::ResidualInfo counts at this pose and level                                       */
  int32_t level;
  int32_t flags;    /* bit0: no evaluation (pose not finite / not orthogonal, or the source record had bit1 or bit3):
                       the record is then all zero except level, flags, R and T                                    */
  float   R[9], T[3]; /* the pose the sums were taken at (curr -> keyframe, column-major), copied from the input   */
  int32_t reserved[3]; /* zero */
} revo_pair_info;

/* The level-lvl information of all n_pairs pairs of a batch in ONE launch.  Exactly one of d_results (n_pairs records in
 * DEVICE memory, e.g. the ones the batch's grid just wrote; the kernel reads the poses itself, a record with flag bit1 or
 * bit3 gives flags bit0) and h_RT (n_pairs x 12 HOST floats: R column-major, T) is non-NULL, else REVO_ERR_INVALID_ARG.  A host
 * pose that is not finite or not orthogonal (the test revo_tracker_track_frames applies) gives that pair flags bit0; the
 * call still returns REVO_OK.  d_info: n_pairs records in device memory, 16-byte aligned.  lvl outside the pyramid:
 * REVO_ERR_LEVEL.  Asynchronous on `stream` (NULL = the batch's own).  Like revo_batch_track_only it first runs, on its
 * stream, whatever the last build left pending for the tracker (never the keyframe-role frames' edge lists) and orders
 * itself behind the batch's last tracker grid; the batch's next build waits for it.  It reads what the tracker reads: the
 * current frames' tile-ordered edge lists and the keyframes' distance transforms.  On a revo_pipeline_batch batch, call it
 * with the after_grid_stream of the step's submit: the information of step t rides in the after-grid slot. */
int revo_batch_pair_info(revo_batch* b, const revo_pair_result* d_results, const float* h_RT, int lvl,
                         revo_pair_info* d_info, void* stream);
/* One pair, host output, waits.  REVO_ERR_NOT_KEYFRAME / REVO_ERR_NOT_ORTHOGONAL / REVO_ERR_LEVEL as the other single-pair
 * calls; a T that is not finite is REVO_ERR_INVALID_ARG. */
int revo_tracker_pair_info(revo_ctx* ctx, const revo_pyr* ref, const revo_pyr* curr, const float R_colmajor[9],
                           const float T[3], int lvl, revo_pair_info* out);
/* Host only, touches no device.  H widened to double; *sigma2 = sum_w / (good - 6) (the weighted residual variance at 6
 * estimated parameters); cov (6x6, symmetric, row == column major) = sigma2 * H^-1 by a double Cholesky factorisation,
 * symmetrised.  sigma2 may be NULL.  REVO_ERR_INVALID_ARG, nothing written: flags bit0, good <= 6, or a pivot that is not
 * positive beyond rounding (pivot <= 64 * 2^-52 * H[j][j]: a rank-deficient system). */
int revo_pair_info_covariance(const revo_pair_info* info, double cov[36], double* sigma2);

/* ---- host-buffer batches: what a producer like IOWrapperRGBD::readNextFrame hands over ------------ */

/* One frame-pair in HOST memory, as the reference's producer thread holds it after cv::imread
 * (iowrapperRGBD.cpp:301-333): BGR8 rows + depth rows (raw uint16 as on disk, or float32 metres after the
 * reference's convertTo), byte strides like cv::Mat::step.  R_init / T_init: initial pose curr -> ref
 * (tracker.cpp:286-288), used when use_init != 0 (else identity). */
typedef struct revo_pair_in {
  const uint8_t* ref_bgr;   size_t ref_bgr_stride;
  const void*    ref_depth; size_t ref_depth_stride;
  const uint8_t* cur_bgr;   size_t cur_bgr_stride;
  const void*    cur_depth; size_t cur_depth_stride;
  float R_init[9], T_init[3];
  int32_t use_init;
} revo_pair_in;
typedef revo_pair_result revo_pair_out;
typedef struct revo_pairs_job revo_pairs_job;

/* n independent frame-pairs from host buffers: upload (H2D on its own stream), both pyramids,
 * keyframe promotion of the reference frame and TrackerNew::trackFrames per pair, results back to the host.
 * depth_is_u16 != 0: the depth rows are raw uint16 and depth = raw * (float)(1 / depth_scale_factor) runs inside
 * the device build (iowrapperRGBD.cpp:326-327).
 *   revo_track_pairs_submit returns once the inputs have been consumed (the caller may reuse its buffers -- the
 *   reference's producer does, iowrapperRGBD.h:163), while the device work of this and earlier jobs continues:
 *   consecutive submits overlap job k+1's PCIe transfer with job k's kernels.  Host memory that is page-locked
 *   (hipHostMalloc / hipHostRegister / torch pin_memory) is read by DMA at PCIe speed; pageable memory works, slower.
 *   revo_track_pairs_wait blocks for the job's results (out: n records) and releases it.  A record with flag bit 3
 *   makes it return REVO_ERR_HIP.  At most 3 jobs may be in flight per context.
 *   revo_track_pairs = submit + wait. */
int revo_track_pairs_submit(revo_ctx* ctx, int n, const revo_pair_in* pairs, int depth_is_u16,
                            double depth_scale_factor, revo_pairs_job** job);
int revo_track_pairs_wait(revo_pairs_job* job, revo_pair_out* out);
int revo_track_pairs(revo_ctx* ctx, int n, const revo_pair_in* pairs, int depth_is_u16,
                     double depth_scale_factor, revo_pair_out* out);

/* ---- the pipelined batch mode as one handle (new in round 5) ------------------------------------------------
 *
 * The reference owns its producer / consumer pipeline: REVO::start drains the queue an IO thread fills
 * (system/system.cpp:96,128-284, io/iowrapperRGBD.cpp:279-288).  The batched mode's counterpart is a rotation of
 * `depth` device-resident batches over FOUR streams the handle owns -- build | edge lists + keyframe EDT | two
 * alternating tracker streams (the resident gate keeps two tracker grids in flight) -- so that step t+3 is built
 * while step t+2 is prepared and steps t+1 and t are tracked.  This is the shape `bench.py` measures; the handle
 * exists so that an integrator gets it without rebuilding the choreography (HIP multiplexes streams onto a few
 * hardware queues, and one stream more, or the same streams created in another order, costs a third of the
 * throughput: DESIGN.md 3.0).  revo_pipeline_create probes its streams (a 150 us kernel on one, a time stamp on
 * another) and replaces those that share a hardware queue; revo_pipeline_info reports the outcome.
 *
 *   submit(t)  enqueues build, deferred work and tracker grid of step t and returns at once: a ticket and the
 *              stream the grid runs on.  Work the caller enqueues on THAT stream before the next submit that uses
 *              the same tracker stream (the next-but-one with two tracker streams, i.e. depth >= 3; the next one
 *              otherwise) runs behind the grid and before the stream's next grid (the result collective, a copy):
 *              the "after the grid" slot.  Do not create a stream of your own for it: a fifth active stream ends up
 *              behind one of the four in a hardware queue.
 *   wait(t)    blocks until step t and its after-grid work are complete; with host_results the n records of the
 *              step are returned from pinned memory (a record with flag bit 3 makes it return REVO_ERR_HIP).
 *
 * d_bgr / d_depth: device-resident inputs of the step, [2*n_pairs][H][W][3] u8 and [2*n_pairs][H][W] depth, frame 2i =
 * reference (keyframe) of pair i, frame 2i+1 = current (revo_batch_track).  depth_kind 0: f32 metres, BORROWED
 * (level 0 of the depth pyramid is the caller's plane: it must stay valid and unchanged for `depth` further
 * submits or until revo_pipeline_wait of the step); 1: f32 metres, copied; 2: raw u16 with depth_scale_factor
 * (iowrapperRGBD.cpp:326-327).  input_ready_event: a hipEvent_t recorded behind whatever produces the inputs, or
 * NULL when they are already complete.  h_init_RT: n_pairs x 12 floats on the host (R column-major, T) or NULL.
 * d_results: n_pairs records in device memory, or NULL for a buffer of the handle's own (host_results).  Results
 * are the same bits as revo_batch_track on one batch: the pipeline only changes when kernels run.
 * One handle is driven by one host thread at a time. */
typedef struct revo_pipeline revo_pipeline;
typedef struct revo_pipeline_info_t {
  int32_t batches;            /* batches in rotation (= depth)                                            */
  int32_t pairs_per_step;
  int32_t tracker_streams;    /* 1 or 2                                                                    */
  int32_t distinct_hw_queues; /* how many of the handle's streams sit on pairwise distinct hardware queues
                                 (4 = none alias; -1 = not probed: REVO_PIPE_PROBE=0)                      */
  int32_t streams_replaced;   /* candidate streams discarded because they aliased one already kept         */
  int32_t probes_run;
  void* streams[4];           /* hipStream_t: tracker 0, tracker 1, build, auxiliary                       */
  uint64_t steps_submitted;
} revo_pipeline_info_t;
/* depth: batches in rotation, 0 = the default (4), 1 = one batch on one stream (nothing overlaps), 2 = build
 * next to one tracker stream.  host_results != 0: every step's records are copied to pinned host memory behind
 * its grid and revo_pipeline_wait returns them; then a slot's step must be waited for before the slot is
 * submitted again (`depth` steps later), else REVO_ERR_CAPACITY. */
int revo_pipeline_create(revo_ctx* ctx, int n_pairs, int depth, int host_results, revo_pipeline** out);
void revo_pipeline_destroy(revo_pipeline* p);
int revo_pipeline_submit(revo_pipeline* p, const uint8_t* d_bgr, const void* d_depth, int depth_kind,
                         double depth_scale_factor, const float* h_init_RT, revo_pair_result* d_results,
                         void* input_ready_event, uint64_t* ticket, void** after_grid_stream);
int revo_pipeline_wait(revo_pipeline* p, uint64_t ticket, revo_pair_result* h_results);
/* Waits for everything submitted so far (all four streams). */
int revo_pipeline_drain(revo_pipeline* p);
int revo_pipeline_info(const revo_pipeline* p, revo_pipeline_info_t* out);
/* The batch that holds step `ticket` (accessors through revo_batch_frame); valid until its slot is submitted again. */
int revo_pipeline_batch(revo_pipeline* p, uint64_t ticket, revo_batch** out);
/* Live timing of the dominant kernel inside the pipelined steps: every every_n-th submit carries a HIP event pair
 * around its tracker grid, on the grid's stream (0 = off; resets the statistics).  revo_pipeline_tracker_ms: mean
 * duration and number of the launches harvested so far (a launch is harvested when its slot is reused, waited
 * for, or drained). */
int revo_pipeline_time_tracker(revo_pipeline* p, int every_n);
int revo_pipeline_tracker_ms(revo_pipeline* p, float* mean_ms, int* launches);

/* ---- Multi-GPU: the result gather behind the C ABI --------------------------------------------
 * The reference is a single-process CPU program (main.cpp:22-47) and has no collective; the batched mode shards
 * independent frame-pairs over the GPUs of a node, ONE PROCESS PER GPU, and its only exchange is an all-gather of
 * the 96-byte pair records over RCCL / xGMI.  A communicator is created like an MPI-style NCCL program does it:
 * rank 0 calls revo_comm_unique_id and ships the 128 bytes to the other ranks by whatever the host has (MPI, a
 * file, a socket, torch.distributed's store); every rank then calls revo_comm_create (ncclCommInitRank on the
 * context's device: a collective).  RCCL is loaded at run time (dlopen: $REVO_RCCL_LIB, a copy the process
 * already carries -- PyTorch bundles one --, librccl.so.1); a box without RCCL still loads the library and only
 * these calls fail (REVO_ERR_HIP, revo_last_error says why). */
typedef struct revo_comm revo_comm;
#define REVO_COMM_ID_BYTES 128
/* REVO_OK iff an RCCL library is loadable; path (optional) = what was loaded, version = ncclGetVersion. */
int revo_comm_available(char* path_out, size_t path_cap, int* version_out);
int revo_comm_unique_id(uint8_t id[REVO_COMM_ID_BYTES]);
int revo_comm_create(revo_ctx* ctx, const uint8_t id[REVO_COMM_ID_BYTES], int world_size, int rank, revo_comm** out);
void revo_comm_destroy(revo_comm* c);
int revo_comm_world(const revo_comm* c, int* world_size, int* rank);
/* ncclAllGather of n_records records per rank, enqueued on `stream` (hipStream_t): d_recv holds
 * world_size * n_records records, rank-major.  Nothing is reduced; the records travel as bytes. */
int revo_comm_allgather_records(revo_comm* c, const revo_pair_result* d_send, revo_pair_result* d_recv,
                                int n_records, void* stream);
/* The pipeline enqueues the collective itself, in the after-grid slot: steps are grouped into windows of `every`
 * (1..8) consecutive steps; the grids of a window write their records into a send buffer of the handle's, and
 * behind the window's LAST grid one all-gather moves them to window slot (k % ring) of d_gathered -- device memory,
 * ring * world_size * every * n_pairs records, laid out [ring][rank][step in window][pair].  revo_pipeline_wait
 * (ticket of the window's last step) covers the collective; a slot is overwritten `ring` (2..16) windows later.
 * With a communicator attached revo_pipeline_submit's d_results may be NULL (non-NULL: the step's own records are
 * copied there as well).  comm = NULL detaches.  Attach / detach drain the pipeline.  Every rank must submit the
 * same number of steps.  revo_pipeline_flush_comm gathers an incomplete last window (*steps_valid of its `every`
 * steps carry records of this run; 0 = the last window was complete and nothing was enqueued) into *slot; it is a
 * collective too (all ranks, same point) and the next submit starts a new window. */
int revo_pipeline_set_comm(revo_pipeline* p, revo_comm* comm, int every, revo_pair_result* d_gathered, int ring);
int revo_pipeline_flush_comm(revo_pipeline* p, int* steps_valid, int* slot);

/* ---- REVO::start sequencing (system/system.cpp:84-305) ----------------------- */

/* The reference runs two threads: IOWrapperRGBD::generateImgPyramid builds pyramids into a
 * queue (iowrapperRGBD.cpp:257-300), REVO::start consumes the oldest one per loop body
 * (system.cpp:128-284).  revo_vo_submit is the producer side (asynchronous: the build of
 * frame N+1 overlaps the tracking of frame N on the device), revo_vo_track_next the consumer:
 * first frame -> keyframe; later frames: trackFrames against the keyframe,
 * assessTrackingQuality, optional promotion of the PREVIOUS frame to keyframe + re-track
 * (system.cpp:203-241), constant-velocity initialisation of the next frame (267-271). */
typedef struct revo_vo revo_vo;
int revo_vo_create(revo_ctx* ctx, revo_vo** out);
void revo_vo_destroy(revo_vo* vo);
int revo_vo_submit(revo_vo* vo, const uint8_t* bgr, size_t bgr_stride,
                   const float* depth_m, size_t depth_stride, double timestamp);
/* Same with raw uint16 depth (iowrapperRGBD.cpp:326-327 fused into the device build). */
int revo_vo_submit_u16(revo_vo* vo, const uint8_t* bgr, size_t bgr_stride,
                       const uint16_t* depth_raw, size_t depth_stride,
                       double depth_scale_factor, double timestamp);
/* pose_colmajor: 4x4 curr->world as REVO::writePose would emit it (system.cpp:275);
 * *new_keyframe: 1 if this frame created a keyframe.  REVO_ERR_INVALID_ARG if the queue is empty. */
int revo_vo_track_next(revo_vo* vo, float pose_colmajor[16], int* new_keyframe,
                       double* timestamp);
int revo_vo_queued(const revo_vo* vo);
/* Two-thread use (the reference's IO thread + consumer loop, system.cpp:96): revo_vo_set_max_queue(n > 0)
 * (re-)opens the stream and makes revo_vo_submit* block while n pyramids wait (n <= 0: never block); the producer ends the stream with revo_vo_close; the
 * consumer calls revo_vo_wait_frame (1: a frame is queued, 0: closed and drained) before revo_vo_track_next. */
int revo_vo_set_max_queue(revo_vo* vo, int max_queue);
int revo_vo_close(revo_vo* vo);
int revo_vo_wait_frame(revo_vo* vo);
int revo_vo_num_keyframes(const revo_vo* vo);
/* The current keyframe (kfPyr) and its pose in the world (getTransKFtoWorld), as REVO::start hands
 * them to the map drawer after a keyframe change (system.cpp:165-167,235-237).  The handle is
 * borrowed: valid until the next revo_vo_track_next / revo_vo_destroy. */
int revo_vo_keyframe(const revo_vo* v, revo_pyr** kf_out, float T_w_kf[16]);

/* Off by default; off, revo_vo_track_next enqueues exactly what it enqueues without this option.  On: every reported frame's
 * level-0 revo_pair_info is taken at its FINAL pose against the keyframe it was reported against (after a keyframe change:
 * the re-track's pose and the new keyframe), enqueued behind that frame's tracker launch, and available from
 * revo_vo_last_pair_info once revo_vo_track_next has returned (*kf_timestamp, may be NULL: that keyframe's time stamp).
 * The first frame of a sequence IS the keyframe: its record has flags bit0 (identity pose).  Poses do not depend on the option.
 * revo_vo_last_pair_info: REVO_ERR_INVALID_ARG while the option is off or before the first frame. */
int revo_vo_set_pair_info(revo_vo* vo, int on);
int revo_vo_last_pair_info(const revo_vo* vo, revo_pair_info* out, double* kf_timestamp);

/* ---------------------------------------------------------------------------
 * Many independent sequential-VO streams in lockstep (revo_vo_multi).
 * Each stream is one REVO::start (system.cpp:84-305) with its own keyframe, past clouds and
 * constant-velocity initialisation; per stream the poses equal what a revo_vo computes.  One
 * revo_vo_multi_step issues ONE tracker grid and ONE quality vote for every stream that has work.
 * A keyframe change is deferred: the step whose vote asks for it promotes the stream's previous
 * frame and reports nothing for that stream; the next step re-tracks the same frame against the
 * new keyframe and reports it with new_keyframe = 1.
 * ------------------------------------------------------------------------- */
typedef struct revo_vo_multi revo_vo_multi;
typedef struct revo_stream_frame {  /* one frame of one stream, host memory (cv::Mat layout) */
  int32_t stream;                   /* 0 .. n_streams-1 */
  const uint8_t* bgr; size_t bgr_stride;
  const void* depth; size_t depth_stride;  /* f32 metres, or raw u16 (depth_is_u16) */
  double timestamp;
} revo_stream_frame;
typedef struct revo_stream_result {
  int32_t stream, new_keyframe;
  double timestamp;
  float pose[16];                   /* curr->world, column-major, as revo_vo_track_next */
} revo_stream_result;
/* n_streams >= 1; max_queue >= 1: frames a stream may hold submitted and not yet reported.  The
 * tracker's cluster size is fixed here from n_streams (REVO_TRACK_CLUSTER / REVO_TRACK_REDUNDANT_BATCH
 * apply as for a batch): a stream's results do not depend on what its neighbours do. */
int revo_vo_multi_create(revo_ctx* ctx, int n_streams, int max_queue, revo_vo_multi** out);
void revo_vo_multi_destroy(revo_vo_multi* m);
/* At most one frame per stream per call; REVO_ERR_CAPACITY if a stream's queue is full.  All n
 * frames are built in one batched build (asynchronous); returns once the host rows are consumed. */
int revo_vo_multi_submit(revo_vo_multi* m, int n, const revo_stream_frame* frames,
                         int depth_is_u16, double depth_scale_factor);
/* One loop body of REVO::start for every stream with work; out: n_streams records, *n_out of them written. */
int revo_vo_multi_step(revo_vo_multi* m, revo_stream_result* out, int* n_out);
int revo_vo_multi_pending(const revo_vo_multi* m, int stream);  /* submitted, not yet reported (-1: bad stream) */
int revo_vo_multi_reset(revo_vo_multi* m, int stream);          /* new sequence on an idle stream (system.cpp:107) */
int revo_vo_multi_num_keyframes(const revo_vo_multi* m, int stream);
/* The stream's current keyframe (borrowed, valid until the next revo_vo_multi_step) and its pose in the world. */
int revo_vo_multi_keyframe(const revo_vo_multi* m, int stream, revo_pyr** kf, float T_w_kf[16]);

/* revo_vo_set_pair_info / revo_vo_last_pair_info per stream: ONE k_pair_info launch per step, on the tracker stream behind the
 * step's grid, covers every stream the step tracks; revo_vo_multi_pair_info returns the record of the stream's last REPORTED
 * frame (per stream the same bytes as a revo_vo's when the poses agree).  Off by default. */
int revo_vo_multi_set_pair_info(revo_vo_multi* m, int on);
int revo_vo_multi_pair_info(const revo_vo_multi* m, int stream, revo_pair_info* out, double* kf_timestamp);

/* Device frames for revo_vo_multi: revo_vo_multi_submit with DEVICE pointers (on the context's device), e.g. the output of
 * revo_png_decode_submit.  The build stream waits for `producer_stream` (an event); the frames are copied device-to-device
 * into the step set (runs of adjacent frames in one copy; the step set owns its copy, a keyframe keeps its colour); then the
 * same batched build runs.  Returns once the copies are done: the caller may reuse its buffers.  Per stream the results are
 * bit-identical to revo_vo_multi_submit on the same pixels.  Argument checks as revo_vo_multi_submit's, plus: every pointer is
 * device memory and the depth rows are aligned to their element size. */
int revo_vo_multi_submit_device(revo_vo_multi* m, int n, const revo_stream_frame* frames, int depth_is_u16,
                                double depth_scale_factor, void* producer_stream);

/* ---------------------------------------------------------------------------
 * World-frame voxel map: what MapDrawer shows (gui/MapDrawer.cc, fed one coloured keyframe cloud + T_w_kf per keyframe from
 * system.cpp:162-168,232-238), fused on the device into one point per voxel.  A keyframe's input points are exactly the
 * level-0 points of revo_pyramid_colored_pcl(kf, 0, dense) with its full-resolution BGR bytes, read from the pyramid's planes
 * (no cloud is formed).  Per point, in float32 with every operation rounded on its own: pw = ((R0*X + R1*Y) + R2*Z) + t, key
 * k = (int)floorf(pw / voxel), fixed point q = llrintf(pw * 2^20).  A point is dropped (and counted) when some |pw| >= 2048 m,
 * some key lies outside [-2^20, 2^20 - 1] or some pw is not finite.  Per voxel: count, sum q (int64 x 3), sum B, G, R (u64),
 * all accumulated with integer atomics: the map depends on its input points and poses only -- not on the order or the
 * batching of integrations, the launch, the stream count or the driver (DESIGN 11 states the contract).
 * Extraction: one point per voxel in ascending order of the key packed as (kx + 2^20) << 42 | (ky + 2^20) << 21 | (kz + 2^20);
 * xyz = (float)((double)sum_q / (double)count * 2^-20), colour = (sum_c + count / 2) / count.  The float64 mean is exact
 * while count <= 2^22 points per voxel.
 * All work of a map runs on its context's tracker stream.  One handle must not be used concurrently.
 * ------------------------------------------------------------------------- */
typedef struct revo_map revo_map;
/* voxel: edge in metres (finite, > 0); dense: the cloud mode of generateColoredPcl's densePcl (imgpyramidrgbd.cpp:279-327);
 * initial_voxels: starting capacity (the table grows by rehashing on the device, no point is lost); max_voxels (1 .. 2^28): hard
 * bound on the voxels of the map. */
int revo_map_create(revo_ctx* ctx, float voxel, int dense, size_t initial_voxels, size_t max_voxels, revo_map** out);
/* Waits for the map's work.  A map still attached to revo_vo_multi streams is detached from them first. */
void revo_map_destroy(revo_map* m);
/* MapDrawer::addPclAndKfPoseToQueue(kfPyr->generateColoredPcl(0, dense), T_w_kf) (system.cpp:165-167,235-237), fused into
 * the map.  Asynchronous: enqueued on the context's tracker stream behind the keyframe's build; the pyramid may be destroyed
 * right after the call.  kf: a pyramid of revo_pyramid_create* / revo_vo_keyframe / revo_vo_multi_keyframe of the map's
 * context (batch views keep no colour: REVO_ERR_INVALID_ARG).  T_w_kf: finite, column-major.
 * REVO_ERR_CAPACITY: the keyframe would take the map past max_voxels.  The integration is then all or nothing: none of its
 * points is in the map, the counters are unchanged except keyframes_rejected, and the map stays usable.  (Only when the map
 * could reach max_voxels does the call wait for the device to decide; otherwise it returns at once.) */
int revo_map_integrate(revo_map* m, const revo_pyr* kf, const float T_w_kf_colmajor[16]);
/* n keyframes in one launch; the result is the same as n revo_map_integrate calls in any order.  All or nothing as a whole. */
int revo_map_integrate_many(revo_map* m, int n, const revo_pyr* const* kfs, const float* T_w_kf_colmajor_n16);
/* Empties the map (capacity and settings stay). */
int revo_map_clear(revo_map* m);
typedef struct revo_map_info_t {
  size_t voxels;              /* occupied voxels                                                    */
  size_t points_integrated;   /* input points accumulated                                           */
  size_t points_dropped;      /* input points outside the range above                               */
  size_t capacity;            /* hash-table slots (a power of two; load factor <= 0.5)              */
  int32_t keyframes;          /* integrations that took effect                                      */
  int32_t keyframes_rejected; /* integrations refused for max_voxels (revo_vo_multi attachments too) */
  int32_t rehashes;           /* table growths                                                      */
} revo_map_info_t;
/* Waits for the map. */
int revo_map_info(revo_map* m, revo_map_info_t* out);
/* Waits for the map, then writes the voxels with count >= max(min_count, 1) in key order: xyz (3 floats), rgb (3 bytes R,G,B),
 * count (1 u32) per voxel, at most cap of them; *n = how many there are.  xyz == NULL only counts (rgb, count may be NULL).
 * REVO_ERR_CAPACITY (nothing written) if cap < *n. */
int revo_map_extract(revo_map* m, size_t min_count, float* xyz, uint8_t* rgb, uint32_t* count, size_t cap, size_t* n);
/* Every keyframe the stream promotes from now on is integrated into m, in the step's one batched launch on the tracker stream,
 * right behind the promotion (the first frame of a sequence included).  m == NULL detaches.  m must belong to the handle's
 * context.  revo_vo_multi_reset detaches the stream's map; a step never fails for a map: a refused integration (max_voxels)
 * is counted in its keyframes_rejected. */
int revo_vo_multi_attach_map(revo_vo_multi* mv, int stream, revo_map* m);

/* Views of the map: what the reference's viewer shows from the camera's pose (MapDrawer + SetCurrentCameraPose), as a depth
 * image and a BGR image per view, splatted through a z-buffer on the device with integer atomics only.
 * All arithmetic is float32 with every operation rounded on its own.  Per view, on the host: Rc = R^T of T_w_c,
 * tc_i = -(((Rc_i0*tx) + (Rc_i1*ty)) + (Rc_i2*tz)).  Per voxel with count >= max(min_count, 1): p and colour exactly as
 * revo_map_extract returns them; pc = ((Rc[:,0]*px + Rc[:,1]*py) + Rc[:,2]*pz) + tc.  Skipped unless pc is finite and
 * z > zmin, z < zmax (imgpyramidrgbd.h:170-173).  Centre pixel (tracker.cpp:153-156): u = (fx*x)/z + cx, v = (fy*y)/z + cy,
 * iu = (int)floorf(u), iv = (int)floorf(v); skipped if u or v is not finite or |u| or |v| >= 2^20.  Footprint:
 * ru = min(splat_max, (int)ceilf(((0.5f*voxel)*fx)/z)), rv likewise with fy; the voxel writes every pixel of
 * [iu-ru, iu+ru] x [iv-rv, iv+rv] inside the image.  It writes the 64-bit word (bits of z) << 32 | R << 16 | G << 8 | B and a
 * pixel keeps the MINIMUM word written to it (z > 0: float bits order like the floats; equal z: the smaller colour word) --
 * a minimum does not depend on order, so a view is the same bytes whatever the table size, integration order or launch.
 * Outputs: depth (h x w floats, 0 where nothing was written), bgr (h x w x 3 bytes, 0 there), covered = written pixels. */
typedef struct revo_map_view {
  int32_t width, height;            /* 1 .. 2048 each                                                              */
  float fx, fy, cx, cy, zmin, zmax; /* all six zero: the context's level-0 camera and DEPTH_MIN / DEPTH_MAX;       */
                                    /* else finite, fx > 0, fy > 0, 0 <= zmin < zmax                                 */
  float T_w_c[16];                  /* camera -> world, column-major, finite                                       */
  int32_t splat_max;                /* 0 .. 8: bound of the footprint's half width in pixels (0: one pixel/voxel)   */
  uint32_t min_count;               /* as revo_map_extract's                                                       */
} revo_map_view;
/* n views (sizes may differ) of the map as it is behind every integration enqueued so far, in one splat launch and one resolve
 * launch on the context's tracker stream.  depth[i], bgr[i]: the outputs of view i, rows packed; covered: n entries or NULL.
 * device_out = 0: host pointers, the call waits.  device_out = 1: device pointers (depth[i], bgr[i] and covered 16-byte
 * aligned), the call only enqueues.  An empty map renders empty views.  The map is not changed.
 * REVO_ERR_INVALID_ARG: n < 1, a NULL array or output, a size outside 1 .. 2048, a pose, intrinsic or range that is not finite,
 * fx or fy <= 0, zmin < 0 or zmin >= zmax, splat_max outside 0 .. 8, a misaligned device output. */
int revo_map_render(revo_map* m, int n, const revo_map_view* views, float* const* depth, uint8_t* const* bgr, uint32_t* covered,
                    int device_out);
/* Waits for the last revo_map_render of m and gives the device time between the start of its splat and the end of its resolve
 * (HIP events on the tracker stream), in milliseconds.  REVO_ERR_INVALID_ARG if m has rendered nothing yet. */
int revo_map_render_last_ms(revo_map* m, float* ms);

/* The map as data.  A voxel is nothing but integer sums, so they can leave the handle and come back without loss:
 * the union of two maps is the slot-wise integer sum -- exact, commutative, associative -- and a map merged from parts is byte
 * for byte the map one handle would have built from all their keyframes. */
typedef struct revo_map_voxel_raw {   /* 64 bytes, little-endian, no padding */
  uint64_t key;        /* (kx + 2^20) << 42 | (ky + 2^20) << 21 | (kz + 2^20), bit 63 clear */
  uint64_t count;      /* >= 1 */
  int64_t  sum_q[3];   /* x, y, z in 2^-20 m */
  uint64_t sum_bgr[3]; /* B, G, R */
} revo_map_voxel_raw;
/* Waits for the map, sets *n to its voxels and writes one record per voxel, at most cap of them.  dst == NULL only counts.
 * REVO_ERR_CAPACITY (nothing written) if cap < *n.  device_out = 0: host memory, ascending key order -- the canonical form:
 * equal maps give equal bytes.  device_out = 1: device memory of the map's device, 16-byte aligned, in unspecified order. */
int revo_map_export_raw(revo_map* m, revo_map_voxel_raw* dst, size_t cap, size_t* n, int device_out);
/* Adds n records into m (device_in = 0: host memory; 1: device memory, 16-byte aligned).  A key may occur several times: the
 * exports of several maps go in one call, concatenated.  On success points_integrated += sum of count, points_dropped +=
 * points_dropped, keyframes += keyframes and voxels is the true count.  All or nothing: REVO_ERR_CAPACITY if the result
 * would pass max_voxels, REVO_ERR_INVALID_ARG if some record has count == 0 or key bit 63 set; a merge refused for either
 * changes no voxel and no counter except keyframes_rejected += keyframes, and the map stays usable (the table may have
 * grown).  Other argument errors (NULL, a misaligned device pointer, keyframes < 0) change nothing at all.  Enqueued on the
 * context's tracker stream behind pending integrations; the call waits for the device when the device has to decide (device
 * input, or a map that could reach max_voxels) and for host input.  n == 0 is a no-op. */
int revo_map_merge_raw(revo_map* m, const revo_map_voxel_raw* src, size_t n, int device_in, size_t points_dropped,
                       int32_t keyframes);
/* revo_map_merge_raw straight from src's table on the device, with src's points_dropped and keyframes.  Waits for src; src is
 * not changed.  REVO_ERR_INVALID_ARG: NULL, dst == src, voxel edges whose float bits differ, maps on different devices.
 * dense may differ. */
int revo_map_merge(revo_map* dst, revo_map* src);
/* The exact inverse of revo_map_merge_raw: per record the voxel of `key` loses count, sum_q and sum_bgr; a key may
 * occur several times.  A voxel whose count reaches 0 is gone: absent from every export, extraction, view and merge, and no
 * longer counted against max_voxels.  On success points_integrated -= sum of count, points_dropped -= points_dropped,
 * keyframes -= keyframes and voxels is the true count; merging the same records again restores the map byte for byte.
 * All or nothing: REVO_ERR_INVALID_ARG if some record has count == 0 or key bit 63 set, some key is not in the map, the
 * records of a voxel together take more than its count, a voxel would keep count 0 with a non-zero sum, or points_dropped or
 * keyframes is larger than the map's own; the map is then as it was, bit for bit, keyframes_rejected included.  Other
 * argument errors (NULL, a misaligned device pointer, keyframes < 0) change nothing either.  n == 0 is a no-op.
 * What the call cannot see is the caller's responsibility: records that leave every voxel they touch a positive count but
 * were never part of this map are subtracted, and the map is then not one that any set of keyframes builds.
 * Enqueued on the context's tracker stream behind pending integrations; the call always waits for the device's decision.
 * The table keeps its capacity (no occupied slot is left with count 0; rehashes does not count the clean-up). */
int revo_map_subtract_raw(revo_map* m, const revo_map_voxel_raw* src, size_t n, int device_in, size_t points_dropped,
                          int32_t keyframes);
/* revo_map_subtract_raw straight from src's table on the device, with src's points_dropped and keyframes: the inverse of
 * revo_map_merge(dst, src).  Waits for src; src is not changed.  REVO_ERR_INVALID_ARG as above, and for NULL, dst == src,
 * voxel edges whose float bits differ, maps on different devices. */
int revo_map_subtract(revo_map* dst, revo_map* src);
/* The voxel edge and cloud mode the map was created with (either output may be NULL). */
int revo_map_voxel_size(revo_map* m, float* voxel, int* dense);

/* ---- registration of voxel maps -----------------------------------------------------------------------
 * Every map operation above assumes the maps share one world frame.  These calls say how two maps lie relative to each
 * other: point-to-point ICP between the voxels' mean points, with the nearest destination voxel found in the 27 voxels
 * around the transformed source point.  A record of sums is, like every record of this library, a pure function of the
 * two maps and the pose: the same bytes whatever the table sizes, the integration order, the grid shape or the stream.
 *
 * revo_map_coarsen: every voxel of src is added into dst under the key whose axis indices are src's shifted right by
 * `shift` (1 .. 20) arithmetically -- floor(k / 2^shift) on the unbiased index, repacked with the 2^20 bias; count, sum_q
 * and sum_bgr are carried unchanged.  dst's voxel edge must be, bit for bit, src's times 2^shift.  All or nothing on
 * max_voxels and counters exactly as revo_map_merge (points_dropped and keyframes come from src); waits for src; src is
 * not changed.  REVO_ERR_INVALID_ARG: NULL, dst == src, shift outside 1 .. 20, another edge ratio, different devices.
 * Contract: the result is byte for byte (revo_map_export_raw) the map a handle with the coarse edge builds from the same
 * keyframes, provided no input point was dropped for key range -- with |pw| < 2048 m that is guaranteed for
 * voxel >= 2^-9 m.  (fdiv_rn(pw, 2^s v) = 2^-s fdiv_rn(pw, v) exactly in the normal range, floor(floor(y) / 2^s) =
 * floor(y / 2^s), and q and the colours do not depend on the edge.) */
int revo_map_coarsen(revo_map* dst, revo_map* src, int shift);

typedef struct revo_map_align_params {
  float    max_dist;       /* finite, 0 < max_dist <= dst's voxel edge: a match farther than this is rejected        */
  uint32_t min_count_dst;  /* as revo_map_extract's min_count, for the destination voxels                            */
  uint32_t min_count_src;  /* ... and for the source voxels                                                          */
  float    centre[3];      /* finite: the point (destination frame) the rotation increment turns about               */
} revo_map_align_params;

/* Per source voxel with count >= max(min_count_src, 1), in float32 with every operation rounded on its own:
 *   p   the voxel's point exactly as revo_map_extract returns it;
 *   p'  = ((R[:,0]*px + R[:,1]*py) + R[:,2]*pz) + t;
 *   k_i = floorf(p'_i / voxel_dst); the voxel is SKIPPED (and counted) if p' is not finite, some |p'_i| >= 2048 or
 *         some k_i lies outside [-2^20, 2^20 - 1];
 *   candidates: the up to 27 destination voxels with indices k + {-1,0,1}^3 that lie in range, are present and have
 *         count >= max(min_count_dst, 1); for each, q as revo_map_extract gives it, d = p' - q per axis,
 *         d2 = (dx*dx + dy*dy) + dz*dz;
 *   the match is the candidate with the smallest (d2, packed key) pair, accepted iff d2 <= max_dist*max_dist (one float
 *         product, formed on the host).
 * Per accepted match, with u = p' - centre and r = p' - q, these float terms are summed:
 *   S[0..2]   u_x, u_y, u_z
 *   S[3..8]   u_x*u_x, u_x*u_y, u_x*u_z, u_y*u_y, u_y*u_z, u_z*u_z
 *   S[9..11]  r_x, r_y, r_z
 *   S[12..14] u x r, two terms per point and axis: u_y*r_z and -(u_z*r_y); u_z*r_x and -(u_x*r_z); u_x*r_y and -(u_y*r_x)
 *   S[15]     r_x*r_x, r_y*r_y, r_z*r_z (three terms)
 * Each S is the float nearest the exact sum of its float terms (carried as a double-double from the first addition on
 * and rounded once; DESIGN 4.1's midpoint caveat applies).  The counts are exact. */
typedef struct revo_map_align_info {   /* 160 bytes, little-endian, no padding holes */
  float    S[16];
  uint64_t matched;      /* accepted matches                                                                          */
  uint64_t considered;   /* source voxels with count >= max(min_count_src, 1)                                         */
  uint64_t skipped;      /* of those, the ones whose p' left the key range                                            */
  float    centre[3], max_dist;  /* copied from the parameters                                                        */
  float    R[9], T[3];   /* the pose the sums were taken at (source -> destination, R column-major), as given         */
  int32_t  flags;        /* bit0: no evaluation (pose not finite or not orthogonal): everything else in the record is
                            then zero except the pose, centre and max_dist                                            */
  int32_t  reserved;     /* zero */
} revo_map_align_info;

/* One record per pose (n >= 1 poses, 4x4 column-major, source -> destination frame).  The call caches the source's points
 * and the destination's means (two small launches), evaluates all n poses in ONE launch on dst's context's tracker stream
 * -- behind the pending integrations of both maps; it waits for src as revo_map_merge does -- and waits for the result.
 * out: n records, host memory (device_out = 0) or device memory of the maps' device, 16-byte aligned (device_out = 1).
 * Neither map is changed; dst == src is allowed; the voxel edges may differ.  An empty source or destination gives
 * matched = 0 and zero sums.  REVO_ERR_INVALID_ARG: NULL, n < 1, max_dist outside its range, a centre that is not finite,
 * maps on different devices, a misaligned device output. */
int revo_map_align_eval(revo_map* dst, revo_map* src, int n, const float* T_dst_src_n16, const revo_map_align_params* prm,
                        revo_map_align_info* out, int device_out);

/* Host only.  The record's sums widened into the Gauss-Newton system of point-to-point ICP for the increment
 * x = (v, w) applied on the left about centre, p'(x) = centre + exp(w)(p' - centre) + v; with n = matched:
 *   H = [[n I, -[Su]x], [[Su]x, S(|u|^2 I - u u^T)]]  (6x6, row == column major),  g = [Sr ; S u x r];  cost = S[15].
 * The step is the solution of H x = -g.  REVO_ERR_INVALID_ARG: NULL, or a record with flags bit0. */
int revo_map_align_system(const revo_map_align_info* info, double H[36], double g[6]);

typedef struct revo_map_align_opts {
  int32_t  max_iters;    /* >= 1                                                                                      */
  int32_t  reserved;     /* zero                                                                                      */
  double   eps_t, eps_r; /* converged when max|v| < eps_t (m) and max|w| < eps_r (rad)                                */
  uint64_t min_matched;  /* fewer accepted matches than this: lost                                                    */
} revo_map_align_opts;
enum { REVO_ALIGN_CONVERGED = 0, REVO_ALIGN_ITER_LIMIT = 1, REVO_ALIGN_LOST = 2 };

/* Gauss-Newton in double on the host over revo_map_align_eval's records (the caches are built once per call): evaluate at
 * the current pose rounded to float; solve H x = -g with the Cholesky and pivot rule of revo_pair_info_covariance; update
 * T <- Tr(c) exp(x) Tr(-c) T (exp: the SE(3) exponential, x = (v, w)); stop when the step is below eps_t / eps_r
 * (converged) or after max_iters evaluations (iteration limit).  Lost: matched < min_matched or a rank-deficient H; T_out
 * is then the last pose that had a system (T_init if none had).  info_out is the record at T_out, from one more
 * evaluation, so (T_out, info_out) satisfies the eval contract on its own.  *iterations = systems evaluated.
 * opt == NULL: 30 iterations, 1e-6 m, 1e-6 rad, 12 matches.  info_out, iterations may be NULL.
 * REVO_ERR_INVALID_ARG: as revo_map_align_eval, a T_init that is not finite, max_iters < 1. */
int revo_map_align(revo_map* dst, revo_map* src, const float T_init[16], const revo_map_align_params* prm,
                   const revo_map_align_opts* opt, float T_out[16], revo_map_align_info* info_out, int32_t* iterations,
                   int32_t* status);

/* ---- point-to-plane registration: per-voxel normals ---------------------------------------------------
 * Point-to-point ICP penalises sliding along a surface, so on dense maps every step is short.  The point-to-plane metric
 * needs a surface normal per destination voxel; a normal is, like a voxel's point, a pure function of the map.
 *
 * revo_map_normals: the voxels of revo_map_extract(m, min_count, ...) in the same (ascending key) order, each with its
 * point xyz[3], normal[3], lambda[3] (l0 <= l1 <= l2) and neighbours.  Every output pointer except n may be NULL; with all
 * four NULL only *n is written (cap is then ignored), otherwise cap < *n is REVO_ERR_CAPACITY.  All arithmetic is float32
 * with every operation rounded on its own.  For a voxel with index k, count >= max(min_count, 1) and point m0:
 *   neighbours: the voxels at k + {-1,0,1}^3 (the voxel itself included) that are in key range, present and have
 *         count >= max(min_count, 1), visited with the x offset outermost and the z offset innermost, each -1, 0, 1;
 *         m_j is the neighbour's point exactly as revo_map_extract gives it; nb is their number;
 *   with d = m_j - m0, added sequentially in that order from +0: S1 += d (3 sums), S2 += d d^T (6 sums: xx, xy, xz, yy,
 *         yz, zz, one product each);
 *   C_ij = S2_ij - (S1_i * S1_j) / (float)nb   (one product, one division, one subtraction; 6 entries, C symmetric);
 *   eigen-decomposition: A = C, V = I, then 6 cyclic Jacobi sweeps over (p,q) = (0,1), (0,2), (1,2).  A rotation is skipped
 *         when a_pq == 0; otherwise, with r the third index,
 *           theta = (a_qq - a_pp) / (2 * a_pq);  t = copysign(1, theta) / (|theta| + sqrt(theta*theta + 1));
 *           c = 1 / sqrt(t*t + 1);  s = t*c;  h = t * a_pq;  a_pp = a_pp - h;  a_qq = a_qq + h;  a_pq = 0;
 *           (a_rp, a_rq) <- (c*a_rp - s*a_rq, s*a_rp + c*a_rq);
 *           (V_ip, V_iq) <- (c*V_ip - s*V_iq, s*V_ip + c*V_iq) for the rows i = 0, 1, 2;
 *   l0 <= l1 <= l2: a_00, a_11, a_22 after the sweeps, sorted with ties to the lower index; the normal is the column of V
 *         that belongs to l0, each component divided by norm = sqrt((x*x + y*y) + z*z); then negated if its component of
 *         largest magnitude (lowest index at ties) is negative;
 *   valid iff nb >= min_neighbours, the three components are finite, l1 > 0, l0 <= planarity * l1 and
 *         l1 >= min_spread * l2 (one product each); an invalid normal is reported as (0, 0, 0).  lambda and neighbours are
 *         reported either way.
 * The map is not written; an empty map gives *n = 0.  REVO_ERR_INVALID_ARG: NULL map or n, min_neighbours < 3, a
 * planarity outside (0, 1) or a min_spread outside [0, 1) (or not finite). */
typedef struct revo_map_normals_params {
  uint32_t min_count;       /* as revo_map_extract's: voxels below it neither get a normal nor count as neighbours */
  uint32_t min_neighbours;  /* >= 3; neighbours include the voxel itself                                            */
  float    planarity;       /* finite, 0 < planarity < 1: valid only if l0 <= planarity * l1                        */
  float    min_spread;      /* finite, 0 <= min_spread < 1: valid only if l1 > 0 and l1 >= min_spread * l2          */
} revo_map_normals_params;   /* NULL: 1, 5, 0.1f, 0.1f */
int revo_map_normals(revo_map* m, const revo_map_normals_params* prm, float* xyz, float* normal, float* lambda,
                     uint32_t* neighbours, size_t cap, size_t* n);

/* The point-to-plane record of one pose.  Everything up to the match is revo_map_align_eval's contract, word for word
 * (p, p', skipping, the 27 candidates, d2, the (d2, packed key) minimum, the inclusive gate), with one change: a
 * destination voxel is a candidate only if it also has a valid normal under nprm, whose min_count must equal
 * max(prm->min_count_dst, 1).  Per accepted match, with u = p' - centre, r = p' - q, (nx, ny, nz) the matched voxel's
 * normal, float32 with every operation rounded on its own:
 *   e  = (nx*rx + ny*ry) + nz*rz;
 *   a  = u x n:  ax = uy*nz - uz*ny,  ay = uz*nx - ux*nz,  az = ux*ny - uy*nx  (two products and one subtraction each);
 *   J  = (nx, ny, nz, ax, ay, az);
 *   S[0..20]  J_i*J_j for i <= j, row by row (00 01 .. 05 11 .. 55);  S[21..26]  J_i*e;  S[27]  e*e  (one product each).
 * Each S is the float nearest the exact sum of its float terms (double-double from the first addition, rounded once;
 * DESIGN 4.1's midpoint caveat applies).  The counts are exact. */
typedef struct revo_map_plane_info {   /* 208 bytes, little-endian, no padding holes */
  float    S[28];
  uint64_t matched, considered, skipped;  /* as revo_map_align_info's                                                 */
  float    centre[3], max_dist;
  float    R[9], T[3];
  int32_t  flags;        /* bit0 as revo_map_align_info's: everything else is then zero except pose, centre, max_dist */
  int32_t  dst_normals;  /* destination voxels with a valid normal, exact (saturating at INT32_MAX)                   */
} revo_map_plane_info;

/* revo_map_align_eval for the point-to-plane metric: the same arguments, caches, launch shape, streams and waits, plus
 * the destination's normal table (nprm == NULL: the defaults with min_count = max(prm->min_count_dst, 1)), built once per
 * call.  A destination without any valid normal gives matched = 0, zero sums and dst_normals = 0.
 * REVO_ERR_INVALID_ARG: as revo_map_align_eval and revo_map_normals, and nprm->min_count != max(prm->min_count_dst, 1). */
int revo_map_align_plane_eval(revo_map* dst, revo_map* src, int n, const float* T_dst_src_n16,
                              const revo_map_align_params* prm, const revo_map_normals_params* nprm,
                              revo_map_plane_info* out, int device_out);

/* Host only.  For the increment x = (v, w) applied on the left about centre (revo_map_align_system's convention),
 * e(x) ~ e + n.v + w.(u x n) = e + J.x:  H = sum J J^T, the symmetric 6x6 matrix whose upper triangle is S[0..20];
 * g = sum J e = S[21..26];  cost = S[27].  The step solves H x = -g.  REVO_ERR_INVALID_ARG: NULL, or flags bit0. */
int revo_map_align_plane_system(const revo_map_plane_info* info, double H[36], double g[6]);

/* revo_map_align's Gauss-Newton loop over revo_map_align_plane_eval's records: the same options, Cholesky and pivot rule,
 * update T <- Tr(c) exp(x) Tr(-c) T, stopping rule and statuses.  A single plane leaves H rank-deficient: lost. */
int revo_map_align_plane(revo_map* dst, revo_map* src, const float T_init[16], const revo_map_align_params* prm,
                         const revo_map_normals_params* nprm, const revo_map_align_opts* opt, float T_out[16],
                         revo_map_plane_info* info_out, int32_t* iterations, int32_t* status);

/* ---- maps under a pose: posed merge and subtract ------------------------------------------------------
 * Registration ends with a pose T (source -> destination).  These calls put a source map into the destination's frame.
 * A voxel is integer sums, its point a pure function of them, and a float32 rigid transform with every operation rounded on
 * its own a pure function of the point and the pose: "the source map seen under T" is a well-defined set of raw records,
 * the same bytes whatever the table size, integration order, launch shape or stream.
 *
 * The posed record of a source voxel (key, n, sum_q, sum_bgr) under T (column-major, float32) at the destination edge
 * voxel_dst, float32 with every operation rounded on its own:
 *   p    the voxel's point exactly as revo_map_extract returns it: (float)((double)sum_q / (double)n * 2^-20);
 *   p'_i = ((R_i0*px + R_i1*py) + R_i2*pz) + t_i   (revo_map_align_eval's p');
 *   k_i  = floorf(p'_i / voxel_dst)   (one correctly rounded division);
 *   the voxel is DROPPED when some p'_i is not finite, some |p'_i| >= 2048 or some k_i lies outside [-2^20, 2^20 - 1]
 *        (revo_map_integrate's test);
 *   otherwise q_i = (int64)rintf(p'_i * 2^20), and the posed record is: the key packed from k, count = n,
 *        sum_q = n * q (an exact int64 product: |q| <= 2^31, n < 2^32), sum_bgr carried unchanged --
 *        n points at the moved mean, with the voxel's own colour sums.
 * Voxels with n < max(min_count, 1) are SKIPPED: neither moved nor dropped.  A source voxel with n >= 2^32 is a bad record
 * (REVO_ERR_INVALID_ARG, nothing changed), as count 0 and key bit 63 are for revo_map_merge_raw.
 * Counts and colour sums are conserved exactly; only positions are resampled. */
typedef struct revo_map_pose_info {   /* 64 bytes, little-endian, no padding */
  uint64_t voxels_in;       /* voxels of the source: moved + dropped + skipped */
  uint64_t voxels_moved;    /* posed records made (before equal keys are summed) */
  uint64_t voxels_dropped;
  uint64_t voxels_skipped;
  uint64_t points_moved;    /* the sums of count over the moved, dropped and skipped voxels */
  uint64_t points_dropped;
  uint64_t points_skipped;
  uint64_t reserved;        /* zero */
} revo_map_pose_info;

/* The posed records of src; src is not changed.  Waits for src, runs on its context's tracker stream.
 * device_out = 1: one record per moved voxel in unspecified order, keys may repeat (revo_map_merge_raw accepts that), into
 *   device memory of src's device, 16-byte aligned; *n = voxels_moved.  A counting launch runs first, so that a refused call
 *   writes nothing; the call then waits for the counters only: the records
 *   are complete once the stream has run (any waiting call of the map, or work enqueued behind it on that stream).
 * device_out = 0: the canonical form in host memory -- ascending keys, equal keys summed; *n = the keys.  Byte for byte what
 *   revo_map_export_raw gives for an empty map of edge voxel_dst (max_voxels out of reach) after revo_map_merge_posed.
 * out == NULL only counts (cap is ignored); cap < *n is REVO_ERR_CAPACITY with nothing written.  info may be NULL.
 * REVO_ERR_INVALID_ARG, nothing written: NULL src, T or n; device_out not 0 or 1; a misaligned device output; voxel_dst not
 * finite or not > 0; a T that is not finite (all 16 numbers); a rotation that fails the is_orthogonal rule of
 * revo_map_align_eval (|R R^T - I|_F < 1e-5 and det > 0, float32); a source voxel with n >= 2^32. */
int revo_map_pose_raw(revo_map* src, const float T_dst_src[16], float voxel_dst, size_t min_count, revo_map_voxel_raw* out,
                      size_t cap, size_t* n, int device_out, revo_map_pose_info* info);
/* By definition revo_map_merge_raw(dst, the device posed records of src at dst's voxel edge, voxels_moved, 1,
 * src's points_dropped + info.points_dropped, src's keyframes): all or nothing on max_voxels exactly as there
 * (REVO_ERR_CAPACITY, no voxel changed, keyframes_rejected += src's keyframes), and a no-op when no voxel moves.  The two
 * edges and dense may differ.  The pose is checked before any table is touched.  Runs on dst's context's tracker stream
 * behind both maps' pending work (it waits for src as revo_map_merge does) and waits for the device; the record buffer
 * (64 bytes per source voxel) is freed once the stream has consumed it.  info may be NULL; it is filled whenever the posed
 * records were made, also when the merge is then refused.
 * REVO_ERR_INVALID_ARG, nothing changed: as revo_map_pose_raw's pose rules, NULL dst or src, dst == src, maps on different
 * devices, a source voxel with n >= 2^32, a source keyframe count past INT32_MAX. */
int revo_map_merge_posed(revo_map* dst, revo_map* src, const float T_dst_src[16], size_t min_count, revo_map_pose_info* info);
/* The exact inverse: revo_map_subtract_raw over the same records and counters.  After revo_map_merge_posed followed by
 * revo_map_subtract_posed with the same src, T and min_count dst is byte for byte what it was, counters included.  Every
 * refusal rule of revo_map_subtract_raw applies, and dst is then untouched. */
int revo_map_subtract_posed(revo_map* dst, revo_map* src, const float T_dst_src[16], size_t min_count, revo_map_pose_info* info);

/* ---- free-space carving: voxels a later view looks through leave the map --------------------------------
 * Whether a view sees through a voxel depends on that voxel's sums, the view's depth image and its pose only, so a carve is
 * a pure function of its inputs: the same bytes whatever the table size, integration order, launch shape or stream.
 * All arithmetic is float32 with every operation rounded on its own.
 *
 * Per view, on the host: Rc and tc exactly as revo_map_render forms them from T_w_c; intrinsics fx, fy, cx, cy; the depth
 * range zmin, zmax; the depth image D, h x w float32 metres, rows packed.
 * Candidates: the voxels with count >= max(min_count, 1), and count <= max_count when max_count != 0; p exactly as
 * revo_map_extract returns it.  Per view a candidate falls into exactly one of six classes:
 *   OUTSIDE    pc = ((Rc[:,0]*px + Rc[:,1]*py) + Rc[:,2]*pz) + tc is not finite, or z <= zmin, or z >= zmax, or
 *              u = (fx*x)/z + cx, v = (fy*y)/z + cy is not finite or |u| or |v| >= 2^20, or, with iu = (int)floorf(u + 0.5f)
 *              and iv likewise (the nearest pixel: back-projection puts pixel x at u = x), the window
 *              [iu-r, iu+r] x [iv-r, iv+r] (r = radius) is not wholly inside the image;
 *   UNKNOWN    some pixel of the window is not a usable depth (usable: finite, > zmin, < zmax);
 *   FREE       z < dmin - (margin + margin_rel*dmin), dmin the minimum of the window's depths (a product, a sum and a
 *              difference, each rounded);
 *   otherwise, with dc = D[iv, iu] and mc = margin + margin_rel*dc:
 *   CONFIRMED  fabsf(z - dc) <= mc;
 *   OCCLUDED   z > dc + mc;
 *   EDGE       the rest: in front of the centre pixel, but a neighbour of the window is nearer.
 * A voxel's votes are the views in which it is FREE; it is carved iff votes >= max(min_views, 1).  The class of a voxel
 * does not look at any other voxel, so: a second identical carve removes nothing; the order of the views cannot show; with
 * min_views = 1, carving with views A and then with views B equals one carve with A and B together.
 * A carved voxel leaves with its whole record (key, count, sum_q, sum_bgr) through revo_map_subtract_raw's exact
 * subtraction: points_integrated falls by its count, keyframes and points_dropped do not move, voxels is the true count and
 * no occupied slot keeps count 0. */
typedef struct revo_map_carve_view {   /* 112 bytes */
  const revo_pyr* kf;               /* a pyramid of the map's context: its level-0 depth plane, the context's level-0 camera   */
                                    /* and DEPTH_MIN / DEPTH_MAX (depth must be NULL; the other image fields are ignored) ...   */
  const float* depth;               /* ... or a raw depth image, rows packed (kf must be NULL)                                 */
  int32_t width, height;            /* 1 .. 2048 each                                                                          */
  float fx, fy, cx, cy, zmin, zmax; /* all six zero: the context's, as in revo_map_view; else finite, fx, fy > 0,              */
                                    /* 0 <= zmin < zmax                                                                        */
  float T_w_c[16];                  /* camera -> world, column-major, finite, rotation orthogonal (revo_map_align_eval's rule) */
} revo_map_carve_view;
typedef struct revo_map_carve_params { /* 24 bytes; NULL: 1, 1, 1, 0, the map's voxel edge, 0 */
  int32_t radius;        /* 0 .. 3: half width of the pixel window                                   */
  uint32_t min_views;    /* votes a voxel needs (0 counts as 1)                                      */
  uint32_t min_count;    /* as revo_map_extract's                                                    */
  uint32_t max_count;    /* 0: no upper bound                                                        */
  float margin;          /* metres, finite, >= 0                                                     */
  float margin_rel;      /* per metre of depth, finite, >= 0                                         */
} revo_map_carve_params;
typedef struct revo_map_carve_info {   /* 64 bytes, little-endian, no padding */
  uint64_t voxels_considered;  /* the candidates                                   */
  uint64_t voxels_carved;
  uint64_t points_carved;      /* the sum of count over the carved voxels          */
  uint64_t votes;              /* FREE classifications over all candidates, views  */
  uint64_t reserved[4];        /* zero */
} revo_map_carve_info;
typedef struct revo_map_carve_view_info { /* 32 bytes per view: the candidates by class; they sum to voxels_considered */
  uint32_t outside, unknown, free_space, confirmed, occluded, edge;
  uint32_t reserved[2];        /* zero */
} revo_map_carve_view_info;
/* The records that revo_map_carve would remove; the map is untouched.  n: 1 .. 64 views.  device_in: where the raw depth
 * images live (0: host memory -- uploaded to a temporary buffer that is freed after the stream has consumed it; 1: device
 * memory of the map's device, 4-byte aligned).  Runs on the context's tracker stream behind the map's pending work and, for a
 * pyramid view, behind that pyramid's build (as revo_map_integrate), and waits for the result.  A counting launch runs first
 * and the records are written by a second one, so a refused call writes nothing.
 * device_out = 0: records in host memory in ascending key order.  device_out = 1: device memory, 16-byte aligned, unspecified
 * order.  records == NULL: counts only (cap is ignored).  *n_records = voxels_carved.  REVO_ERR_CAPACITY, nothing written, when
 * cap < *n_records.  info and view_info (n entries, host memory) may be NULL.
 * REVO_ERR_INVALID_ARG, before anything is enqueued: NULL m, views or n_records; n outside 1 .. 64; device_in or device_out
 * not 0 or 1; a view with both or neither of kf / depth; a pyramid of another context, or a batch view -- a pyramid
 * revo_map_integrate does not take: the frames of revo_batch_frame, not the keyframe slots of
 * revo_vo_keyframe / revo_vo_multi_keyframe (every pyramid is checked before any of them orders the stream); a size outside
 * 1 .. 2048; an intrinsic, range or pose that is not finite; fx or fy <= 0; zmin < 0 or zmin >= zmax; a rotation that fails
 * the is_orthogonal rule of revo_map_align_eval; radius outside 0 .. 3; margin or margin_rel not finite or negative; a
 * misaligned device pointer. */
int revo_map_carve_eval(revo_map* m, int n, const revo_map_carve_view* views, int device_in, const revo_map_carve_params* prm,
                        revo_map_voxel_raw* records, size_t cap, size_t* n_records, int device_out, revo_map_carve_info* info,
                        revo_map_carve_view_info* view_info);
/* The same arguments and outputs; the carved voxels then leave the map: revo_map_subtract_raw(m, the device records,
 * voxels_carved, 1, 0, 0).  revo_map_merge_raw(m, records, n_records, ., 0, 0) afterwards restores the map byte for byte,
 * counters included.  When cap is too small nothing is written and nothing is removed; host records are written after the
 * removal has succeeded, so a call that fails (REVO_ERR_HIP: no memory for the clean-up table, the map as it was) writes none;
 * a device buffer may then hold the records that were to go. */
int revo_map_carve(revo_map* m, int n, const revo_map_carve_view* views, int device_in, const revo_map_carve_params* prm,
                   revo_map_voxel_raw* records, size_t cap, size_t* n_records, int device_out, revo_map_carve_info* info,
                   revo_map_carve_view_info* view_info);

/* ---- rays through the map: hole-free views and range queries ---------------------------------------------
 * A ray visits the cells of the voxel grid in an order fixed by float32 arithmetic, one thread walks one ray alone and a hit
 * is a table lookup: no atomics decide anything, so the outputs are a pure function of the map's bytes and the rays -- the same
 * bytes whatever the table size, integration order, batching of views or launch.
 * All arithmetic is float32 with every operation rounded on its own; a / b is the correctly rounded quotient.
 *
 * A ray is o[3], s0, d[3], s1: the points o + s*d for s0 <= s < s1.  d is not normalised: s is in the unit d gives it.
 * The march, with `voxel` the map's edge:
 *  1. Start cell: g_i = o_i + s0*d_i, f_i = floorf(g_i / voxel).  The ray is OUTSIDE with 0 cells unless s0 < s1 (false for
 *     NaN), s1 is finite, every g_i is finite and -1048576 <= f_i <= 1048575.  k_i = (int)f_i.
 *  2. Per axis: inv_i = 1 / d_i.  d_i > 0: step_i = +1, pos_i = 1.  d_i < 0: step_i = -1, pos_i = 0.  d_i zero or NaN, or inv_i
 *     not finite: step_i = 0 and t_i = +inf.  Otherwise t_i = (((float)(k_i + pos_i)) * voxel - o_i) * inv_i.
 *  3. Loop, starting with s = s0 and cells = 0:
 *     - if cells == max_steps the ray is EXHAUSTED;
 *     - cells += 1; the cell k, packed into a key as integration packs it, is examined at entry parameter s: if it is solid,
 *       the ray is a HIT;
 *     - a = 0; if (t_1 < t_a) a = 1; if (t_2 < t_a) a = 2 (ties go to the lowest axis, NaN never wins); sn = t_a;
 *     - if !(sn < s1) the ray is a RANGE miss;
 *     - k_a += step_a; if k_a leaves [-2^20, 2^20 - 1] the ray is OUTSIDE;
 *     - s = sn, then t_a = (((float)(k_a + pos_a)) * voxel - o_a) * inv_a: recomputed from the integer index, never
 *       accumulated, so there is no drift.
 * Solid: the table holds the key with count >= max(min_count, 1).  For the rays of a view there is one more condition: the
 * voxel's point p, exactly as revo_map_extract forms it, taken to the camera exactly as revo_map_render does (Rc, tc formed on
 * the host, pc = ((Rc[:,0]*px + Rc[:,1]*py) + Rc[:,2]*pz) + tc), must be finite with zmin < z < zmax; a voxel that fails this is
 * transparent, as it is invisible to revo_map_render.  Cells that are not solid are marched through.
 *
 * A view is a revo_map_view with revo_map_render's rules and all-zero defaults; splat_max is not read.  Pixel (x, y) casts
 * dcx = ((float)x - cx)/fx, dcy = ((float)y - cy)/fy, d_i = ((R_i0*dcx) + (R_i1*dcy)) + R_i2 (R the rotation of T_w_c),
 * o = the translation of T_w_c, s0 = zmin, s1 = zmax: s is camera depth.
 * Hit: depth = z of the hit voxel's pc (> 0, so never the 0 of a miss), bgr = its colour as revo_map_extract rounds it,
 * key = its key: the voxel's mean, not the face of its cell.  Miss: depth 0, bgr 0, key all ones. */
typedef struct revo_map_ray_params {  /* 16 bytes; NULL: max_steps 4096 */
  uint32_t max_steps;       /* 1 .. 2^20: the cells a ray examines at most */
  uint32_t reserved[3];     /* zero */
} revo_map_ray_params;
typedef struct revo_map_ray {         /* 32 bytes */
  float o[3], s0, d[3], s1;
} revo_map_ray;
#define REVO_RAY_HIT 0u
#define REVO_RAY_RANGE 1u
#define REVO_RAY_OUTSIDE 2u
#define REVO_RAY_EXHAUSTED 3u
typedef struct revo_map_ray_hit {     /* 16 bytes per ray */
  uint64_t key;             /* the hit voxel's key; all ones unless the ray is a hit                               */
  float s;                  /* the entry parameter of the last cell examined (0 when no cell was)                  */
  uint32_t cells;           /* bits 0-23: the cells examined; bits 30-31: the status REVO_RAY_*; the rest zero      */
} revo_map_ray_hit;
typedef struct revo_map_ray_info {    /* 64 bytes, little-endian, no padding: integer sums over the rays of a call */
  uint64_t rays, hits, range, outside, exhausted;   /* rays = the sum of the four statuses */
  uint64_t cells;           /* cells examined in total */
  uint64_t reserved[2];     /* zero */
} revo_map_ray_info;
/* n views (1 .. 64, sizes may differ) of the map as it is behind every integration enqueued so far: one launch that builds the
 * table of occupied 8 x 8 x 8 blocks and one that marches a ray per pixel, on the context's tracker stream.  depth[i] (h x w
 * floats) is required; bgr (h x w x 3 bytes per view), key (h x w uint64 per view), hits (n entries: the hit pixels of each
 * view) and info (one record for the call) may be NULL, and bgr[i] / key[i] follow their array.  Every view must carry the
 * same max(min_count, 1).  device_out = 0: host pointers, the call waits.  device_out = 1: device pointers (every output,
 * hits and info included, 16-byte aligned), the call only enqueues.  An empty map gives all misses.  The map is not changed.
 * REVO_ERR_INVALID_ARG, before anything is enqueued and with nothing written: NULL m, views or depth, a NULL depth[i], bgr[i]
 * or key[i] of a given array; n outside 1 .. 64; revo_map_render's view rules (size, pose, intrinsics, depth range); views of
 * different min_count; max_steps outside 1 .. 2^20; a reserved word that is not 0; device_out not 0 or 1; a misaligned device
 * pointer. */
int revo_map_raycast(revo_map* m, int n, const revo_map_view* views, const revo_map_ray_params* prm, float* const* depth,
                     uint8_t* const* bgr, uint64_t* const* key, uint32_t* hits, int device_out, revo_map_ray_info* info);
/* n rays (1 .. 2^24) against the voxels with count >= max(min_count, 1): one revo_map_ray_hit per ray.  device_in: where the
 * rays live (0: host memory, uploaded to a temporary buffer, the call waits; 1: device memory of the map's device, 16-byte
 * aligned).  device_out: as above, for out and info (NULL allowed).  A ray that is not finite or has s0 >= s1 is no argument
 * error: it comes back OUTSIDE with 0 cells.  REVO_ERR_INVALID_ARG as above: NULL m, rays or out; n outside 1 .. 2^24; the
 * parameter rules; a flag outside 0 / 1; a misaligned device pointer. */
int revo_map_cast_rays(revo_map* m, size_t n, const revo_map_ray* rays, int device_in, uint32_t min_count,
                       const revo_map_ray_params* prm, revo_map_ray_hit* out, int device_out, revo_map_ray_info* info);
/* Waits for the last revo_map_raycast / revo_map_cast_rays of m and gives the device time from the start of its block-table
 * launch to the end of its march (HIP events on the tracker stream), in milliseconds.  REVO_ERR_INVALID_ARG if m has cast
 * nothing yet. */
int revo_map_raycast_last_ms(revo_map* m, float* ms);

/* The map's distance field: what a planner asks -- how far is the nearest surface from here, and in which
 * direction.  The field is the exact squared Euclidean distance, in cells, from every cell of a box of voxel indices to the
 * nearest solid voxel inside the box: an integer with one value, so a pure function of the map's records -- the same bytes
 * whatever the table size, integration order or launch.
 *
 * The box: cell (ix, iy, iz) is the voxel index lo + (ix, iy, iz) and lives at out[(ix*n[1] + iy)*n[2] + iz] (z fastest, the
 * key's own order).  Every lo[i] and lo[i] + n[i] - 1 lies in [-2^20, 2^20 - 1], and n[0]*n[1]*n[2] <= 2^27.
 * The field: a voxel is solid when its count >= max(min_count, 1).  out[c] = the minimum, over the solid voxels s whose index
 * lies inside the box, of (cx-sx)^2 + (cy-sy)^2 + (cz-sz)^2; REVO_DF_NONE when the box holds no solid voxel.  With clamp > 0
 * every value other than REVO_DF_NONE is written as min(value, clamp).  Voxels outside the box are NOT seen: a value is exact
 * only up to the cell's distance to the nearest face, so the caller pads the box by the distance it cares about.  The largest
 * possible value is 3 * 1023^2 < 2^24, so (float)out[c] is exact. */
typedef struct revo_map_df_box {
  int32_t lo[3];            /* voxel index of the first cell, per axis x, y, z */
  int32_t n[3];             /* cells per axis, 1 .. 1024 */
} revo_map_df_box;
#define REVO_DF_NONE 0xFFFFFFFFu
typedef struct revo_map_df_info {     /* 64 bytes, little-endian, no padding: integer sums and maxima, so order-free */
  uint64_t cells;           /* n[0]*n[1]*n[2] */
  uint64_t solid;           /* solid voxels inside the box */
  uint64_t outside;         /* solid voxels outside it */
  uint64_t below;           /* voxels under max(min_count, 1) */
  uint64_t max_d2;          /* the largest value written other than REVO_DF_NONE, after the clamp; 0 if there is none */
  uint64_t reserved[3];     /* zero */
} revo_map_df_info;
typedef struct revo_map_df_sample_t { /* 16 bytes per point */
  float dist;               /* metres to the nearest solid voxel's cell; -1: the point is outside the box; +inf: no solid voxel */
  float grad[3];            /* central difference of the distance in cells per cell, dimensionless; one-sided at a face */
} revo_map_df_sample_t;
/* The field of `box` over the map as it is behind every integration enqueued so far, on the context's tracker stream: n[0]*
 * n[1]*n[2] values into d2, the call's counters into info (may be NULL).  device_out = 0: host pointers, the call waits.
 * device_out = 1: device pointers (d2 and info 16-byte aligned), the call only enqueues.  An empty map gives all
 * REVO_DF_NONE.  The map is not changed.  REVO_ERR_INVALID_ARG, before anything is enqueued and with nothing written: NULL m,
 * box or d2; a size outside 1 .. 1024; more than 2^27 cells; a box that leaves the index range; device_out not 0 or 1; a
 * misaligned device pointer. */
int revo_map_distance_field(revo_map* m, const revo_map_df_box* box, uint32_t min_count, uint32_t clamp, uint32_t* d2, int device_out,
                            revo_map_df_info* info);
/* Waits for the map and gives the smallest (lo) and largest (hi) voxel index per axis over the voxels with count >=
 * max(min_count, 1), and how many there are (n).  With *n == 0, lo and hi are written as zeros. */
int revo_map_bounds(revo_map* m, uint32_t min_count, int32_t lo[3], int32_t hi[3], size_t* n);
/* n points (1 .. 2^24; xyz: 3 floats each, metres in the map's frame) against the field d2 of `box` (device_field: where d2
 * lives; a host field is uploaded to a temporary buffer).  All arithmetic is float32 with every operation rounded on its own;
 * sqrtf and / are correctly rounded.  Per axis f_i = floorf(p_i / voxel), voxel the map's edge.  The point is OUTSIDE unless
 * every p_i and f_i is finite and lo_i <= f_i <= lo_i + n_i - 1: then dist = -1 and grad = 0.  Otherwise, with a the cell
 * f - lo: d2[a] == REVO_DF_NONE gives dist = +inf and grad = 0; else dist = sqrtf((float)d2[a]) * voxel and, per axis i with
 * a_i the cell's index along it, lo' = max(a_i - 1, 0), hi' = min(a_i + 1, n_i - 1), span = hi' - lo', grad_i = span == 0 ? 0
 * : (sqrtf((float)d2[a with a_i = hi']) - sqrtf((float)d2[a with a_i = lo'])) / (float)span.
 * device_in / device_out: where xyz and out live (device pointers 16-byte aligned); the call only enqueues when all three
 * flags are 1 and waits otherwise.  A point that is not finite is no argument error: it comes back OUTSIDE.
 * REVO_ERR_INVALID_ARG, with nothing written: a NULL pointer; n outside 1 .. 2^24; the box rules above; a flag outside 0 / 1;
 * a misaligned device pointer. */
int revo_map_df_sample(revo_map* m, const revo_map_df_box* box, const uint32_t* d2, int device_field, size_t n, const float* xyz,
                       int device_in, revo_map_df_sample_t* out, int device_out);
/* Waits for the last revo_map_distance_field of m and gives the device time from its first memset to the end of its last pass
 * (HIP events on the tracker stream), in milliseconds.  REVO_ERR_INVALID_ARG if m has built no field yet. */
int revo_map_distance_field_last_ms(revo_map* m, float* ms);

/* ---- registration against the distance field ----------------------------------------------------------
 * revo_map_align and revo_map_align_plane match a source voxel among the 27 destination voxels around it, so a pose more
 * than about a voxel off finds no or wrong matches, and their source must be a map.  Here the residual of a source POINT
 * under a pose is the field's value at the moved point, read by trilinear interpolation of sqrt(d2) between cell centres,
 * and its gradient the exact derivative of that interpolant: no neighbour search, any point set as the source, and a basin
 * as wide as the box the field was built over.
 *
 * The record of one pose.  m, box, d2, device_field: revo_map_df_sample's field arguments with its rules; m gives the voxel
 * edge v, the context and the stream.  Per point p (xyz: npts packed float[3], source frame) and pose (R column-major, t),
 * float32 with every operation rounded on its own (/ and sqrtf correctly rounded, no fused multiply-add):
 *   p'_i = ((R_i0*px + R_i1*py) + R_i2*pz) + t_i;
 *   per axis  g_i = p'_i / v - 0.5f,  f_i = floorf(g_i),  w_i = g_i - f_i,  a_i = f_i - (float)lo_i;
 *   the point is SKIPPED (and counted) unless every p'_i and g_i is finite and 0 <= a_i <= (float)(n_i - 2) on every axis
 *         (compared in float before the conversion; an axis of one cell skips every point), or if any of the 8 cells
 *         a + {0,1}^3 holds REVO_DF_NONE;
 *   s_abc = sqrtf((float)d2[a + (a,b,c)]);  lerp(x0, x1, w) = x0 + w*(x1 - x0)  (one subtraction, product, addition);
 *   along z:  m_ab = lerp(s_ab0, s_ab1, w_z),  dz_ab = s_ab1 - s_ab0;
 *   along y:  l_a = lerp(m_a0, m_a1, w_y),  h_a = m_a1 - m_a0,  k_a = lerp(dz_a0, dz_a1, w_y);
 *   along x:  c = lerp(l_0, l_1, w_x),  gx = l_1 - l_0,  gy = lerp(h_0, h_1, w_x),  gz = lerp(k_0, k_1, w_x);
 *   e = c*v, the residual in metres; (gx, gy, gz) its dimensionless gradient, the exact derivative of the interpolant;
 *   the point is accepted iff e <= max_dist (inclusive), otherwise GATED (the gated count is considered - matched - skipped).
 * Per accepted point, with u = p' - centre:
 *   a  = u x g:  ax = uy*gz - uz*gy,  ay = uz*gx - ux*gz,  az = ux*gy - uy*gx  (two products and one subtraction each);
 *   J  = (gx, gy, gz, ax, ay, az);
 *   S[0..20]  J_i*J_j for i <= j, row by row (00 01 .. 05 11 .. 55);  S[21..26]  J_i*e;  S[27]  e*e  (one product each).
 * Each S is the float nearest the exact sum of its float terms (double-double from the first addition, rounded once;
 * DESIGN 4.1's midpoint caveat applies).  The counts are exact. */
typedef struct revo_map_df_align_info {   /* 208 bytes, little-endian, no padding holes */
  float    S[28];
  uint64_t matched;      /* accepted points                                                                           */
  uint64_t considered;   /* npts                                                                                      */
  uint64_t skipped;      /* points outside the interpolation cells of the box, not finite, or next to REVO_DF_NONE    */
  float    centre[3], max_dist;  /* copied from the parameters                                                        */
  float    R[9], T[3];   /* the pose the sums were taken at (source -> field frame, R column-major), as given         */
  int32_t  flags;        /* bit0 as revo_map_align_info's: everything else is then zero except pose, centre, max_dist */
  int32_t  reserved;     /* zero */
} revo_map_df_align_info;

/* One record per pose (nposes 1 .. 65535, 4x4 column-major, source -> field frame), all poses in ONE launch on m's
 * context's tracker stream.  npts: 1 .. 2^24.  prm: max_dist finite and > 0 (no upper bound: the field decides how far a
 * point may lie), centre finite as in revo_map_align; min_count_dst and min_count_src must be 0.  device_in / device_out:
 * where xyz and out live (device pointers 16-byte aligned); a host field or host points are uploaded to temporary buffers.
 * The call only enqueues when field, points and output are all on the device, and waits otherwise (revo_map_df_sample's
 * rule).  The map is not read or changed.  A point that is not finite is no argument error: it is skipped.
 * REVO_ERR_INVALID_ARG, before anything is enqueued and with nothing written: a NULL pointer; npts or nposes out of range;
 * the box rules of revo_map_distance_field; a flag outside 0 / 1; a misaligned device pointer; a max_dist or centre that is
 * not finite, or max_dist <= 0; a min_count field that is not 0. */
int revo_map_df_align_eval(revo_map* m, const revo_map_df_box* box, const uint32_t* d2, int device_field, size_t npts,
                           const float* xyz, int device_in, int nposes, const float* T_dst_src_n16,
                           const revo_map_align_params* prm, revo_map_df_align_info* out, int device_out);

/* Host only.  revo_map_align_plane_system's arithmetic with g in the normal's place: e(x) ~ e + g.v + w.(u x g) = e + J.x,
 * H = sum J J^T from its upper triangle S[0..20], g = S[21..26], cost = S[27].  REVO_ERR_INVALID_ARG: NULL, or flags bit0. */
int revo_map_df_align_system(const revo_map_df_align_info* info, double H[36], double g[6]);

/* revo_map_align's Gauss-Newton loop over revo_map_df_align_eval's records: the same options, Cholesky and pivot rule,
 * update T <- Tr(c) exp(x) Tr(-c) T, stopping rule and statuses; info_out from one more evaluation.  A host field and host
 * points are uploaded once per call.  The call waits.  REVO_ERR_INVALID_ARG: as revo_map_df_align_eval, a T_init that is
 * not finite, max_iters < 1. */
int revo_map_df_align(revo_map* m, const revo_map_df_box* box, const uint32_t* d2, int device_field, size_t npts,
                      const float* xyz, int device_in, const float T_init[16], const revo_map_align_params* prm,
                      const revo_map_align_opts* opt, float T_out[16], revo_map_df_align_info* info_out, int32_t* iterations,
                      int32_t* status);

/* ---- planning through the map -------------------------------------------------------------------------
 * The planner's own step: the clearance-aware cost-to-go from a set of goal cells to every cell of a field's box, and the
 * paths that descend it.  A shortest-path cost over integer step weights has one value per cell, so it is a pure function of
 * the field, the clearance and the seeds -- the same bytes on every run, whatever the launch.
 *
 * The grid: m, box, d2, device_field are revo_map_df_sample's field arguments with its box rules; m gives the context, the
 * stream and the voxel edge and is neither read nor changed.  With r2 >= 1 the squared clearance in cells, a cell c is FREE
 * iff d2[c] >= r2.  REVO_DF_NONE is therefore free (nothing in the box: infinite clearance); a solid cell (d2 = 0) never is.
 * A field clamped below r2 has no free cell but its REVO_DF_NONE ones: build the field with clamp = 0 or clamp >= r2.
 * The moves: from a free cell to any of its 26 neighbours inside the box that is free, at the weight 3, 4 or 5 for a step
 * that changes 1, 2 or 3 coordinates (the 3-4-5 chamfer).  There is no corner rule: the clearance has inflated the obstacles.
 * The seeds: n_seeds (1 .. 2^20) records in host memory, cell a voxel index (absolute, like box.lo), cost0 <= 2^24.  A seed
 * outside the box is ignored and counted in seeds_outside, one on a cell that is not free in seeds_blocked, every other one
 * in seeds_used (seeds_used + seeds_outside + seeds_blocked = n_seeds); seeds of one cell act as the one of smallest cost0.
 * The cost: cost[c], in the field's own layout (ix*n[1] + iy)*n[2] + iz, is the minimum over the used seeds s and over all
 * paths of moves from s's cell to c of cost0[s] + the weights; REVO_PLAN_NONE for a cell that is not free or that no seed
 * reaches.  The largest finite value is below 2^24 + 5 * 2^27 < 2^30.  In a box that is all free the cost from one seed of
 * cost0 = 0 at the offset (a >= b >= c >= 0), axes sorted, is 3a + b + c. */
typedef struct revo_map_plan_seed {   /* 16 bytes */
  int32_t cell[3];          /* voxel index x, y, z */
  uint32_t cost0;           /* the cost at the seed, <= 2^24 */
} revo_map_plan_seed;
#define REVO_PLAN_NONE 0xFFFFFFFFu
typedef struct revo_map_plan_info {   /* 64 bytes, little-endian, no padding: integer sums and maxima, so order-free */
  uint64_t cells;           /* n[0]*n[1]*n[2] */
  uint64_t free;            /* cells with d2 >= r2 */
  uint64_t reachable;       /* cells with a cost other than REVO_PLAN_NONE */
  uint64_t max_cost;        /* the largest of them; 0 if nothing is reachable */
  uint64_t seeds_used, seeds_outside, seeds_blocked;
  uint64_t reserved;        /* zero */
} revo_map_plan_info;
/* The cost field of `box` on the context's tracker stream: n[0]*n[1]*n[2] values into cost, the counters into info (may be
 * NULL).  device_out: where cost and info live (1: device memory of the map's device, 16-byte aligned).  max_rounds: how
 * many relaxation rounds may run (0: 65 536).  The call ALWAYS waits: the host decides when the fixed point is reached.
 * REVO_ERR_INVALID_ARG, before anything is enqueued and with nothing written: NULL m, box, d2, seeds or cost; the box rules
 * of revo_map_distance_field; r2 = 0; n_seeds outside 1 .. 2^20; a cost0 above 2^24; a flag outside 0 / 1; a misaligned
 * device pointer.  REVO_ERR_CAPACITY: the fixed point was not reached within max_rounds; the contents of cost are then
 * unspecified (upper bounds in an internal encoding, or untouched host memory) and info is not written. */
int revo_map_plan(revo_map* m, const revo_map_df_box* box, const uint32_t* d2, int device_field, uint32_t r2, size_t n_seeds,
                  const revo_map_plan_seed* seeds, uint32_t max_rounds, uint32_t* cost, int device_out, revo_map_plan_info* info);
/* Waits for the last revo_map_plan of m and gives its device time from the first kernel to the end of the last one (HIP
 * events on the tracker stream, the host's waits between the groups of rounds included), in milliseconds, and the number of
 * the last relaxation round in which a tile did work.  Both depend on the implementation, so they are not part of
 * revo_map_plan_info.  Either pointer may be NULL, not both.  REVO_ERR_INVALID_ARG if m has planned nothing yet. */
int revo_map_plan_last(revo_map* m, float* ms, uint32_t* rounds);

enum { REVO_PLAN_REACHED = 0,     /* the path ends on a seed's cell */
       REVO_PLAN_UNREACHABLE = 1, /* the start's cost is REVO_PLAN_NONE: length 0 */
       REVO_PLAN_OUTSIDE = 2,     /* the start is not in the box: length 0, cost REVO_PLAN_NONE */
       REVO_PLAN_TRUNCATED = 3    /* max_len cells were written before a seed was reached */ };
typedef struct revo_map_plan_path {   /* 16 bytes per start */
  uint32_t length;          /* cells written for this start */
  uint32_t status;          /* REVO_PLAN_* */
  uint32_t cost;            /* the start's cost */
  uint32_t reserved;        /* zero */
} revo_map_plan_path;
/* Paths down a cost field (cost, device_cost: where it lives; a host field is uploaded to a temporary buffer): one per start
 * (n_starts 1 .. 2^20, int32[3] voxel indices each, host memory), at most max_len (1 .. 2^20) cells each.  From cell c the
 * next cell is the FIRST neighbour in the fixed order -- dx outermost, then dy, then dz, each -1, 0, 1, the cell itself
 * skipped -- that lies inside the box and has cost[nb] != REVO_PLAN_NONE and cost[nb] + w == cost[c], w the move's weight;
 * where there is none, c is a seed's cell and the path ends there.  cells_out[i][k] (int32[n_starts][max_len][3]) is the
 * k-th cell of path i as an absolute voxel index, the start first; entries past length are not written.  No d2 is needed:
 * the cost field says which cells are free.  device_out: where cells_out and path_out live (device pointers 16-byte
 * aligned); with host outputs cells_out travels to the device and back, so that what the call does not write stays.  The
 * call only enqueues when cost field and outputs are on the device, and waits otherwise.  REVO_ERR_INVALID_ARG, with
 * nothing written: a NULL pointer; n_starts or max_len out of range; the box rules; a flag outside 0 / 1; a misaligned
 * device pointer. */
int revo_map_plan_paths(revo_map* m, const revo_map_df_box* box, const uint32_t* cost, int device_cost, size_t n_starts,
                        const int32_t* starts, uint32_t max_len, int32_t* cells_out, revo_map_plan_path* path_out, int device_out);

/* ---- known space: the seen volume, the known field, the frontiers ------------------------------------------
 * The map says what is there; the seen volume says what has been looked at.  It is one byte per cell of a distance-field box
 * (revo_map_df_box with its rules; cell (ix, iy, iz) at seen[(ix*n[1] + iy)*n[2] + iz], z fastest): the low seven bits count
 * the views that looked through the cell's centre (free votes, saturating at 127), bit 7 says that a view measured a surface
 * there.  Every value is an integer decided by float32 arithmetic with one definition, so the bytes are a pure function of
 * the inputs -- the same on every run, whatever the launch.
 *
 * The cell's point: for the cell a of the box, p_i = ((float)(lo_i + a_i) + 0.5f) * voxel, voxel the map's edge (the sum is
 * exact, the product rounded once): the cell's centre.  The cell's class in a view is revo_map_carve_eval's class of p, with
 * the views, the radius and the margins read exactly as there.  The map's voxels play no part: a solid voxel's cell gets what
 * its centre's class gives.
 * The byte: with in = accumulate ? seen[c] : 0, f the number of views of the call in which p is FREE and s = 1 if p is
 * CONFIRMED in any of them,
 *     seen[c] = ((in | (s << 7)) & 0x80) | min(127, (in & 0x7F) + f).
 * Exact properties: the order of the views cannot show; revo_map_observe with views A followed by an accumulating call with
 * views B leaves the bytes of one call with A and B together, saturation included; a call that does not accumulate does not
 * read seen. */
typedef struct revo_map_observe_params { /* 16 bytes; NULL: 1, 0, the map's voxel edge, 0 */
  int32_t radius;        /* 0 .. 3: half width of the pixel window, as revo_map_carve_params'     */
  uint32_t accumulate;   /* 0: seen is written; 1: seen is read and updated                        */
  float margin;          /* metres, finite, >= 0                                                   */
  float margin_rel;      /* per metre of depth, finite, >= 0                                       */
} revo_map_observe_params;
typedef struct revo_map_observe_info {   /* 64 bytes, little-endian, no padding: integer sums, so order-free */
  uint64_t cells;           /* n[0]*n[1]*n[2]                                               */
  uint64_t cells_free;      /* cells whose free votes are not 0 after the call              */
  uint64_t cells_surface;   /* cells whose bit 7 is set after the call                      */
  uint64_t votes;           /* the sum of f over the cells: this call's FREE classifications */
  uint64_t newly_known;     /* cells with in == 0 and a byte other than 0 after the call    */
  uint64_t reserved[3];     /* zero */
} revo_map_observe_info;
/* The seen volume of `box` from n views (1 .. 64; revo_map_carve_view with every rule of revo_map_carve_eval: kf or a raw
 * depth image, the all-zero intrinsics, the pose rules, device_in; every pyramid is checked before anything is enqueued, host
 * images are uploaded to one temporary buffer).  Runs on the context's tracker stream, for a pyramid view behind that
 * pyramid's build.  The map gives the context, the stream and the voxel edge and is not changed.
 * device_seen = 0: seen, info and view_info (n records: the cells of the box by class, summing to cells) are host pointers
 * and the call waits.  device_seen = 1: all three are device pointers of the map's device, 16-byte aligned; with device images
 * or pyramids the call only enqueues, with host images it waits.  info and view_info may be NULL.
 * REVO_ERR_INVALID_ARG, before anything is enqueued and with nothing written: NULL m, box, views or seen; the box rules of
 * revo_map_distance_field; n outside 1 .. 64; the view rules of revo_map_carve_eval; radius outside 0 .. 3; accumulate above
 * 1; a margin that is not finite or negative; a flag outside 0 / 1; a misaligned device pointer. */
int revo_map_observe(revo_map* m, const revo_map_df_box* box, int n, const revo_map_carve_view* views, int device_in,
                     const revo_map_observe_params* prm, uint8_t* seen, int device_seen, revo_map_observe_info* info,
                     revo_map_carve_view_info* view_info);

/* The distance field with unseen space as an obstacle.  A cell is SOLID as in revo_map_distance_field; it is KNOWN if it is
 * solid, or (seen[c] & 0x7F) >= max(min_views, 1), or seen[c] & 0x80; otherwise it is UNKNOWN.  d2 is
 * revo_map_distance_field's definition over the obstacle set solid + unknown: the exact squared distance in cells to the
 * nearest such cell inside the box, REVO_DF_NONE only if the set is empty, clamp as there.  revo_map_plan over this field
 * keeps the clearance from unseen space too, and a goal in unseen space counts in seeds_blocked. */
typedef struct revo_map_known_info {  /* 64 bytes; the first five words are revo_map_df_info's */
  uint64_t cells, solid, outside, below;
  uint64_t max_d2;
  uint64_t unknown;         /* cells of the box that are not known                          */
  uint64_t known_free;      /* cells - solid - unknown                                      */
  uint64_t reserved;        /* zero */
} revo_map_known_info;
/* seen: the box's seen volume, n[0]*n[1]*n[2] bytes (device_seen: where it lives; a host volume is uploaded).  d2, device_out
 * and info as revo_map_distance_field's.  The call only enqueues when both flags are 1 and waits otherwise.
 * REVO_ERR_INVALID_ARG, before anything is enqueued and with nothing written: revo_map_distance_field's rules; NULL seen; a
 * flag outside 0 / 1; a device seen that is not 16-byte aligned. */
int revo_map_known_field(revo_map* m, const revo_map_df_box* box, uint32_t min_count, uint32_t clamp, const uint8_t* seen,
                         int device_seen, uint32_t min_views, uint32_t* d2, int device_out, revo_map_known_info* info);

/* Where known space ends.  A frontier cell is not solid, has (seen[c] & 0x7F) >= max(min_views, 1), and at least one of its six
 * face neighbours INSIDE the box is unknown as defined above (cells at the box's faces have fewer neighbours: the outside of
 * the box is not unknown).  The records are revo_map_plan_seed: the absolute voxel index and cost0 = 0; revo_map_plan takes
 * them as they are.  *n_cells = the number of frontier cells.  device_out = 0: host records in ascending order of the cell's
 * place in the box (x, then y, then z).  device_out = 1: device memory, 16-byte aligned, unspecified order.  cells == NULL:
 * count only (cap is ignored).  REVO_ERR_CAPACITY with nothing written when cap < *n_cells.  A counting launch runs first and
 * a second one writes; the call waits.  REVO_ERR_INVALID_ARG, with nothing written: NULL m, box, seen or n_cells; the box
 * rules; a flag outside 0 / 1; a misaligned device pointer (16 bytes). */
int revo_map_frontiers(revo_map* m, const revo_map_df_box* box, uint32_t min_count, const uint8_t* seen, int device_seen,
                       uint32_t min_views, revo_map_plan_seed* cells, size_t cap, size_t* n_cells, int device_out);

/* ---- what a view would add: the unknown space candidate poses would reveal --------------------------------
 * A read-only, batched question to the map and a seen volume: for each of n_poses camera poses, how many cells that are
 * unknown now would one depth view from there make known?  Nothing is observed and nothing is written but the records.  Every
 * value is an integer decided by float32 arithmetic with one definition, so a pose's record is a pure function of the map, the
 * seen volume, the camera and that pose -- the same bytes on every run, whatever the launch.
 *
 * The predicted view.  cam gives the size, the intrinsics, the depth range and min_count with revo_map_raycast's rules and
 * its all-zero defaults; cam's own T_w_c and splat_max are not read.  The predicted depth image of pose i (16 floats,
 * column-major camera -> world, revo_map_carve_eval's pose rules: finite, rotation orthogonal) is exactly the depth output
 * of revo_map_raycast for cam with that pose and max_steps: the hit voxel's z, 0 for a ray that hits nothing.  With
 * miss_depth != 0 every 0 of the image (a miss) is then replaced by miss_depth: free space is taken as seen up to there.
 * The cells.  A cell's centre p is revo_map_observe's; its class in the predicted view is revo_map_carve_eval's class of p
 * in a raw view with cam's size, intrinsics and range, the pose and the predicted image, with radius, margin and margin_rel
 * read exactly as there.  A cell is UNKNOWN exactly as in revo_map_known_field: not solid at cam's min_count,
 * (seen[c] & 0x7F) < max(min_views, 1), and bit 7 clear.
 * Exact properties: the record of a pose does not depend on the other poses of the call, on their order, or on how the call
 * is split into launches; seen and the map are not written; with min_views = 1 the cells counted by unknown_free +
 * unknown_surface are exactly the unknown cells whose byte changes under revo_map_observe(accumulate = 1) with the predicted
 * image (its misses replaced when miss_depth != 0) as a raw view. */
typedef struct revo_map_gain_params {  /* 32 bytes; NULL: 1, 1, the map's voxel edge, 0, 0, 4096 */
  int32_t radius;        /* 0 .. 3: half width of the pixel window, as revo_map_observe_params'                    */
  uint32_t min_views;    /* free votes that make a cell known; 0 counts as 1                                        */
  float margin;          /* metres, finite, >= 0                                                                    */
  float margin_rel;      /* per metre of depth, finite, >= 0                                                        */
  float miss_depth;      /* 0: a miss stays a depth hole; else zmin < miss_depth < zmax, the depth a miss is read as */
  uint32_t max_steps;    /* 1 .. 2^20: the cells a ray examines at most, as revo_map_ray_params'                    */
  uint32_t reserved[2];  /* zero */
} revo_map_gain_params;
typedef struct revo_map_gain {         /* 32 bytes per pose; the three cell counts are over the UNKNOWN cells of the box */
  uint32_t unknown_free;     /* unknown cells whose class is FREE                                   */
  uint32_t unknown_surface;  /* unknown cells whose class is CONFIRMED                              */
  uint32_t unknown_inside;   /* unknown cells whose class is not OUTSIDE                            */
  uint32_t hits;             /* hit pixels of the predicted view, before miss_depth is applied      */
  uint32_t reserved[4];      /* zero */
} revo_map_gain;
typedef struct revo_map_gain_info {    /* 64 bytes, little-endian, no padding: integer sums, so order-free */
  uint64_t poses;            /* n_poses                                                             */
  uint64_t cells;            /* n[0]*n[1]*n[2]                                                      */
  uint64_t unknown;          /* unknown cells of the box                                            */
  uint64_t unknown_free, unknown_surface, unknown_inside;  /* the sums of the per-pose counts      */
  uint64_t rays;             /* rays cast: width*height per pose that keeps the pose rules          */
  uint64_t ray_hits;         /* the sum of the per-pose hits                                        */
} revo_map_gain_info;
/* seen: the box's seen volume (device_seen: where it lives; a host volume is uploaded).  T_w_c_n16: n_poses (1 .. 4096)
 * poses (device_in: where they live).  out: n_poses records, info: NULL or the call's record (device_out: where both live).
 * Device pointers are 16-byte aligned.  Runs on the context's tracker stream; the call only enqueues when all three flags are
 * 1 and waits otherwise.  Poses in host memory are checked; poses in device memory are not: one that breaks the pose rules
 * gives an all-zero record, casts no ray and is no error, as revo_map_cast_rays treats a bad ray.
 * REVO_ERR_INVALID_ARG, before anything is enqueued and with nothing written: NULL m, box, seen, cam, poses or out; the box
 * rules of revo_map_distance_field; the view rules of revo_map_raycast on cam; n_poses outside 1 .. 4096; a host pose that is
 * not finite or whose rotation is not orthogonal; radius outside 0 .. 3; a margin that is not finite or negative; a
 * miss_depth that is neither 0 nor inside (zmin, zmax); max_steps outside 1 .. 2^20; a reserved word that is not 0; a flag
 * outside 0 / 1; a misaligned device pointer. */
int revo_map_view_gain(revo_map* m, const revo_map_df_box* box, const uint8_t* seen, int device_seen,
                       const revo_map_view* cam, size_t n_poses, const float* T_w_c_n16, int device_in,
                       const revo_map_gain_params* prm, revo_map_gain* out, int device_out,
                       revo_map_gain_info* info);

/* ---- a surface: the TSDF volume fused from depth views, and the mesh of its zero level set -----------------
 * The volume is one 8-byte cell per cell of a distance-field box (revo_map_df_box with its rules, z fastest, at most 2^27
 * cells): the integer sum of the views' truncated signed distances in units of trunc / 1024, and how many views gave one.
 * Every value is an integer decided by float32 arithmetic with one definition and the sums are integer sums, so the volume
 * is a pure function of the inputs -- the same bytes on every run, whatever the launch and whatever the order of the views.
 *
 * The cell's point p is revo_map_observe's centre.  Per view, the class of p is revo_map_carve_eval's class at radius 0 with
 * margin = trunc and margin_rel = 0, read exactly as there.  With dc the centre pixel's depth D[iv, iu] and z the camera-space
 * depth of p that the class rule computes:
 *   FREE       q = 1024                                                  (in front of the surface by more than trunc)
 *   CONFIRMED  q = (int32_t)rintf(((dc - z) / trunc) * 1024.0f), a difference, a quotient, a product and the rounding to the
 *              nearest integer (ties to even), each on its own; |z - dc| <= trunc holds, so |q| <= 1024 without a clamp
 *   every other class: no update.
 * An update is sum += q, weight += 1, the views taken in their order.  A cell whose weight has reached 2^20 takes no further
 * update; a dropped update is counted in saturated.  So |sum| <= 2^30.
 * Exact properties: while saturated == 0 the order of the views cannot show; revo_map_tsdf_fuse with views A followed by an
 * accumulating call with views B leaves the bytes of one call with A and B together; a call that does not accumulate does not
 * read the volume; for at most 127 views weight > 0 holds exactly where revo_map_observe with radius 0, margin = trunc and
 * margin_rel = 0 leaves a byte other than 0, and view_info equals that call's view_info. */
typedef struct revo_map_tsdf_cell {      /* 8 bytes */
  int32_t sum;           /* the sum of q over the cell's updates, in units of trunc / 1024                 */
  uint32_t weight;       /* the updates, at most 2^20                                                       */
} revo_map_tsdf_cell;
typedef struct revo_map_tsdf_params {    /* 16 bytes; NULL: 4 x the map's voxel edge, 0 */
  float trunc;           /* metres, finite, > 0                                                             */
  uint32_t accumulate;   /* 0: the volume is written; 1: it is read and updated                             */
  uint32_t reserved[2];  /* zero */
} revo_map_tsdf_params;
typedef struct revo_map_tsdf_info {      /* 64 bytes, little-endian, no padding: integer sums, so order-free */
  uint64_t cells;           /* n[0]*n[1]*n[2]                                               */
  uint64_t updates;         /* the updates of this call                                     */
  uint64_t cells_weighted;  /* cells with weight > 0 after the call                         */
  uint64_t cells_inside;    /* of those, the cells with sum < 0                             */
  uint64_t saturated;       /* the updates of this call that a full weight dropped          */
  uint64_t reserved[3];     /* zero */
} revo_map_tsdf_info;
/* The volume of `box` from n views (1 .. 64; revo_map_carve_view with every rule of revo_map_carve_eval, device_in as there;
 * every pyramid and image is checked before anything is enqueued, host images are uploaded to one temporary buffer).  Runs on
 * the context's tracker stream, for a pyramid view behind that pyramid's build.  The map gives the context, the stream and the
 * voxel edge and is not changed.
 * device_tsdf = 0: tsdf, info and view_info (n records: the cells of the box by class, summing to cells) are host pointers and
 * the call waits.  device_tsdf = 1: all three are device pointers of the map's device, 16-byte aligned; with device images or
 * pyramids the call only enqueues, with host images it waits.  info and view_info may be NULL.
 * REVO_ERR_INVALID_ARG, before anything is enqueued and with nothing written: NULL m, box, views or tsdf; the box rules of
 * revo_map_distance_field; n outside 1 .. 64; the view rules of revo_map_carve_eval; a trunc that is not finite or not > 0;
 * accumulate above 1; a reserved word that is not 0; a flag outside 0 / 1; a misaligned device pointer. */
int revo_map_tsdf_fuse(revo_map* m, const revo_map_df_box* box, int n, const revo_map_carve_view* views, int device_in,
                       const revo_map_tsdf_params* prm, revo_map_tsdf_cell* tsdf, int device_tsdf, revo_map_tsdf_info* info,
                       revo_map_carve_view_info* view_info);

/* The mesh of the volume's zero level set, in one canonical order: a pure function of the volume's bytes, the box, the voxel
 * edge and min_weight.  All decisions are integer.
 * A cell is VALID when weight >= max(min_weight, 1) and INSIDE when it is valid and sum < 0 (sum >= 0 is outside).  A cube at
 * the cell c has the corners c + {0,1}^3, all inside the box (a box with an axis of 1 has no cube); it is ACTIVE when all eight
 * corners are valid.  An active cube is split into the six tetrahedra of the Kuhn triangulation, one per permutation pi of
 * (x, y, z) in lexicographic order (xyz, xzy, yxz, yzx, zxy, zyx): v0 = c, v1 = v0 + e_pi(0), v2 = v1 + e_pi(1), v3 = c + (1,1,1).
 * Face diagonals agree between neighbouring cubes, so the mesh is watertight inside the active region.
 * Vertices sit on lattice edges.  An edge is (cell, type), type = dx + 2 dy + 4 dz - 1 in 0 .. 6, from the cell to cell +
 * (dx, dy, dz).  It carries a vertex when its end points differ in INSIDE and it is an edge of a tetrahedron of at least one
 * active cube (an axis edge belongs to four cubes, a face diagonal to two, the body diagonal to one).  With (s0, w0) the cell
 * at the lower end and (s1, w1) at the upper: n0 = (int64)s0*w1, n1 = (int64)s1*w0 (both below 2^51 in size),
 * a = (float)((double)n0 / (double)(n0 - n1)), and per axis pos_i = (((float)(lo_i + c_i) + 0.5f) + (d_i ? a : 0.0f)) * voxel,
 * every operation rounded on its own.  Vertices are listed in ascending order of (the cell's place in the box, type).
 * Triangles are listed in ascending order of (the cube's place, tetrahedron, k), three vertex indices each.  By how many of
 * v0 .. v3 are inside: 0 or 4: none.  1 or 3, with a the lone corner and b < c < d the others: (ab, ac, ad).  2, with a < b
 * inside and c < d outside: (ac, ad, bd) and (ac, bd, bc).  The triangles of a case are listed as written or all with their last
 * two vertices swapped, whichever makes the normal point from the inside corners to the outside corners (decided at the edge
 * midpoints in exact arithmetic).  With the case code = sum over the inside v_i of 2^i, they are swapped when bit `code` is
 * set in 0x4D24 for the tetrahedra xyz, yzx, zxy and in 0x32DA for xzy, yxz, zyx.
 * info: cells; valid; inside; cubes = (n[0]-1)(n[1]-1)(n[2]-1); cubes_active; vertices; triangles. */
typedef struct revo_map_mesh_info {      /* 64 bytes, little-endian, no padding */
  uint64_t cells, valid, inside, cubes, cubes_active, vertices, triangles;
  uint64_t reserved;        /* zero */
} revo_map_mesh_info;
/* tsdf: the box's volume (device_tsdf: where it lives; a host volume is uploaded).  vertices: room for cap_vertices vertices of
 * 3 floats, triangles: room for cap_triangles triangles of 3 indices (device_out: where both live).  n_vertices, n_triangles
 * and info (may be NULL) are host pointers.  A counting pass runs first and the call waits for it: REVO_ERR_CAPACITY, with
 * nothing written but the two counts and info, when an output that is not NULL holds fewer than there are.  vertices and
 * triangles both NULL: count only (the caps are ignored); one of them NULL: only the other is written.  The order is the
 * canonical one for host and device outputs alike.  Runs on the context's tracker stream; the map gives the context, the
 * stream and the voxel edge and is not changed.
 * REVO_ERR_INVALID_ARG, with nothing written: NULL m, box, tsdf, n_vertices or n_triangles; the box rules; a flag outside
 * 0 / 1; a device pointer that is not 16-byte aligned. */
int revo_map_tsdf_mesh(revo_map* m, const revo_map_df_box* box, const revo_map_tsdf_cell* tsdf, int device_tsdf, uint32_t min_weight,
                       float* vertices, size_t cap_vertices, uint32_t* triangles, size_t cap_triangles, size_t* n_vertices,
                       size_t* n_triangles, int device_out, revo_map_mesh_info* info);

/* ---- colour and normals on the surface ---------------------------------------------------------------------
 * The colour volume: one 16-byte cell per cell of the TSDF volume's box, with its layout and alignment rules (z fastest, the
 * same place per cell).  A view's colour image is h x w x 3 bytes, B, G, R, rows packed; for a pyramid view it is the
 * pyramid's level-0 BGR plane.  For a cell and a view a colour update takes place exactly when the cell's TSDF update takes
 * place (the TSDF weight was below 2^20, so the update was not dropped) and the class is CONFIRMED:
 *   sum_c += BGR[iv, iu][c] for c = B, G, R;  weight += 1,   (iu, iv) the centre pixel the class rule computed.
 * FREE updates the TSDF cell only.  So color.weight <= tsdf.weight <= 2^20, every sum_c <= 255 * 2^20, nothing overflows.
 * Exact properties: the tsdf bytes, info and view_info equal revo_map_tsdf_fuse's on the same arguments; while nothing
 * saturates the order of the views cannot show in either volume; views A and then an accumulating call with views B leave the
 * bytes of one call with A and B, in both volumes; a call that does not accumulate reads neither volume; for volumes fused
 * only through this entry point color.weight > 0 holds in every cell with tsdf.sum < 0 (a negative sum needs a CONFIRMED
 * update). */
typedef struct revo_map_tsdf_color {       /* 16 bytes */
  uint32_t sum_b, sum_g, sum_r;  /* the sums of the centre pixels' bytes over the cell's colour updates   */
  uint32_t weight;               /* the colour updates, at most the TSDF cell's weight                    */
} revo_map_tsdf_color;
typedef struct revo_map_tsdf_color_info {  /* 32 bytes, little-endian, no padding */
  uint64_t color_updates;   /* the colour updates of this call                              */
  uint64_t cells_colored;   /* cells with color.weight > 0 after the call                   */
  uint64_t reserved[2];     /* zero */
} revo_map_tsdf_color_info;
/* revo_map_tsdf_fuse with the colour volume fused in the same pass.  bgr: n pointers (a host array); bgr[i] is NULL for a
 * pyramid view and the colour image of a raw view, on the side of the depth images (device_in).  color and color_info live where
 * tsdf and info live (device_tsdf); color_info may be NULL.  Every other rule is revo_map_tsdf_fuse's: everything is checked
 * before anything is enqueued, host images (depth and colour) are uploaded to one temporary buffer, the call only enqueues when
 * everything is on the device, device pointers are 16-byte aligned.
 * REVO_ERR_INVALID_ARG, with nothing written, as revo_map_tsdf_fuse and also for a NULL bgr or color and a bgr[i] that does not
 * match its view's kind. */
int revo_map_tsdf_fuse_color(revo_map* m, const revo_map_df_box* box, int n, const revo_map_carve_view* views,
                             const uint8_t* const* bgr, int device_in, const revo_map_tsdf_params* prm,
                             revo_map_tsdf_cell* tsdf, revo_map_tsdf_color* color, int device_tsdf,
                             revo_map_tsdf_info* info, revo_map_tsdf_color_info* color_info,
                             revo_map_carve_view_info* view_info);

/* revo_map_tsdf_mesh with two arrays per vertex, each a pure function of the two volumes' bytes, the box, the voxel edge and
 * min_weight.  Vertices and triangles are byte for byte revo_map_tsdf_mesh's, in its order; the counting, capacity and NULL
 * rules are its rules (normals and colors hold cap_vertices entries; each may be NULL and is then not written; all four
 * outputs NULL: count only).  color may be NULL when colors is NULL; colors != NULL with color == NULL is an argument error.
 * The vertex sits on the edge from the cell c0 to c1 with the parameter a.  Every float32 operation is rounded on its own.
 * Normal (3 floats): f(c) = (float)sum / (float)weight.  The gradient at a cell, per axis i, with VALID as the mesh defines it
 * and a cell outside the box not valid: both c +- e_i valid: (f(c+e_i) - f(c-e_i)) * 0.5f; only c+e_i: f(c+e_i) - f(c); only
 * c-e_i: f(c) - f(c-e_i); neither: 0.0f.  g_i = g0_i + a * (g1_i - g0_i); l2 = (g_x*g_x + g_y*g_y) + g_z*g_z;
 * n_i = g_i / sqrtf(l2), square root and division correctly rounded; (0, 0, 0) when l2 is 0 or not finite.  The field is
 * positive outside, so the normal points from inside to outside, as the triangles' normals do.
 * Colour (4 bytes B, G, R, k): k is the number of the edge's end cells with color.weight > 0.  Per channel
 * m(c) = (float)sum_c / (float)weight; k = 2: v = m0 + a * (m1 - m0); k = 1: the coloured end's m; k = 0: v = 0; the byte is
 * (uint8_t)rintf(fminf(fmaxf(v, 0.0f), 255.0f)). */
int revo_map_tsdf_mesh_attr(revo_map* m, const revo_map_df_box* box, const revo_map_tsdf_cell* tsdf,
                            const revo_map_tsdf_color* color, int device_tsdf, uint32_t min_weight,
                            float* vertices, float* normals, uint8_t* colors, size_t cap_vertices,
                            uint32_t* triangles, size_t cap_triangles, size_t* n_vertices, size_t* n_triangles,
                            int device_out, revo_map_mesh_info* info);

/* ---- views of the surface: depth, normal and colour images ray-cast from the TSDF volume ---------------------
 * One thread marches one ray alone through the fused field in steps of camera depth; a surface is the sign change between two
 * neighbouring samples, found with sub-voxel accuracy from the trilinear interpolant.  No atomic decides an output, so a view's
 * images are a pure function of the two volumes' bytes, the box, the voxel edge, the view and the parameters: the same bytes
 * whatever the launch, the other views of the call, or the side the volumes live on.
 * All arithmetic is float32 with every operation rounded on its own; a / b is the correctly rounded quotient, sqrtf too.
 *
 * Rays.  A view is a revo_map_view with revo_map_render's rules and all-zero defaults; splat_max and min_count are not read.
 * Pixel (x, y) casts revo_map_raycast's ray: dcx = ((float)x - cx)/fx, dcy = ((float)y - cy)/fy,
 * d_i = ((R_i0*dcx) + (R_i1*dcy)) + R_i2 (R the rotation of T_w_c), o = the translation of T_w_c: the parameter is camera depth.
 * Samples.  Sample k = 0, 1, ... sits at s_k = zmin + (float)k * step, computed from the integer and never accumulated.  The
 * march visits the samples in order, starting with "no previous sample":
 *  1. if k == max_steps the ray is EXHAUSTED;
 *  2. if !(s_k < zmax) the ray is a RANGE miss;
 *  3. the sample's place in the box: g_i = o_i + s_k*d_i, u_i = g_i / voxel - ((float)lo_i + 0.5f) (cell centres sit at
 *     integers), b_i = floorf(u_i), r_i = u_i - b_i;
 *  4. the sample is VALID when every u_i is finite with 0 <= b_i <= n_i - 2 and all eight cells b + {0,1}^3 are valid by the
 *     mesh's rule, weight >= max(min_weight, 1).  A box with an axis of 1 has no valid sample;
 *  5. for a valid sample f(c) = (float)sum / (float)weight at the eight cells, written f(dx, dy, dz).  L(x0, x1, a) =
 *     x0 + a*(x1 - x0).  A value at the eight corners is interpolated along z first, then y, then x:
 *     T(v) = L(L(L(v000, v001, r_z), L(v010, v011, r_z), r_y), L(L(v100, v101, r_z), L(v110, v111, r_z), r_y), r_x); F = T(f).
 *     G is the interpolant's own gradient, in field units per cell: G_x interpolates the four differences f(1,y,z) - f(0,y,z)
 *     along z with r_z, then along y with r_y; G_y the four f(x,1,z) - f(x,0,z) along z with r_z, then along x with r_x; G_z
 *     the four f(x,y,1) - f(x,y,0) along y with r_y, then along x with r_x;
 *  6. the decision, from this sample and the previous one: an invalid sample forgets the previous one (a surface is never
 *     found across unknown space); a valid sample behind a valid previous sample with Fp >= 0 and F < 0 is a HIT (inside is
 *     F < 0, as the mesh has it); with Fp < 0 and F >= 0 it ends the ray as BACKFACE (a surface seen from behind is not
 *     shown); otherwise the sample becomes the previous one.
 * A hit is computed from the two samples alone: a = Fp / (Fp - F); depth = s_{k-1} + a*step; the normal is the unit vector of
 * g_i = L(Gp_i, G_i, a) exactly as revo_map_tsdf_mesh_attr normalises (l2 = (g_x*g_x + g_y*g_y) + g_z*g_z, n_i = g_i / sqrtf(l2),
 * (0, 0, 0) when l2 is 0 or not finite): in the world frame, pointing from inside to outside.  A sample's colour cell is its
 * nearest corner b_i + (r_i >= 0.5f ? 1 : 0); the pixel's B, G, R are revo_map_tsdf_mesh_attr's bytes over the two samples'
 * colour cells with a, the previous sample as the lower end; k counts the two cells with color.weight > 0, and k = 0 gives
 * 0, 0, 0.  A miss: depth 0, normal (0, 0, 0), BGR 0. */
typedef struct revo_map_tsdf_ray_params {  /* 16 bytes; NULL: the defaults */
  float step;               /* metres of camera depth between samples; 0: the map's voxel edge; else finite and > 0 */
  uint32_t min_weight;      /* the views a cell needs, as revo_map_tsdf_mesh's; 0 counts as 1 */
  uint32_t max_steps;       /* 1 .. 2^20: the samples of a ray at most; 0: 4096 */
  uint32_t reserved;        /* zero */
} revo_map_tsdf_ray_params;
#define REVO_TSDF_RAY_HIT 0u
#define REVO_TSDF_RAY_RANGE 1u
#define REVO_TSDF_RAY_BACKFACE 2u
#define REVO_TSDF_RAY_EXHAUSTED 3u
typedef struct revo_map_tsdf_ray_info {    /* 64 bytes, little-endian, no padding: integer sums over the rays of a call */
  uint64_t rays, hits, range, backface, exhausted;  /* rays = the sum of the four statuses */
  uint64_t samples;         /* the samples of the march above whose place was formed (step 3): k + 1 for a ray that sample k
                               ended (HIT, BACKFACE), k for a RANGE miss at sample k, max_steps for an EXHAUSTED ray -- not the
                               samples a kernel happened to evaluate */
  uint64_t uncolored;       /* the hits with k = 0; 0 when color is NULL */
  uint64_t reserved;        /* zero */
} revo_map_tsdf_ray_info;
/* n views (1 .. 64, sizes may differ) of the surface in the volumes of `box` (revo_map_distance_field's box rules; tsdf a
 * revo_map_tsdf_cell and color a revo_map_tsdf_color volume with revo_map_tsdf_mesh_attr's layout; device_tsdf: where both
 * live, a host volume is uploaded).  m gives the context, the tracker stream and the voxel edge and is not changed; its voxels
 * play no part.  color may be NULL when bgr is NULL; it is then not read.  Two launches on the tracker stream: one over the
 * cells that marks the 8 x 8 x 8 blocks of sample bases near an inside cell, one that marches a ray per pixel and looks a
 * sample's eight cells up only where that can decide the ray -- the outputs are those of the march above, byte for byte.
 * depth[i] (h x w floats) is required; normal (h x w x 3 floats per view), bgr (h x w x 3 bytes per view, B, G, R), hits (n
 * entries: the hit pixels of each view) and info (one record for the call) may be NULL, and normal[i] / bgr[i] follow their
 * array.  device_out = 0: host pointers, the call waits.  device_out = 1: device pointers (every output, hits and info
 * included, 16-byte aligned); with a device volume the call only enqueues.
 * REVO_ERR_INVALID_ARG, before anything is enqueued and with nothing written: NULL m, box, tsdf, views or depth, a NULL
 * depth[i], normal[i] or bgr[i] of a given array; the box rules; n outside 1 .. 64; revo_map_render's view rules (size, pose,
 * intrinsics, depth range); a step that is not finite or is negative; max_steps above 2^20; a reserved word that is not 0; a
 * flag outside 0 / 1; a misaligned device pointer (volumes included); bgr without color. */
int revo_map_tsdf_raycast(revo_map* m, const revo_map_df_box* box, const revo_map_tsdf_cell* tsdf, const revo_map_tsdf_color* color,
                          int device_tsdf, int n, const revo_map_view* views, const revo_map_tsdf_ray_params* prm,
                          float* const* depth, float* const* normal, uint8_t* const* bgr, uint32_t* hits, int device_out,
                          revo_map_tsdf_ray_info* info);

/* ---- tracking a depth frame against the surface ----------------------------------------------------------------
 * Frame-to-model tracking: every pixel of a depth image is back-projected, moved by a candidate pose and looked up in the fused
 * field, whose value there is the signed distance to the surface and whose interpolant's gradient is its direction.  No cloud is
 * extracted, uploaded or searched, and no distance field is rebuilt: the TSDF is the model as it stands.
 * All arithmetic is float32 with every operation rounded on its own; a / b is the correctly rounded quotient.  No atomic decides
 * an output.
 *
 * The record of one pose.  m, box, tsdf, device_tsdf: revo_map_tsdf_raycast's volume arguments with its rules (m gives the voxel
 * edge v, the context and the stream); trunc: the volume's truncation distance in metres.  frame: one revo_map_carve_view with
 * every rule of revo_map_carve_eval (kf: a pyramid's level-0 depth plane with the context's camera and range; or a raw depth
 * image with its size and either six zeros or its own intrinsics and range); its T_w_c is NOT read.  Pose: T_w_c, R column-major
 * and t.  Per pixel (x, y) with x % stride == 0 and y % stride == 0:
 *   D = depth[y*w + x]; the pixel is SKIPPED unless D is finite, > zmin and < zmax (the carve rule);
 *   dcx = ((float)x - cx)/fx, dcy = ((float)y - cy)/fy;  pc = (dcx*D, dcy*D, D);
 *   p'_i = ((R_i0*pcx + R_i1*pcy) + R_i2*pcz) + t_i;
 *   the place: u_i = p'_i / v - ((float)lo_i + 0.5f), b_i = floorf(u_i), r_i = u_i - b_i (revo_map_tsdf_raycast's step 3 with
 *         g_i = p'_i); the pixel is SKIPPED unless every u_i is finite with 0 <= b_i <= n_i - 2 and the eight cells b + {0,1}^3
 *         are valid, weight >= max(min_weight, 1); then F and G are revo_map_tsdf_raycast's step 5;
 *   kq = trunc / 1024.0f;  e = F*kq, the signed residual in metres (positive in front of the surface);
 *   g_i = (G_i*kq) / v, dimensionless: the exact derivative of the interpolant;
 *   the pixel is accepted iff fabsf(e) <= max_dist (inclusive), otherwise GATED (the gated count is considered - matched -
 *         skipped).
 * Per accepted pixel, with u = p' - centre:  a = u x g, J = (g, a) and the 28 terms S[0..20] J_i*J_j (i <= j, row by row),
 * S[21..26] J_i*e, S[27] e*e exactly as revo_map_df_align_eval forms them.  Each S is the float nearest the exact sum of its float
 * terms (double-double from the first addition, rounded once; DESIGN 4.1's midpoint caveat applies).  The counts are exact. */
typedef struct revo_map_tsdf_track_info {   /* 208 bytes, little-endian, no padding holes: revo_map_df_align_info's layout */
  float    S[28];
  uint64_t matched;      /* accepted pixels                                                                            */
  uint64_t considered;   /* the pixels the stride visits: ceil(w / stride) * ceil(h / stride)                          */
  uint64_t skipped;      /* pixels without a usable depth, outside the interpolation cells, or next to an invalid cell */
  float    centre[3], max_dist;  /* the parameters the call ran with (max_dist after its default)                      */
  float    R[9], T[3];   /* the pose the sums were taken at (R column-major), as given                                 */
  int32_t  flags;        /* bit0: the pose is not finite or its rotation not orthogonal (revo_map_align_eval's rule):
                            everything else is then zero except pose, centre, max_dist                                 */
  int32_t  reserved;     /* zero */
} revo_map_tsdf_track_info;
typedef struct revo_map_tsdf_track_params {  /* 32 bytes; NULL: the defaults and centre 0 */
  float    max_dist;     /* metres; 0: trunc / 2; else finite, 0 < max_dist <= trunc */
  uint32_t stride;       /* 1 .. 8; 0: 1 */
  uint32_t min_weight;   /* the views a cell needs; 0 counts as 1 */
  float    centre[3];    /* finite: the rotation centre of J */
  uint32_t reserved[2];  /* zero */
} revo_map_tsdf_track_params;

/* One record per pose (nposes 1 .. 4096, 4x4 column-major T_w_c), all poses in ONE launch on m's context's tracker stream; for
 * a pyramid frame behind that pyramid's build.  device_in: where a raw depth image lives (a device pointer 4-byte aligned);
 * device_out: where out lives (a device pointer 16-byte aligned); a device volume is 16-byte aligned.  A host volume and a host
 * image are uploaded into the handle's buffers.  The call only enqueues when volume, frame and output are all on the device (a
 * pyramid frame is), and waits otherwise.  The map is not read or changed.
 * REVO_ERR_INVALID_ARG, before anything is enqueued and with nothing written: a NULL m, box, tsdf, frame, poses or out; the box
 * rules; revo_map_carve_eval's view rules except those of T_w_c; nposes out of range; a trunc that is not finite or not > 0; a
 * max_dist that is not finite, negative or above trunc; a stride above 8; a centre that is not finite; a reserved word that is
 * not 0; a flag outside 0 / 1; a misaligned device pointer. */
int revo_map_tsdf_track_eval(revo_map* m, const revo_map_df_box* box, const revo_map_tsdf_cell* tsdf, int device_tsdf, float trunc,
                             const revo_map_carve_view* frame, int device_in, int nposes, const float* T_w_c_n16,
                             const revo_map_tsdf_track_params* prm, revo_map_tsdf_track_info* out, int device_out);

/* Host only.  revo_map_df_align_system's arithmetic: e(x) ~ e + g.v + w.(u x g) = e + J.x, H = sum J J^T from its upper triangle
 * S[0..20], g = S[21..26], cost = S[27].  REVO_ERR_INVALID_ARG: NULL, or flags bit0. */
int revo_map_tsdf_track_system(const revo_map_tsdf_track_info* info, double H[36], double g[6]);

/* revo_map_align's Gauss-Newton loop over revo_map_tsdf_track_eval's records: the same options, Cholesky and pivot rule, update
 * T <- Tr(c) exp(x) Tr(-c) T, stopping rule and statuses; info_out from one more evaluation.  A host volume and a host image are
 * uploaded once per call.  The call waits.  REVO_ERR_INVALID_ARG: as revo_map_tsdf_track_eval, a T_init that is not finite,
 * max_iters < 1. */
int revo_map_tsdf_track(revo_map* m, const revo_map_df_box* box, const revo_map_tsdf_cell* tsdf, int device_tsdf, float trunc,
                        const revo_map_carve_view* frame, int device_in, const float T_init[16],
                        const revo_map_tsdf_track_params* prm, const revo_map_align_opts* opt, float T_out[16],
                        revo_map_tsdf_track_info* info_out, int32_t* iterations, int32_t* status);

/* ---- a box that follows the camera: exact shift, spill and refill of the surface volumes -----------------------
 * revo_map_tsdf_fuse, _mesh, _raycast and _track take (box, volume) per call; these two calls move the box.  Everything is an
 * integer that leaves the handle and comes back without loss, in ascending key order, and every output is a pure function of
 * the input bytes.
 *
 * The record of one cell that has left a box: the cell's voxel index as the voxel map's packed key (21 bits per axis biased by
 * 2^20, x highest: revo_map_voxel_raw's key, so ascending keys are ascending places in any box) and the bytes of its two cells;
 * the four colour words are zero without a colour volume.
 * A cell is EMPTY when every byte of its revo_map_tsdf_cell is zero and, with a colour volume, every byte of its
 * revo_map_tsdf_color too (a cell with weight 0 and sum != 0 is not EMPTY).
 * A cell FITS when, decided in 64 bits, weight <= 2^20, |sum| <= 2^30, colour weight <= 2^20 and each colour sum <= 255 * 2^20:
 * what any sequence of fuse calls can leave.
 * Exact properties: (a) revo_map_tsdf_shift by d, then by -d, then revo_map_tsdf_refill of the first shift's records restores the
 * bytes of both volumes, for any bytes that FIT; (b) for d1, d2 with no opposite signs on any axis, a shift by d1 followed by one
 * by d2 leaves the destination bytes of one shift by d1 + d2, and the two record lists merged by key are that shift's list;
 * (c) no other call's bytes change. */
typedef struct revo_map_tsdf_record {      /* 32 bytes, little-endian, no padding */
  uint64_t key;                            /* the cell's voxel index, packed                  */
  int32_t  sum;                            /* revo_map_tsdf_cell                              */
  uint32_t weight;
  uint32_t sum_b, sum_g, sum_r;            /* revo_map_tsdf_color; zero without a colour volume */
  uint32_t color_weight;
} revo_map_tsdf_record;
typedef struct revo_map_tsdf_shift_info {  /* 64 bytes, little-endian, no padding */
  uint64_t cells;        /* n[0]*n[1]*n[2]                                                       */
  uint64_t staying;      /* source cells that lie in the destination box                         */
  uint64_t leaving;      /* cells - staying                                                      */
  uint64_t records;      /* leaving cells that are not EMPTY                                     */
  uint64_t dropped;      /* of those, the cells a move without records discarded                 */
  uint64_t reserved[3];  /* zero */
} revo_map_tsdf_shift_info;
/* The volumes of the box (box->lo, box->n) moved out of place into the volumes of the box (box->lo + delta, box->n): the
 * destination cell c' receives the bytes of the source cell c' + delta when that cell lies in the source box (it is STAYING) and
 * zero bytes otherwise; every other source cell is LEAVING, and every leaving cell that is not EMPTY gives one record, in
 * ascending key order, the same bytes for host and device outputs (the order comes from a scan over the leaving cells in place
 * order, never from arrival).  src_color and dst_color: both NULL (the TSDF volume alone) or both given.  device_tsdf: where the
 * four volumes live; device_out: where records lives.  Host volumes are uploaded into the handle's buffers, the result is
 * downloaded and the call waits.  Runs on the context's tracker stream; the map gives the context and the stream and is not changed.
 *   records and n_records given: move and emit.  A counting pass runs first and the call waits for it; when cap_records is below
 *       the count the call returns REVO_ERR_CAPACITY with nothing written but *n_records and info (the destination is untouched).
 *   records NULL, n_records given: count only; the destination is not written (dst_tsdf must still be given).  The call waits.
 *   both NULL: move and drop; the leaving cells are discarded and info->dropped counts those that were not EMPTY.  With device
 *       volumes the call only enqueues.
 * info (may be NULL) is a host pointer whenever the call waits; in the one case that only enqueues (move and drop with device
 * volumes) it is a device pointer, 16-byte aligned.  delta = 0 is a copy without a record; |delta_i| >= n_i on any axis leaves a
 * destination of zeros and every source cell leaving.
 * REVO_ERR_INVALID_ARG, before anything is enqueued and with nothing written: NULL m, box, delta, src_tsdf or dst_tsdf; exactly
 * one of the colour volumes NULL; the box rules of revo_map_distance_field for the source or for the destination box (a
 * destination that leaves the index range included); source and destination byte ranges that overlap (an in-place shift is not
 * offered); records with a NULL n_records; a flag outside 0 / 1; a misaligned device pointer (16 bytes). */
int revo_map_tsdf_shift(revo_map* m, const revo_map_df_box* box, const int32_t delta[3], const revo_map_tsdf_cell* src_tsdf,
                        const revo_map_tsdf_color* src_color, revo_map_tsdf_cell* dst_tsdf, revo_map_tsdf_color* dst_color,
                        int device_tsdf, revo_map_tsdf_record* records, size_t cap_records, size_t* n_records, int device_out,
                        revo_map_tsdf_shift_info* info);

typedef struct revo_map_tsdf_refill_info {  /* 32 bytes, little-endian, no padding */
  uint64_t records;      /* n                                            */
  uint64_t applied;      /* records whose key lies inside the box        */
  uint64_t outside;      /* records - applied: ignored                   */
  uint64_t reserved;     /* zero */
} revo_map_tsdf_refill_info;
/* Every record (n of them, device_in: where they live; n = 0 is valid and changes nothing) whose key lies inside the box is added
 * to its cell: sum += sum, weight += weight, and with a colour volume the four colour words likewise.  Records outside the box
 * are ignored and counted.  The records must be in strictly ascending key order, so keys are unique and no atomic touches a cell.
 * All or nothing, as revo_map_subtract_raw is: a check pass runs first and the call waits for it, then the apply pass is enqueued
 * (a host volume is uploaded, updated, downloaded and the call waits again).  info (may be NULL) is a host pointer.
 * REVO_ERR_INVALID_ARG, with no byte of either volume changed: NULL m, box or tsdf, NULL records with n > 0, n above 2^30; the box
 * rules; a flag outside 0 / 1; a misaligned device pointer (16 bytes); a key that is not ascending or has bit 63 set; a record
 * with a colour word that is not zero when color is NULL; a record inside the box whose cell would not FIT afterwards. */
int revo_map_tsdf_refill(revo_map* m, const revo_map_df_box* box, revo_map_tsdf_cell* tsdf, revo_map_tsdf_color* color, int device_tsdf,
                         size_t n, const revo_map_tsdf_record* records, int device_in, revo_map_tsdf_refill_info* info);

/* ---- views taken out of the surface again: the exact inverse of the fuse ----------------------------------------
 * A cell is sum += q, weight += 1 with q an integer that is a pure function of the cell, the view and trunc, and colour is the
 * same with the centre pixel's bytes; so a view that was fused can be taken out again exactly, as revo_map_subtract_raw takes
 * out what revo_map_merge_raw put in.
 * Per cell and view the class, the centre pixel and q are exactly revo_map_tsdf_fuse's (FREE: q = 1024; CONFIRMED: its rounded
 * quotient; every other class: no update).  An update is sum -= q, weight -= 1; for a CONFIRMED update with a colour volume the
 * three colour sums lose the centre pixel's bytes and color.weight -= 1.
 * The call is all or nothing.  Per cell let k be the views of this call that update the cell and kc the CONFIRMED ones among
 * them, Q the sum of their q and B, G, R the sums of their pixels' bytes.  A cell with k == 0 is not looked at.  A cell with
 * k > 0 FITS when, decided in 64-bit integers,
 *   weight < 2^20                      (a full cell may have dropped updates: its history cannot be inverted)
 *   weight >= k                        (no more views leave than came)
 *   |sum - Q| <= 1024 * (weight - k)   (an emptied cell has sum 0; the cell stays a state a fuse can reach)
 * and with a colour volume
 *   color.weight >= kc,  sum_c >= C for c = B, G, R               (nothing goes below zero)
 *   color.weight - kc <= weight - k                               (the colour weight never passes the TSDF weight)
 *   sum_c - C <= 255 * (color.weight - kc) for c = B, G, R        (an emptied colour cell has sums 0).
 * If any cell does not fit the call returns REVO_ERR_INVALID_ARG and no byte of either volume has changed, in host or device
 * memory; info->misfits is the number of such cells, updates and color_updates are 0 and the other counters describe the
 * volumes as they stand.  Otherwise every update is applied.
 * Exact properties: while nothing saturated, fusing the views A and B in any order and any split into accumulating calls and
 * then taking out B in any split leaves the bytes of fusing A alone, in both volumes; taking out everything leaves all-zero
 * volumes; taking out B1 and then B2 equals taking out B1 and B2 in one call when each step fits; a host volume and a device
 * volume give the same bytes; a pyramid view and the raw view of its level-0 planes give the same bytes; view_info is byte for
 * byte revo_map_tsdf_fuse's for the same views, refused or not. */
typedef struct revo_map_tsdf_unfuse_info {  /* 64 bytes, little-endian, no padding */
  uint64_t cells;           /* n[0]*n[1]*n[2]                                                */
  uint64_t updates;         /* the updates taken out                                         */
  uint64_t cells_weighted;  /* cells with weight > 0 after the call                          */
  uint64_t cells_inside;    /* of those, the cells with sum < 0                              */
  uint64_t misfits;         /* cells with k > 0 that do not FIT: the call changed nothing    */
  uint64_t color_updates;   /* the colour updates taken out                                  */
  uint64_t cells_colored;   /* cells with color.weight > 0 after the call; 0 without color   */
  uint64_t reserved;        /* zero */
} revo_map_tsdf_unfuse_info;
/* n views (1 .. 64) taken out of the volumes of `box`.  The view, box, side and alignment rules are revo_map_tsdf_fuse_color's:
 * bgr[i] is NULL for a pyramid view and the colour image of a raw view, on the side of the depth images (device_in); tsdf, color
 * and view_info (n records, may be NULL) live where device_tsdf says, device pointers 16-byte aligned.  color may be NULL: bgr
 * must then be NULL too and the colour volume is not touched.  trunc: the distance the views were fused with; 0 means 4 x the
 * map's voxel edge.  info (may be NULL) is a host pointer.  A check pass that writes nothing to the volumes runs first and the
 * call waits for its verdict; then the apply pass is enqueued, and the call waits again for a host volume or a given info.
 * Runs on the context's tracker stream, for a pyramid view behind that pyramid's build.
 * REVO_ERR_INVALID_ARG, before anything is enqueued and with nothing written: NULL m, box, views or tsdf; color without bgr or
 * bgr without color; the box rules; n outside 1 .. 64; the view rules; a bgr[i] that does not match its view's kind; a trunc that
 * is not 0 and not finite and > 0; a flag outside 0 / 1; a misaligned device pointer. */
int revo_map_tsdf_unfuse(revo_map* m, const revo_map_df_box* box, int n, const revo_map_carve_view* views,
                         const uint8_t* const* bgr, int device_in, float trunc,
                         revo_map_tsdf_cell* tsdf, revo_map_tsdf_color* color, int device_tsdf,
                         revo_map_tsdf_unfuse_info* info, revo_map_carve_view_info* view_info);

/* ---- surfaces for many sequences at once: batched fuse and track -------------------------------------------------
 * revo_map_tsdf_fuse* and revo_map_tsdf_track* are one volume per call.  These calls take a list of jobs, each with its own
 * volume, box, view or frame and voxel edge, and run all of them in one launch (the Gauss-Newton loop: one launch, one copy and
 * one wait per round for all jobs together).  Every output has an exact specification, the single calls: a job's bytes are the
 * bytes the single call leaves for that job alone.  Everything lives in device memory of m's device; m gives the context, the
 * tracker stream and the scratch, a job's own map (of m's context; NULL: m) gives the job's voxel edge.
 *
 * One fuse job: the view is fused into the job's volumes as revo_map_tsdf_fuse_color (color given) or revo_map_tsdf_fuse (color
 * NULL) does with n = 1, accumulate = 1, device_in = 1 and device_tsdf = 1: the volumes are read and updated. */
typedef struct revo_map_tsdf_fuse_job {  /* 200 bytes, no padding holes */
  revo_map* map;                         /* gives the voxel edge; of m's context; NULL: m                                   */
  revo_map_df_box box;                   /* the box rules of revo_map_distance_field                                          */
  float trunc;                           /* metres; 0: 4 x the job's voxel edge; else finite and > 0                          */
  uint32_t reserved;                     /* zero                                                                              */
  revo_map_tsdf_cell* tsdf;              /* device, 16-byte aligned: n[0]*n[1]*n[2] cells                                     */
  revo_map_tsdf_color* color;            /* device, 16-byte aligned, or NULL: no colour is fused                              */
  revo_map_carve_view view;              /* kf, or a raw depth image in device memory (4-byte aligned); every view rule of    */
                                         /* revo_map_carve_eval                                                               */
  const uint8_t* bgr;                    /* with color: NULL for a pyramid view, the device colour image of a raw view;       */
                                         /* without color: NULL                                                               */
  revo_map_tsdf_info* info;              /* device, 16-byte aligned, or NULL                                                  */
  revo_map_tsdf_color_info* color_info;  /* device, 16-byte aligned, or NULL; NULL without color                              */
  revo_map_carve_view_info* view_info;   /* device, 16-byte aligned, or NULL: one record                                      */
} revo_map_tsdf_fuse_job;
/* n_jobs (1 .. 1024) fuse jobs in ONE launch on m's context's tracker stream, for a pyramid view behind that pyramid's build.
 * The call only enqueues.  After it every job's volumes and records hold exactly the bytes the single call leaves (above); the
 * order of the jobs cannot show.  No atomic touches a cell, so two jobs must not share one.
 * REVO_ERR_INVALID_ARG, the call refused as a whole before anything is enqueued and with no byte written: NULL m or jobs; n_jobs
 * outside 1 .. 1024; in any job: a map of another context, a NULL tsdf, a box, view, bgr, trunc or alignment rule of the single
 * call broken, a reserved word that is not 0, bgr or color_info given without color, a volume or an image that is not in device
 * memory of m's device; two volumes (TSDF or colour, of any two jobs) whose byte ranges overlap. */
int revo_map_tsdf_fuse_many(revo_map* m, int n_jobs, const revo_map_tsdf_fuse_job* jobs);

/* One unfuse job: ONE view taken out of the job's volumes as revo_map_tsdf_unfuse does with n = 1, device_in = 1 and
 * device_tsdf = 1.  The members are revo_map_tsdf_fuse_job's with the unfuse's meaning; several views of one volume stay the
 * single call's business. */
typedef struct revo_map_tsdf_unfuse_job {  /* 192 bytes, no padding holes */
  revo_map* map;                         /* offset   0: gives the voxel edge; of m's context; NULL: m                        */
  revo_map_df_box box;                   /* offset   8: the box rules of revo_map_distance_field                             */
  float trunc;                           /* offset  32: what the view was fused with; 0: 4 x the job's voxel edge            */
  uint32_t reserved;                     /* offset  36: zero                                                                 */
  revo_map_tsdf_cell* tsdf;              /* offset  40: device, 16-byte aligned                                              */
  revo_map_tsdf_color* color;            /* offset  48: device, 16-byte aligned, or NULL: the colour volume is not touched   */
  revo_map_carve_view view;              /* offset  56: kf, or a raw depth image in device memory (4-byte aligned)           */
  const uint8_t* bgr;                    /* offset 168: with color: NULL for a pyramid view, the device colour image of a    */
                                         /*             raw view; without color: NULL                                        */
  revo_map_tsdf_unfuse_info* info;       /* offset 176: device, 16-byte aligned, or NULL                                     */
  revo_map_carve_view_info* view_info;   /* offset 184: device, 16-byte aligned, or NULL: one record                         */
} revo_map_tsdf_unfuse_job;
typedef struct revo_map_tsdf_unfuse_result {  /* 80 bytes, no padding holes */
  revo_map_tsdf_unfuse_info info;        /* offset  0: the job's info, as the single call gives it (refused or not)          */
  int32_t status;                        /* offset 64: REVO_OK, or REVO_ERR_INVALID_ARG: the job had a misfit and changed    */
                                         /*            nothing, the single call's code for a refusal                         */
  int32_t reserved[3];                   /* offset 68: zero                                                                  */
} revo_map_tsdf_unfuse_result;
/* n_jobs (1 .. 1024) unfuse jobs in TWO launches on m's context's tracker stream (a check pass and an apply pass over all jobs),
 * for a pyramid view behind that pyramid's build.  The verdict stays on the device: the apply pass reads each job's misfit count
 * where the check pass left it, and the blocks of a refused job return at once; there is no host wait between the passes.
 * Per job, the single call:
 *   a job whose cells all FIT leaves the volumes, info and view_info that revo_map_tsdf_unfuse leaves for that job alone;
 *   a job with a misfit changes no byte of its volumes; its info is the single call's refused info (misfits counted, updates and
 *   color_updates 0, the other counters describing the volumes as they stand) and its view_info is still the fuse's;
 *   every other job of the call is applied all the same; neither the order of the jobs nor the other jobs show in a job's bytes.
 * results (may be NULL): n_jobs records, in device memory 16-byte aligned (device_out = 1; status is written by the kernel) or in
 * host memory (device_out = 0).  With results == NULL or device_out = 1 the call only enqueues; with host results it waits once,
 * at the end.  The return value is REVO_OK whenever the argument rules hold, even if jobs were refused: a refusal is a per-job
 * result, not a failed call.  No atomic touches a cell, so two jobs must not share a volume.
 * REVO_ERR_INVALID_ARG, the call refused as a whole before anything is enqueued and with no byte written: NULL m or jobs; n_jobs
 * outside 1 .. 1024; in any job: a map of another context, a NULL tsdf, a box, view, bgr, trunc or alignment rule of the single
 * call broken, a reserved word that is not 0, bgr given without color, a volume, an image or a record that is not in device
 * memory of m's device; two volumes (TSDF or colour, of any two jobs) whose byte ranges overlap; device_out outside 0 / 1; device
 * results that are misaligned or not in device memory of m's device. */
int revo_map_tsdf_unfuse_many(revo_map* m, int n_jobs, const revo_map_tsdf_unfuse_job* jobs,
                              revo_map_tsdf_unfuse_result* results, int device_out);

/* One track job: revo_map_tsdf_track_eval's arguments for one volume and one frame (device_tsdf = 1, device_in = 1). */
typedef struct revo_map_tsdf_track_job {  /* 200 bytes, no padding holes */
  revo_map* map;                          /* gives the voxel edge; of m's context; NULL: m                                    */
  revo_map_df_box box;
  float trunc;                            /* the volume's truncation distance in metres: finite and > 0                       */
  int32_t n_poses;                        /* revo_map_tsdf_track_eval_many: the job's poses, >= 1; revo_map_tsdf_track_many: the job's own */
                                          /* max_iters, 0: the options'                                                       */
  const revo_map_tsdf_cell* tsdf;         /* device, 16-byte aligned                                                          */
  revo_map_carve_view frame;              /* kf, or a raw depth image in device memory; its T_w_c is not read                 */
  revo_map_tsdf_track_params prm;         /* all zero: the defaults and centre 0                                              */
  const float* poses;                     /* host: n_poses 4x4 column-major T_w_c (eval_many), or the 16 floats of T_init (track_many) */
} revo_map_tsdf_track_job;
/* The records of all jobs, job after job (job j's records start behind those of the jobs before it), from ONE launch for all
 * poses of all jobs: at most 4096 poses in total.  A job's records are the bytes revo_map_tsdf_track_eval gives for that job
 * alone, the flags-bit-0 record of a pose that is not finite or not orthogonal included.  Frames may differ in size and stride.
 * out: device memory 16-byte aligned (device_out = 1, the call only enqueues) or host memory (0, the call waits).
 * REVO_ERR_INVALID_ARG, before anything is enqueued and with nothing written: NULL m, jobs or out; n_jobs outside 1 .. 1024; in
 * any job every rule of revo_map_tsdf_track_eval, n_poses < 1, NULL poses, a map of another context, a volume or an image that is
 * not in device memory of m's device; more than 4096 poses in total; device_out outside 0 / 1; a misaligned device output. */
int revo_map_tsdf_track_eval_many(revo_map* m, int n_jobs, const revo_map_tsdf_track_job* jobs, revo_map_tsdf_track_info* out,
                                  int device_out);

typedef struct revo_map_tsdf_track_result {  /* 288 bytes, no padding holes */
  float T[16];                     /* revo_map_tsdf_track's T_out                                  */
  revo_map_tsdf_track_info info;   /* ... info_out                                                 */
  int32_t iterations, status;      /* ... iterations and status                                    */
  int32_t evaluations;             /* the records the job's loop took: iterations + 1, or + 2 for REVO_ALIGN_LOST */
  int32_t reserved;                /* zero */
} revo_map_tsdf_track_result;
/* revo_map_tsdf_track's Gauss-Newton loop for all jobs (1 .. 1024) in lockstep from each job's T_init (poses); opt: one set of
 * options for all jobs (NULL: revo_map_tsdf_track's defaults; a job's n_poses > 0 is that job's max_iters instead).  A round evaluates, in one launch, the current pose of every job
 * that still needs an evaluation (the closing evaluation that gives info counts as one), copies those records once, waits once
 * and advances each job on the host.  Per job T, info, iterations and status are exactly revo_map_tsdf_track's for that job
 * alone.  *rounds (may be NULL): the rounds taken, which is the largest `evaluations` of any job.  results: host memory, n_jobs
 * records.  The call waits.
 * REVO_ERR_INVALID_ARG, before anything is enqueued and with nothing written: as revo_map_tsdf_track_eval_many without the
 * output's rules; NULL results; a T_init that is not finite; max_iters < 1; a job's n_poses < 0. */
int revo_map_tsdf_track_many(revo_map* m, int n_jobs, const revo_map_tsdf_track_job* jobs, const revo_map_align_opts* opt,
                             revo_map_tsdf_track_result* results, int32_t* rounds);

/* One ray-cast job: revo_map_tsdf_raycast's arguments for one volume, with device_tsdf = 1 and device_out = 1.  The
 * volumes are only read, so, unlike the fuse, several jobs may name one volume: that is how a caller gets more than 64 views
 * of a volume in one call. */
typedef struct revo_map_tsdf_ray_job {   /* 120 bytes, no padding holes */
  revo_map* map;                         /* offset   0: gives the voxel edge; of m's context; NULL: m                        */
  revo_map_df_box box;                   /* offset   8: the box rules of revo_map_distance_field                             */
  revo_map_tsdf_ray_params prm;          /* offset  32: by value; all zero: the defaults                                     */
  const revo_map_tsdf_cell* tsdf;        /* offset  48: device, 16-byte aligned: n[0]*n[1]*n[2] cells                        */
  const revo_map_tsdf_color* color;      /* offset  56: device, 16-byte aligned, or NULL: no colour is read                  */
  int32_t n_views;                       /* offset  64: 1 .. 64                                                              */
  uint32_t reserved;                     /* offset  68: zero                                                                 */
  const revo_map_view* views;            /* offset  72: host array of n_views views, revo_map_tsdf_raycast's view rules      */
  float* const* depth;                   /* offset  80: host array of n_views device pointers, each 16-byte aligned           */
  float* const* normal;                  /* offset  88: likewise, or NULL: no normal images                                  */
  uint8_t* const* bgr;                   /* offset  96: likewise, or NULL: no colour images; needs color                     */
  uint32_t* hits;                        /* offset 104: device, 16-byte aligned, n_views words, or NULL                      */
  revo_map_tsdf_ray_info* info;          /* offset 112: device, 16-byte aligned, one record for the job, or NULL             */
} revo_map_tsdf_ray_job;
/* n_jobs (1 .. 1024) ray-cast jobs with at most 4096 views between them, on m's context's tracker stream: one memset, one launch
 * that marks the block masks of the call's distinct volumes, one launch that marches every view of every job, and one small
 * launch that hands every job its counters.  The call only enqueues and never waits.  After it every job's images, hits and info
 * hold exactly the bytes revo_map_tsdf_raycast leaves for that job alone (device_tsdf = 1, device_out = 1); neither the order of
 * the jobs nor the other jobs show in them.  The block mask is built once per distinct (tsdf pointer, box, effective min_weight)
 * of the call, not once per job.  REVO_MAP_TSDF_RAY_MASK=0 selects the plain march, as in the single call.
 * REVO_ERR_INVALID_ARG, the call refused as a whole before anything is enqueued and with no byte written: NULL m or jobs; n_jobs
 * outside 1 .. 1024; more than 4096 views; in any job: a map of another context, a NULL tsdf, views or depth, n_views outside
 * 1 .. 64, a box, view, parameter or alignment rule of the single call broken, a NULL depth[i], normal[i] or bgr[i] of a given
 * array, bgr without color, a reserved word that is not 0, a volume, an image or a record that is not in device memory of m's
 * device; two outputs (images, hits, info, of any two views or jobs) whose byte ranges overlap; an output that overlaps a volume
 * of the call. */
int revo_map_tsdf_raycast_many(revo_map* m, int n_jobs, const revo_map_tsdf_ray_job* jobs);

/* A surface for a stream of revo_vo_multi: the caller-owned device volumes of a box, fused from every keyframe the stream
 * promotes from now on, in the step, right behind the batched map integration of the step's promoted keyframes. */
typedef struct revo_vo_multi_surface {  /* 120 bytes, no padding holes */
  revo_map* map;                        /* gives the voxel edge; of the handle's context                            */
  revo_map_df_box box;
  float trunc;                          /* metres; 0: 4 voxel edges                                                 */
  int32_t track;                        /* 0 / 1: each keyframe is tracked against the surface before it is fused   */
  revo_map_tsdf_cell* tsdf;             /* device, 16-byte aligned; they outlive the attachment                     */
  revo_map_tsdf_color* color;           /* or NULL                                                                  */
  revo_map_tsdf_track_params track_prm; /* read with track                                                          */
  revo_map_align_opts track_opts;       /* read with track; max_iters 0: revo_map_tsdf_track's defaults             */
} revo_vo_multi_surface;
typedef struct revo_vo_multi_surface_report {  /* 408 bytes, no padding holes: a stream's last keyframe */
  double timestamp;
  float T_w_kf[16];                     /* the keyframe's pose as the tracker has it: the trajectory's and the map's    */
  float T_fused[16];                    /* the pose it was fused at: the refined pose of a CONVERGED track, else T_w_kf */
  revo_map_tsdf_track_info track;       /* with tracked: revo_map_tsdf_track's info_out; else zero                      */
  int32_t iterations, status;           /* revo_map_tsdf_track's; REVO_ALIGN_LOST without a track                       */
  int32_t tracked;                      /* 1: the loop ran (track on and T_w_kf passes the orthogonality rule)          */
  int32_t fused;                        /* 1: the keyframe was fused; 0: T_fused fails the rule (or the call failed)    */
  revo_map_carve_view_info view_info;   /* of the fuse; zero when not fused                                             */
  uint64_t keyframes_fused, keyframes_skipped;  /* running counts since the surface was attached                        */
} revo_vo_multi_surface_report;
/* s == NULL detaches; revo_vo_multi_reset detaches.  In revo_vo_multi_step every promoted keyframe whose stream has a surface is
 * handled as the sequential driver handles it: with track, one revo_map_tsdf_track_many over those keyframes against their
 * volumes as they stand, from T_w_kf (a T_w_kf that fails revo_map_align_eval's orthogonality rule is not tracked); the fuse pose
 * is the refined pose where the status is REVO_ALIGN_CONVERGED and T_w_kf otherwise; a keyframe whose fuse pose fails the rule is
 * not fused and is counted; then one revo_map_tsdf_fuse_many over the rest.  A step never fails for a surface, as it never fails
 * for a map; the reported trajectory and the map integration keep T_w_kf.  Without a surface on any promoted stream nothing is
 * enqueued.
 * REVO_ERR_INVALID_ARG: a stream out of range; a map of another context or NULL; the box, trunc, alignment or parameter rules of
 * revo_map_tsdf_fuse_many and revo_map_tsdf_track_many; track outside 0 / 1; volumes that are not in device memory. */
int revo_vo_multi_attach_surface(revo_vo_multi* mv, int stream, const revo_vo_multi_surface* s);
/* The report of the stream's last keyframe since the surface was attached; waits for that step's fuse.
 * REVO_ERR_INVALID_ARG: a bad stream or NULL out, no surface attached, or no keyframe since it was. */
int revo_vo_multi_surface_last(revo_vo_multi* mv, int stream, revo_vo_multi_surface_report* out);

/* A bounded surface for a stream: with window = N (1 .. 1024) the stream's volumes hold its last N fused keyframes;
 * 0, the default of every attachment, switches the window off and the surface only grows.  Valid after
 * revo_vo_multi_attach_surface; setting it (also to the value it has) starts an empty window: views held so far are forgotten and
 * stay in the volumes.  With a window the step does two more things behind its revo_map_tsdf_fuse_many:
 *   keep   for every keyframe it fused, what names the view again -- device copies of the keyframe slot's level-0 depth plane and
 *          colour image ((4 + 3) bytes per pixel; no colour image without a colour volume) and T_fused -- enqueued on the tracker
 *          stream where the fuse is; a window's N + 1 slots are allocated when first used.  A keyframe that was skipped is not held;
 *   evict  for every stream that now holds more than its window, the oldest view is taken out with ONE
 *          revo_map_tsdf_unfuse_many over all such streams, as the raw view of the kept copies (which gives the bytes of the
 *          pyramid view it was fused as); each job's info goes to a device record of its stream, and nothing waits.
 * A step still never fails for a surface.  The host rotates the window without knowing the device's verdict: an eviction the
 * device refuses FORGETS the view and leaves it in the volumes.  That can happen only for volumes that were attached pre-filled
 * (so that a cell's state is one no fuse of the held views reaches) or that hold a cell at the full weight 2^20;
 * revo_vo_multi_surface_window_last reports it.  With track = 1 keyframes are tracked against the windowed surface as it stands.
 * Detaching the surface, revo_vo_multi_reset and revo_vo_multi_destroy free the window.
 * REVO_ERR_INVALID_ARG: a stream out of range; no surface attached; window outside 0 .. 1024. */
int revo_vo_multi_surface_window(revo_vo_multi* mv, int stream, int window);
typedef struct revo_vo_multi_surface_window_report {  /* 104 bytes, no padding holes */
  int32_t window;                       /* offset  0: the window's size                                                     */
  int32_t held;                         /* offset  4: the views held, <= window                                             */
  uint64_t evictions;                   /* offset  8: the views that have left the window since it was set                  */
  double evicted_timestamp;             /* offset 16: the keyframe time stamp of the last one; 0 without an eviction        */
  revo_map_tsdf_unfuse_result evicted;  /* offset 24: its info as revo_map_tsdf_unfuse_many left it on the device, and its  */
                                        /*            status by that call's rule: REVO_ERR_INVALID_ARG when misfits != 0,   */
                                        /*            the view then stayed in the volumes; zero without an eviction         */
} revo_vo_multi_surface_window_report;
/* The stream's window as it stands; waits for the step's work on the tracker stream when there has been an eviction.
 * REVO_ERR_INVALID_ARG: a bad stream or NULL out, no surface attached, or no window set. */
int revo_vo_multi_surface_window_last(revo_vo_multi* mv, int stream, revo_vo_multi_surface_window_report* out);

/* ---------------------------------------------------------------------------
 * PNG decoding on the device: replaces the cv::imread(IMREAD_COLOR) / cv::imread(IMREAD_UNCHANGED) of the TUM front-end
 * (iowrapperRGBD.cpp:257-333) for the multi-stream driver.  Inflate (zlib, RFC 1950/1951: stored, fixed and dynamic blocks,
 * Adler-32 checked) runs one wave64 per image; the row filters (None, Sub, Up, Average, Paeth) are undone in a second
 * kernel that writes the caller's layout.  Throughput comes from many images per launch: one image is a serial decode.
 * ------------------------------------------------------------------------- */
typedef struct revo_png_info {
  int32_t width, height, bit_depth, color_type, interlace;
  uint64_t idat_bytes;  /* the zlib stream: all IDAT payloads together */
  uint64_t raw_bytes;   /* its inflated size: height * (1 + row bytes) */
} revo_png_info;
/* Host only, never touches a device: checks the signature, every chunk's CRC and the IHDR, skips ancillary chunks and
 * reports the layout.  REVO_ERR_CORRUPT: malformed (bad signature or CRC, no IHDR / IEND / IDAT, zero size, bad IHDR
 * fields).  REVO_ERR_UNSUPPORTED (info still filled): interlaced, palette, bit depth < 8, 16-bit colour, an unknown critical
 * chunk -- the caller decodes those on the CPU. */
int revo_png_probe(const uint8_t* png, size_t len, revo_png_info* out);

enum { REVO_PNG_BGR8 = 0, /* [H][W][3] u8 B,G,R: cv::imread(IMREAD_COLOR).  From RGB8 (swapped), RGBA8 (alpha dropped),
                             gray8 and gray+alpha 8 (gray replicated) */
       REVO_PNG_U16 = 1   /* [H][W] u16, native order: cv::imread(IMREAD_UNCHANGED) of a depth map.  From gray16 (big-endian
                             in the file) or gray8 (zero-extended) */ };
typedef struct revo_png_decoder revo_png_decoder;
/* ctx: the device to decode on (NULL: the calling thread's current device).  Capacity: max_images files per submit,
 * max_compressed_bytes of image data per submit (page-locked host + device), max_raw_bytes_per_image of inflated rows per
 * image (device scratch: max_images of them).  Rows of at most 8192 bytes (e.g. 2048 RGBA pixels). */
int revo_png_decoder_create(revo_ctx* ctx, int max_images, size_t max_compressed_bytes, size_t max_raw_bytes_per_image,
                            revo_png_decoder** out);
void revo_png_decoder_destroy(revo_png_decoder* d);
typedef struct revo_png_job {
  const uint8_t* png; size_t len;  /* host bytes of one file; reusable once revo_png_decode_submit returns */
  int32_t format;                  /* REVO_PNG_BGR8 | REVO_PNG_U16 */
  int32_t width, height;           /* expected; a mismatch is that image's REVO_ERR_INVALID_ARG */
  void* d_dst; size_t dst_stride;  /* device rows the image is written to */
} revo_png_job;
/* Parses on the host, packs the image data of all n files into one page-locked slab, issues ONE host-to-device copy and
 * the decode kernels on `stream`, and returns.  REVO_ERR_CAPACITY: the batch exceeds the decoder's capacity, or two
 * tickets are outstanding.  A failed image never affects another; its destination rows are then undefined. */
int revo_png_decode_submit(revo_png_decoder* d, int n, const revo_png_job* jobs, void* stream, uint64_t* ticket);
/* Waits for a ticket and writes its n per-image codes: REVO_OK, REVO_ERR_CORRUPT, REVO_ERR_UNSUPPORTED, REVO_ERR_INVALID_ARG
 * (size mismatch). */
int revo_png_decode_wait(revo_png_decoder* d, uint64_t ticket, int32_t* status);

/* ---------------------------------------------------------------------------
 * Diagnostics for bench.py and profiles/, not a stable interface: names, arguments and meaning may change in any release.
 * ------------------------------------------------------------------------- */
/* out3 = {workgroups of the tracker grids that have started, resident gates that gave up waiting, workgroups enqueued}
 * on `device`; after hipDeviceSynchronize the first equals the third in a healthy process.  -1: no tracker launch yet. */
int revo_debug_census_(int device, unsigned out3[3]);
/* how many resident gates of `device` gave up waiting so far (0 in a healthy process); -1: no tracker launch yet */
int revo_debug_gate_timeouts_(int device);
/* the longest time (ns) each of 12 sections of a frame submission has taken so far; reset != 0 clears them after reading */
void revo_debug_section_max_(unsigned long long out[12], int reset);
/* out = {waits for a device result, waits that fell back to a blocking synchronise, longest wait in ns} */
void revo_debug_wait_stats_(unsigned long long out[3]);
/* builds with -DREVO_TRACK_PROFILE: the phase cycle counters of the context's last single-pair tracker launch */
int revo_debug_track_profile_(revo_ctx* ctx, float out13[13]);
/* builds with -DREVO_TRACK_PROFILE: 64 floats of cycle counters per pair of the last batch tracker launch */
int revo_debug_batch_profile_(float* out, int n_pairs);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* REVO_HIP_H */
