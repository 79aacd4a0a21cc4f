/*
 * vo_hip.h -- C-ABI of the MI355X (gfx950) back end for the feature-matching +
 * sliding-window bundle-adjustment hot path of cteufel13/VisualOdometry.
 *
 * Plain C: pointers, sizes and status codes only.  The Python host package
 * (visualodometry_amd/_lib.py) binds it with ctypes; INTEGRATION.md shows the
 * binding.  Every entry point is host-synchronous unless its name ends in
 * _async, and returns VO_OK (0) or a negative vo_status.
 *
 * Reference interfaces replaced (paths relative to the reference repo root):
 *   vo_match_knn2_ratio   <- FeatureFrontend.match_frames, SIFT branch,
 *                            src/modules/frontend.py:86-111
 *                            (cv2.BFMatcher(cv2.NORM_L2, crossCheck=False)
 *                             .knnMatch(des0, des1, k=2) at :34/:101 and the
 *                             Lowe ratio test at :103-109)
 *   vo_match_knn2         <- the knnMatch(k=2) call alone, frontend.py:101
 *   vo_triangulate        <- triangulate_points, src/modules/frontend.py:115-148
 *   vo_pnp_ransac         <- cv2.solvePnPRansac in the tracking step,
 *                            src/modules/vo.py:135-141
 *   vo_sift_detect_and_compute <- cv2.SIFT_create(...).detectAndCompute,
 *                            src/modules/frontend.py:27-32,55 (vo_sift_detect: its
 *                            extrema stage, for parity)
 *   vo_ba_*               <- new: the reference has no BA (pyceres/pycolmap
 *                            are declared in pyproject.toml:11-12 but never
 *                            imported).  Insertion point: the keyframe hook
 *                            VisualOdometry._create_keyframe,
 *                            src/modules/vo.py:252-288.  Projection model of
 *                            frontend.py:128-140, pose convention T_cw of
 *                            vo.py:260-261.
 */
#ifndef VO_HIP_H
#define VO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VO_ABI_VERSION 1

typedef enum {
  VO_OK = 0,
  VO_ERR_ARG = -1,      /* bad argument / unsupported shape */
  VO_ERR_HIP = -2,      /* HIP runtime error */
  VO_ERR_NOT_SPD = -3,  /* reduced camera system not positive definite */
  VO_ERR_RCCL = -4,     /* RCCL error */
  VO_ERR_NOMEM = -5,    /* device allocation failed */
  VO_ERR_STATE = -6,    /* call out of order (e.g. vo_ba_run before vo_ba_setup) */
  VO_ERR_NODEV = -7     /* no usable gfx950 device */
} vo_status;

typedef struct vo_ctx vo_ctx;

/* ---- library / context -------------------------------------------------- */
int vo_abi_version(void);
/* Thread-local message for the last failing call on this thread. */
const char* vo_last_error(void);
/* Creates a context bound to HIP device `device` with its own stream.  flags: 0.
 * Returns NULL on failure (vo_last_error() says why). */
vo_ctx* vo_create(int device, int flags);
void vo_destroy(vo_ctx* ctx);
/* The context's HIP stream (hipStream_t), for callers that enqueue on it. */
void* vo_stream(vo_ctx* ctx);
int vo_synchronize(vo_ctx* ctx);

/* Device buffers on the context's device (so callers need no second HIP
 * runtime in-process).  Copies are synchronous on the context stream. */
void* vo_device_alloc(vo_ctx* ctx, uint64_t bytes);
int vo_device_free(vo_ctx* ctx, void* ptr);
int vo_memcpy_h2d(vo_ctx* ctx, void* dst, const void* src, uint64_t bytes);
int vo_memcpy_d2h(vo_ctx* ctx, void* dst, const void* src, uint64_t bytes);

/* ---- descriptor matching (knn k=2 + Lowe ratio) --------------------------
 * des0: (n0, dim) float32 row-major, the "query" (previous keyframe) set;
 * des1: (n1, dim) float32 row-major, the "train" (current frame) set.
 * Semantics of OpenCV BFMatcher(NORM_L2).knnMatch(k=2) followed by the
 * reference ratio test:
 *   dist(i,j) = sqrtf(sum_d (a_id - b_jd)^2), the two nearest train rows per
 *   query under the order (dist, j) -- equal distances keep the lower j --,
 *   and pair (i, j1) is kept iff (double)dist1 < ratio * (double)dist2.
 *   Queries with n1 < 2 neighbours emit nothing.  Pairs are written in
 *   ascending query order as int32 (query, train).
 * Descriptors whose values are all integers in [0, 255] (OpenCV SIFT) take the
 * exact int8 MFMA path; any other values take the fp32 path, whose per-pair
 * distance is the k-ordered fmaf chain sum((a-b)^2).
 * out_pairs capacity: 2*n0 int32.  Empty inputs give *out_count = 0.        */
int vo_match_knn2_ratio(vo_ctx* ctx, const float* des0, int n0, const float* des1,
                        int n1, int dim, double ratio, int32_t* out_pairs,
                        int32_t* out_count);

/* Top-2 per query without the ratio test.  idx_out: (n0, 2) int32 (-1 when
 * fewer than 2 neighbours exist), dist_out: (n0, 2) float32 distances
 * (FLT_MAX where idx is -1). */
/* The same with a cached query side: the reference matches every frame against the same
 * keyframe (vo.py:64-65, des0 = the keyframe's descriptors), so a nonzero des0_tag keys a cache
 * of des0's device copy and packed rows.  A call whose (des0 pointer, n0, dim, des0_tag) equal
 * the cached ones skips des0's upload and packing; the caller gives a new tag whenever des0's
 * contents may have changed (0 = no cache).  Results are vo_match_knn2_ratio's. */
int vo_match_knn2_ratio_q(vo_ctx* ctx, const float* des0, int n0, uint64_t des0_tag, const float* des1,
                          int n1, int dim, double ratio, int32_t* out_pairs, int32_t* out_count);
/* Device-resident descriptors (pointers into this process's HIP device memory, e.g. the
 * feature dicts' GPU tensors, which frontend.py:66-67 moves to config.device): no descriptor
 * crosses PCIe, only the pairs come back to the host.  The caller orders the producer of the
 * descriptors before the call (e.g. synchronises its stream).  des0_tag as in _q. */
int vo_match_knn2_ratio_dev(vo_ctx* ctx, const float* d_des0, int n0, uint64_t des0_tag,
                            const float* d_des1, int n1, int dim, double ratio, int32_t* out_pairs,
                            int32_t* out_count);
int vo_match_knn2(vo_ctx* ctx, const float* des0, int n0, const float* des1, int n1,
                  int dim, int32_t* idx_out, float* dist_out);

/* Batched frame pairs, device pointers, enqueued on the context stream.
 * d_des0: (batch, n0, dim), d_des1: (batch, n1, dim) float32 on the device;
 * d_best: (batch, n0) int32 -- the train index kept for each query by the
 * ratio test, or -1.  Nothing is copied to the host. */
int vo_match_batch_async(vo_ctx* ctx, const float* d_des0, const float* d_des1,
                         int batch, int n0, int n1, int dim, double ratio,
                         int32_t* d_best);

/* Mutual-check matching: the ratio test above plus OpenCV's BFMatcher(crossCheck=True) rule
 * (the brute-force stand-in for a one-to-one learned matcher: the VO loop indexes
 * keyframe["ids"][ref_indices], vo.py:66,121,252-288, which needs one-to-one pairs).
 *   Forward pass: unchanged -- top-2 per query under keys (sqrtf(d2), j), equal distances
 *   keep the lower j; (i, j1) kept iff (double)dist1 < ratio * (double)dist2; queries with
 *   fewer than 2 neighbours emit nothing.
 *   Cross check: a kept pair (i, j) survives iff i is the nearest query row of train row j
 *   under keys (sqrtf(d2(i', j)), i') over all query rows i' -- equal distances keep the lower
 *   query index.  The distances are the forward pass's arithmetic (the exact integer d2 on
 *   the int8 path, the k-ordered fmaf chain on the float path); (a-b)^2 and (b-a)^2 are
 *   bit-identical, so the reverse nearest is vo_match_knn2(des1, des0)'s first column.
 * Output as vo_match_knn2_ratio's (ascending query order, capacity 2*n0 int32); no train index
 * appears twice.  n0 == 0 or n1 == 0 gives *out_count = 0, n1 == 1 nothing (the forward rule),
 * n0 == 1 is legal.  Results never depend on vo_match_hint, the query cache or the splits.
 * flags: VO_MATCH_DEVICE_PTRS = des0 / des1 are device pointers, validated as
 * vo_match_knn2_ratio_dev's (VO_ERR_ARG before any launch); otherwise host arrays.  A nonzero
 * des0_tag keys the query cache as in _q: on a hit des0 is neither uploaded nor packed again,
 * for either role it plays (query rows forward, columns in the reverse pass). */
#define VO_MATCH_DEVICE_PTRS 1
int vo_match_mutual(vo_ctx* ctx, const float* des0, int n0, uint64_t des0_tag, const float* des1,
                    int n1, int dim, double ratio, int flags, int32_t* out_pairs, int32_t* out_count);
/* vo_match_batch_async with the cross check: d_best (batch, n0) int32, the train index of each
 * surviving pair or -1. */
int vo_match_mutual_batch_async(vo_ctx* ctx, const float* d_des0, const float* d_des1,
                                int batch, int n0, int n1, int dim, double ratio,
                                int32_t* d_best);
/* Projection-gated matching (search by projection): query rows (landmarks) against train rows
 * (the frame's keypoints), each query only among the keypoints inside a window around its
 * predicted pixel position.  Build-defined: the reference has no such association step.
 *   Inputs: des0 (n0, dim), opt->pred (n0, 2) and opt->radius (n0, or NULL: opt->radius0 for every
 *   query) are host arrays; des1 (n1, dim) and opt->kp1 (n1, 2) are host arrays, or with
 *   VO_MATCH_DEVICE_PTRS in opt->flags device pointers (the feature dict's tensors), validated as
 *   vo_match_knn2_ratio_dev's (VO_ERR_ARG before any launch).
 *   Gate: train row j is a candidate of query i iff query i is active and, with the float32
 *   differences dx = kp1[j].x - pred[i].x, dy = kp1[j].y - pred[i].y,
 *   (double)dx*dx + (double)dy*dy <= (double)r_i*r_i.  Query i is inactive (no candidates) when
 *   pred[i] has a non-finite component or !(r_i >= 0) (negative or NaN).  r_i = 0 admits an exactly
 *   coincident keypoint, r_i = +inf every keypoint with finite coordinates; a keypoint with a
 *   non-finite coordinate is never a candidate.
 *   Distance: the float path's arithmetic for every call -- d2 the k-ordered fp32 chain
 *   acc = fmaf(a_k - b_k, a_k - b_k, acc), dist = sqrtf(d2) correctly rounded (for SIFT integers
 *   with dim <= 256 the exact integer d2, so the int8 path's values).
 *   Selection: the two smallest keys (dist, j) among the candidates, equal distances keeping the
 *   lower j; a candidate whose distance is not < FLT_MAX is never selected.  (i, j1) is kept iff
 *   query i has a selected candidate, max_dist == 0 or dist1 <= (float)max_dist, and it has only
 *   one selected candidate or (double)dist1 < ratio * (double)dist2: a lone candidate passes the
 *   ratio test vacuously (what max_dist is for).
 *   VO_MATCH_GATE_UNIQUE: among the kept pairs naming the same train row j only the one with the
 *   smallest key (dist1, i) survives; the output is then one-to-one.
 *   Output: out_pairs int32 (query, train) in ascending query order, capacity 2*n0 int32;
 *   out_dist (optional, n0 floats) dist1 per pair; *out_count the number of pairs.  n0 == 0 or
 *   n1 == 0 gives *out_count = 0.
 *   VO_ERR_ARG (before the context or a device is touched): opt, out_pairs or out_count NULL,
 *   negative sizes, dim < 1, a null array with a nonzero size, non-finite or negative ratio or
 *   max_dist, unknown flag bits, reserved != 0.
 * width / height are a hint for the extent of the cell grid the keypoints are binned into (0:
 * unknown).  Results never depend on them, on vo_match_hint, on the query cache or on how the
 * search is binned: binning only prunes, the gate is evaluated exactly for every pair.
 * Profiler ids: the clears and the grid build count under 3 (match_pack), the gated search and
 * the unique filter under 5 (match_f32). */
#define VO_MATCH_GATE_UNIQUE 2
typedef struct {
  const float* pred;    /* (n0, 2) host: predicted pixel position of each query in the train image */
  const float* radius;  /* (n0) host, or NULL: radius0 for every query */
  const float* kp1;     /* (n1, 2) keypoint positions of the train rows (host, or device with the flag) */
  float radius0;
  int32_t width, height;  /* image extent hint; 0 = unknown */
  double ratio, max_dist; /* max_dist 0 = not tested */
  int32_t flags;          /* VO_MATCH_DEVICE_PTRS | VO_MATCH_GATE_UNIQUE */
  int32_t reserved;       /* must be 0 */
} vo_match_gate_options;
int vo_match_gated(vo_ctx* ctx, const float* des0, int n0, const float* des1, int n1, int dim,
                   const vo_match_gate_options* opt, int32_t* out_pairs, float* out_dist,
                   int32_t* out_count);

/* Segment-gated matching: vo_match_gated with a capsule for a gate.  Query i is compared only with
 * the train rows whose keypoint lies within r_i of the segment a_i b_i given in the train image:
 * dist(kp1[j], segment) <= r_i.  One producer of such segments is the epipolar search for new
 * landmarks (a keypoint of one view with a depth range is a piece of its epipolar line in the
 * other: matcher.epipolar_segments); a zero-length segment is vo_match_gated's circular gate with
 * pred = a, to the bit.  Build-defined: the reference has no such step.
 *   Everything but the gate is vo_match_gated's contract word for word: the inputs (opt->seg
 *   (n0, 4) = ax, ay, bx, by and opt->radius are host arrays; des1 and opt->kp1 host, or device
 *   with VO_MATCH_DEVICE_PTRS and validated alike), the distance, the selection of the two
 *   smallest (dist, j) with dist < FLT_MAX, the keep rule (max_dist, then the ratio test, vacuous
 *   for a lone candidate), VO_MATCH_GATE_UNIQUE, the output layout and capacity, count 0 for
 *   n0 == 0 or n1 == 0, and the VO_ERR_ARG cases, answered before the context or a device is
 *   touched.
 *   Gate: query i is active iff its four segment values are finite and r_i >= 0 (not NaN); a
 *   keypoint with a non-finite coordinate is never a candidate.  With the float32 differences
 *     dx = bx - ax, dy = by - ay, vx = kx - ax, vy = ky - ay, wx = kx - bx, wy = ky - by
 *   widened to double (every product of two of them is exact, every two-term sum below is rounded
 *   once, so fused and unfused evaluation agree to the bit):
 *     dd = dx*dx + dy*dy, s = vx*dx + vy*dy, cr = vx*dy - vy*dx, r2 = (double)r*r
 *     if      s <= 0 : candidate iff vx*vx + vy*vy <= r2      (nearest point a)
 *     else if s >= dd: candidate iff wx*wx + wy*wy <= r2      (nearest point b)
 *     else           : candidate iff cr*cr <= r2*dd           (the interior; no division)
 *   in this order, so a == b and r = +inf never form inf * 0; r = +inf admits every keypoint with
 *   finite coordinates.
 * width / height size the cell grid only (0: unknown); results never depend on them nor on how
 * the search walks the grid: binning only prunes, every pair in a walked cell takes the gate above.
 * Profiler ids as vo_match_gated: the grid build under 3 (match_pack), search and unique filter
 * under 5 (match_f32). */
typedef struct {
  const float* seg;     /* (n0, 4) host: ax, ay, bx, by -- the segment of each query in the train image */
  const float* radius;  /* (n0) host, or NULL: radius0 for every query */
  const float* kp1;     /* (n1, 2) host, or device with VO_MATCH_DEVICE_PTRS */
  float radius0;
  int32_t width, height;   /* grid extent hint, 0 = unknown; results never depend on it */
  double ratio, max_dist;  /* max_dist 0 = not tested */
  int32_t flags;           /* VO_MATCH_DEVICE_PTRS | VO_MATCH_GATE_UNIQUE */
  int32_t reserved;        /* 0 */
} vo_match_segment_options;
int vo_match_segment(vo_ctx* ctx, const float* des0, int n0, const float* des1, int n1, int dim,
                     const vo_match_segment_options* opt, int32_t* out_pairs, float* out_dist,
                     int32_t* out_count);

/* Descriptor-kind hint for this context's later matcher calls (results never depend on
 * it; the device checks every call's values either way):
 *   VO_DESC_AUTO (0, default) launches both paths' kernels; a call runs the one its
 *     values need (a device-side flag) -- SIFT integers on the int8 MFMA sweep, other
 *     floats on the bf16 MFMA shortlist + exact re-rank;
 *   VO_DESC_SIFT (1): OpenCV SIFT integers expected (FeatureFrontend with the SIFT
 *     extractor, frontend.py:25-34): the float shortlist is not launched, and a call
 *     whose values are not 0..255 integers takes the exact fp32 sweep instead;
 *   VO_DESC_FLOAT (2): SuperPoint-like floats expected: no int8 pack, integer check, int8
 *     sweep or merge is launched; every call takes the bf16 shortlist + exact re-rank (exact
 *     for SIFT integers too), and a call with a non-finite value is answered by the re-rank
 *     kernel's exact scan (the exact fp32 sweep's result). */
#define VO_DESC_AUTO 0
#define VO_DESC_SIFT 1
#define VO_DESC_FLOAT 2
int vo_match_hint(vo_ctx* ctx, int kind);

/* ---- sliding-window bundle adjustment ------------------------------------ */
typedef struct {
  int32_t n_poses;   /* N cameras in the window                               */
  int32_t n_points;  /* L landmarks                                           */
  int32_t n_obs;     /* M observations                                        */
  int32_t n_fixed;   /* poses 0..n_fixed-1 are held fixed (gauge)             */
  double fx, fy, cx, cy;      /* pinhole K, no distortion (frontend.py:139)  */
  double lambda;              /* Levenberg damping added to every block (>=0) */
  const int32_t* point_ptr;   /* (n_points+1) CSR: obs of point p are
                                 point_ptr[p]..point_ptr[p+1]-1               */
  const int32_t* obs_cam;     /* (n_obs) camera index of each observation    */
  const float* obs_uv;        /* (n_obs, 2) pixel measurement (float32, as
                                 FeatureFrontend keypoints, frontend.py:59)   */
} vo_ba_problem;

/* Uploads the observation structure and builds the static execution plan
 * (landmark chunks, per-workgroup camera-pair windows, reduced-system profile).
 * Replaces any previous problem in this context.  *session_out receives the id of
 * this problem (unique in the process); every later vo_ba_* call on it passes that
 * id and fails with VO_ERR_STATE once another vo_ba_setup on the context has replaced
 * the problem (whose sizes the caller's buffers no longer match).  With a
 * communicator (vo_comm_init) every rank reaches the same verdict: a shard that
 * fails its checks on one rank is VO_ERR_ARG on all ranks. */
int vo_ba_setup(vo_ctx* ctx, const vo_ba_problem* prob, uint64_t* session_out);
/* Optional, once per context before its first keyframe (SlidingWindowBA's constructor, with
 * the window and map capacity of the VO configuration): pre-sizes every host and device
 * buffer a window of about n_poses cameras, n_points landmarks and n_obs observations needs
 * (page-locked plan images, device slabs and systems, kernel attributes), so the first
 * vo_ba_setup of the drive (vo.py:252-288, the first keyframe) allocates nothing and faults in
 * no page.  The context has no problem afterwards.  VO_ERR_STATE with a communicator of more
 * than one rank (call it before vo_comm_init). */
int vo_ba_reserve(vo_ctx* ctx, int n_poses, int n_points, int64_t n_obs, int n_fixed);
/* poses: (n_poses, 12) float64 = R_cw row-major (9) then t_cw (3);
 * points: (n_points, 3) float64 -- the sizes of the session's problem. */
int vo_ba_set_state(vo_ctx* ctx, uint64_t session, const double* poses, const double* points);
int vo_ba_get_state(vo_ctx* ctx, uint64_t session, double* poses, double* points);
/* Runs `iters` pure Gauss-Newton iterations (every step accepted, the damping fixed at the
 * problem's lambda; vo_ba_run_lm below is the variant that tests each step) on the
 * device-resident state.  cost_out (iters+1 doubles, may be NULL): sum of
 * squared residuals (of rho under vo_ba_set_robust) before each iteration and after the last one.
 * Returns VO_ERR_NOT_SPD (state left at the last good iterate) if the reduced
 * camera system is not positive definite. */
int vo_ba_run(vo_ctx* ctx, uint64_t session, int iters, double* cost_out);
/* Same, enqueued on the context stream with no host synchronisation and no
 * cost read-back (for timing).  Errors surface at the next synchronous call. */
int vo_ba_run_async(vo_ctx* ctx, uint64_t session, int iters);
/* One GN iteration with the intermediate quantities exported (parity tests):
 * S_out: dense (6F, 6F) float64 reduced camera matrix with F = n_poses-n_fixed
 * (may be NULL), b_out: (6F), dc_out: (6F) pose update (may be NULL),
 * cost_out: 1 double.  The state is advanced by the step. */
int vo_ba_gn_step(vo_ctx* ctx, uint64_t session, double* S_out, double* b_out, double* dc_out,
                  double* cost_out);
/* Levenberg-Marquardt step control: `iters` trial steps, each kept only if it lowers the cost,
 * with the damping adapted on the device (no host round trip per iteration).  With x the
 * accepted state, c = cost(x) (sum ||r||^2, or sum rho under vo_ba_set_robust) and l the damping:
 *   for k in 0 .. iters-1:
 *     cost[k] = c; lambda[k] = l
 *     x' = x (+) the step vo_ba_gn_step takes at x with the problem's lambda replaced by l
 *     t = cost(x'); trial[k] = t
 *     if t < c (false for NaN, +inf): x = x'; c = t; l = max(l * down, lambda_min); accepted[k] = 1
 *     else:                                          l = min(l * up, lambda_max);   accepted[k] = 0
 *   cost[iters] = c; lambda[iters] = l
 * Every c and t is one kernel path's fixed-order sum, so cost[k+1] == trial[k] bit for bit after
 * an accepted step; a rejected step restores poses and points bit for bit.  LM guarantees a
 * non-increasing cost and needs no hand-tuned lambda; it does not promise a smaller error against
 * ground truth than a heavily damped vo_ba_run (Step control).
 * opt == NULL or a zero field takes the default: up 10, down 0.1, lambda_min 1e-6, lambda_max 1e6,
 * lambda0 = the problem's lambda when that is > 0, else 1e-4; lambda0 is clamped into
 * [lambda_min, lambda_max].  VO_ERR_ARG: a non-finite field, lambda0 < 0, up <= 1, down outside
 * (0, 1), lambda_min <= 0, lambda_min > lambda_max.  VO_ERR_STATE: a stale session, or a
 * communicator of more than one rank (LM over landmark shards is not built).  iters == 0 is
 * legal: cost_out[0] is the cost, the state is untouched.  Outputs (any may be NULL): cost_out and
 * lambda_out iters+1 doubles, trial_out iters doubles, accepted_out iters bytes.
 * A non-SPD reduced system or a timed-out fused reduction fails the run as it fails vo_ba_run
 * (VO_ERR_NOT_SPD / VO_ERR_HIP): the state is the last accepted one, cost and lambda of the
 * failing iteration are its accepted state's, its trial and decision and every later entry are
 * NaN / 0.  (A non-SPD system is not treated as a rejected step.  The loop runs every trial unless
 * vo_ba_set_lm_stop below gave it a termination criterion.)
 * A pending vo_ba_gn_step's landmark update is applied first, under the lambda and delta it was
 * solved with; after the call no step is pending, and every other vo_ba_* call works as on any
 * state. */
typedef struct {
  double lambda0, up, down, lambda_min, lambda_max;
} vo_ba_lm_options;
int vo_ba_run_lm(vo_ctx* ctx, uint64_t session, int iters, const vo_ba_lm_options* opt, double* cost_out,
                 double* lambda_out, double* trial_out, uint8_t* accepted_out);
/* Same, enqueued on the context stream with no host synchronisation and no read-back. */
int vo_ba_run_lm_async(vo_ctx* ctx, uint64_t session, int iters, const vo_ba_lm_options* opt);
/* Synchronises and returns the log of the session's last vo_ba_run_lm / _async: its first n
 * iterations (n + 1 costs and lambdas, n trials and decisions; n at most that run's iters, else
 * VO_ERR_ARG; any pointer may be NULL), and that run's return code. */
int vo_ba_lm_log(vo_ctx* ctx, uint64_t session, int n, double* cost_out, double* lambda_out, double* trial_out,
                 uint8_t* accepted_out);
/* Termination of the LM loop, decided on the device (still one fixed launch sequence and no host
 * round trip per iteration).  With rej the number of consecutive rejections, 0 at the start of each
 * run, three tests follow the decision of trial k (c = cost[k], t = trial[k], in doubles):
 *   accepted:  rej = 0
 *              if ftol > 0 and (c - t) <= ftol * c:        stop, VO_BA_LM_FTOL
 *              else if xtol > 0 and max_i |dc_i| <= xtol:  stop, VO_BA_LM_XTOL   (dc: the 6F entries of
 *                                                                                 trial k's pose update)
 *   rejected:  rej += 1
 *              if max_rejects > 0 and rej >= max_rejects:  stop, VO_BA_LM_REJECTS
 * A stop at trial k ends the run with trials = k + 1; a run that never stops has trials = iters and
 * VO_BA_LM_RAN_ALL.  A stop changes nothing before it: log entries 0 .. k (cost and lambda to
 * k + 1), poses and points are bit for bit those of vo_ba_run_lm(iters = k + 1) with no criterion
 * set.  The trials behind a stop are still enqueued, but their kernels leave at their first test
 * of the status word; their log entries read trial = NaN, accepted = 0, and cost and lambda repeat
 * entry k + 1, so cost_out[iters] is the final cost whether or not the run stopped.  A stopped run
 * returns VO_OK and leaves nothing behind: the next vo_ba_run* call on the session, synchronous or
 * not, needs no read in between.
 * vo_ba_set_lm_stop: session state like vo_ba_set_robust, for every later vo_ba_run_lm / _async.
 * stop == NULL or all fields zero: never stop, the state after every vo_ba_setup.  VO_ERR_ARG: a
 * non-finite or negative field, ftol >= 1, reserved != 0.  VO_ERR_STATE: a stale session.
 * vo_ba_lm_stop_info: synchronises as vo_ba_lm_log does and reports how the session's last LM run
 * ended (either pointer may be NULL).  After a failed run (non-SPD or timeout, above): trials = the
 * failing iteration's index, reason = VO_BA_LM_FAILED.  VO_ERR_STATE: no LM run on this session. */
typedef struct {
  double ftol, xtol;
  int32_t max_rejects, reserved;
} vo_ba_lm_stop;
#define VO_BA_LM_FAILED (-1)
#define VO_BA_LM_RAN_ALL 0
#define VO_BA_LM_FTOL 1
#define VO_BA_LM_XTOL 2
#define VO_BA_LM_REJECTS 3
int vo_ba_set_lm_stop(vo_ctx* ctx, uint64_t session, const vo_ba_lm_stop* stop);
int vo_ba_lm_stop_info(vo_ctx* ctx, uint64_t session, int32_t* trials_out, int32_t* reason_out);
/* Robust cost: huber_delta = delta >= 0 in pixels, 0 (the default of every vo_ba_setup) is the
 * plain sum of squares.  For an observation with raw residual r, n^2 = r.r: n^2 <= delta^2 gives
 * rho = n^2; otherwise rho = 2 delta n - delta^2, and the linearisation scales r and both
 * Jacobians by s = sqrt(delta / n) (first-order IRLS).  Every cost the API reports is then
 * sum(rho).  Valid any time after vo_ba_setup; the new delta holds from the next linearisation
 * (a pending step's landmark update is applied first, under the delta it was computed with).
 * VO_ERR_ARG for a negative or non-finite delta.  With a communicator every rank sets it on its
 * own shard. */
int vo_ba_set_robust(vo_ctx* ctx, uint64_t session, double huber_delta);
/* Per observation, in the order of vo_ba_problem.obs_cam (n_obs doubles each, either pointer
 * may be NULL): the raw, unweighted squared reprojection error in pixels^2 and the camera-frame
 * depth z, at the device-resident state (after any pending landmark update).  With a
 * communicator: the rank's own observations. */
int vo_ba_residuals(vo_ctx* ctx, uint64_t session, double* err2_out, double* depth_out);
/* Covariance read-out at the device-resident state (after any pending landmark update), for UNIT
 * pixel variance: the caller scales every value by sigma^2, its estimate of the measurement
 * variance in pixels^2 (e.g. final cost / degrees of freedom).
 * H = J^T J of the session's problem in the solver's own parametrisation (the left se(3) twist
 * (rho, phi) per free pose, the 3 world coordinates per landmark), with the session's Huber scale
 * as the linearisation applies it and lambda * I added to every pose and landmark block: `lambda`
 * is this call's argument, not the problem's; 0 gives the Gauss-Newton covariance.  A landmark
 * whose 3x3 block V_p fails the pivot test is frozen and leaves the system, as in every step.  S is
 * the reduced camera system of that linearisation (vo_ba_gn_step's S_out under `lambda`),
 * F = n_poses - n_fixed, W_o = J_pose^T J_point of observation o.  Outputs, any may be NULL:
 *   pose_dense_out (6F, 6F) row-major: Sigma_cc = S^-1; one triangle is computed and mirrored, so
 *     it is symmetric bit for bit;
 *   pose_cov_out (F, 6, 6): the diagonal blocks of Sigma_cc, the same bits;
 *   point_cov_out (n_points, 3, 3), in the problem's landmark order:
 *     Sigma_pp = V_p^-1 + T_p Sigma_cc T_p^T, where T_p (3 x 6F) holds in the columns of free
 *     camera f the sum over p's observations o in f of (W_o V_p^-1)^T (duplicate observations
 *     add; fixed cameras enter V_p only, so a landmark seen by fixed cameras alone has
 *     V_p^-1); each block symmetric bit for bit; nine NaNs for a frozen landmark.
 * Nothing is solved and nothing but the pending update is written: poses and points are
 * afterwards what they were, and every later vo_ba_run* gives the bits it would have given
 * without this call.  All sums run in a fixed order: two calls at one state agree bit for bit.
 * VO_ERR_NOT_SPD: S is not positive definite; the requested outputs are filled with NaN and the
 * session stays usable.  VO_ERR_ARG: lambda negative or not finite, or more than 567 free poses
 * (the solve kernels keep 6F x 6 doubles in the 160 KiB of LDS).  VO_ERR_STATE: a stale session,
 * no state set, or a communicator of more than one rank (covariance over landmark shards is not
 * built). */
int vo_ba_covariance(vo_ctx* ctx, uint64_t session, double lambda, double* pose_cov_out, double* pose_dense_out,
                     double* point_cov_out);
/* Observation weights.  Every observation o has an information weight w_o >= 0 (1 / sigma^2 in
 * pixels^-2), 1 after every vo_ba_setup.  With r, J_pose, J_point the raw residual and Jacobians:
 *   w_o > 0: the linearisation uses sqrt(w_o) r, sqrt(w_o) J_pose, sqrt(w_o) J_point; the session's
 *     Huber rule, if any, is applied to the whitened residual (n^2 = w_o r.r against delta^2, the
 *     Huber scale multiplying on top), and the observation's cost term is rho(w_o r.r), which is
 *     w_o r.r without Huber.  sqrt(w_o) is taken once on the host (IEEE double); the device only
 *     multiplies.
 *   w_o == 0: the observation is inactive and contributes exact zeros to the cost, V, W, S, b and
 *     g -- by a select, not a product, so an inactive observation whose raw residual is not finite
 *     (zero or negative depth) turns no sum into NaN.
 * A landmark its active observations no longer support is frozen by the pivot test as ever (at
 * lambda = 0; under damping it stays put).  vo_ba_residuals stays raw and unweighted;
 * vo_ba_covariance honours the weights (H = J^T W J, the Huber scale on the whitened residual).
 * vo_ba_set_obs_weights: w holds n_obs weights in the order of vo_ba_problem.obs_cam; NULL restores
 * all ones.  Valid any time after vo_ba_setup; a pending vo_ba_gn_step's landmark update is applied
 * first, under the weights it was solved with.  While a session has no weights (after vo_ba_setup,
 * and after NULL until a cull) every launch is the one a session without this feature makes; with
 * weights, K1 is always a launch of its own (never inside the solve launch), and a K1 layout
 * without a weighted form (the four-wave K1 of the testing switch) fails the run with
 * VO_ERR_STATE.  VO_ERR_ARG: a negative or non-finite weight, and nothing is changed.
 * VO_ERR_STATE: a stale session, or a communicator of more than one rank (weights over landmark
 * shards are not built).
 * vo_ba_get_obs_weights: synchronises and returns the current weights in problem order: what was
 * set, the culled observations at 0. */
int vo_ba_set_obs_weights(vo_ctx* ctx, uint64_t session, const double* w);
int vo_ba_get_obs_weights(vo_ctx* ctx, uint64_t session, double* w_out);
/* Device-side outlier culling at the device-resident state (after any pending landmark update).
 * With err2_o and z_o the values vo_ba_residuals reports there (the same arithmetic), an active
 * observation is deactivated (w_o := 0) iff
 *   max_chi2 > 0 and w_o * err2_o > max_chi2,  or  z_o <= min_depth,  or  err2_o or z_o is not finite;
 * then every landmark with fewer than min_track active observations loses all of them
 * (min_track <= 0: not tested; the sensible value is 2).  A culled observation comes back only
 * through vo_ba_set_obs_weights.  Nothing else is written: poses, points, the LM log and the
 * status word stay as they were, and a second cull at the same state with the same options culls
 * nothing.  n_culled_out: observations this call deactivated; n_active_out: observations active
 * after it (either may be NULL).  vo_ba_cull_async enqueues the same kernels on the context
 * stream without any host synchronisation, so run_lm_async, cull_async, run_lm_async, ... makes no
 * round trip; its outcome is read with vo_ba_get_obs_weights.  VO_ERR_ARG: a non-finite field,
 * max_chi2 < 0 or reserved != 0.  VO_ERR_STATE: a stale session, no state set, or a communicator
 * of more than one rank. */
typedef struct {
  double max_chi2;   /* 0: not tested */
  double min_depth;
  int32_t min_track; /* <= 0: not tested */
  int32_t reserved;  /* 0 */
} vo_ba_cull_options;
int vo_ba_cull(vo_ctx* ctx, uint64_t session, const vo_ba_cull_options* opt, int32_t* n_culled_out,
               int32_t* n_active_out);
int vo_ba_cull_async(vo_ctx* ctx, uint64_t session, const vo_ba_cull_options* opt);
/* Pose prior.  vo_ba_setup_prior is vo_ba_setup with a quadratic cost on the leading free poses,
 * e.g. the Schur complement of what left a sliding window.  prior == NULL is vo_ba_setup itself:
 * the same plan, digests, launches and bits.
 * For free pose f < K let xi_f = (rho, phi) be the twist that the solver's own update map
 * T <- exp(delta^) T takes poses0[f] to the current pose by: the SE(3) log of T_f T0_f^-1 (the
 * exp map's coefficients, series below its threshold included, so the two are inverses; pose
 * differences of less than pi).  With xi the 6K stacked entries, every cost the API reports
 * (vo_ba_run, vo_ba_run_lm costs and trials, vo_ba_gn_step) gains
 *   E_prior = cost0 - 2 eta^T xi + xi^T Lambda xi,
 * and the reduced system S dc = b of every linearisation becomes
 *   (S + Lambda^) dc = b + (eta^ - Lambda^ xi^),     ^: padded with zeros to 6F,
 * which uses the first-order Jacobian d xi / d delta ~ I of the log (exact at xi = 0, the state a
 * marginalisation hands over; the right Jacobian of the log is not applied).  The prior is not
 * robustified, weighted or culled; the problem's lambda and LM's are added as without it.
 * vo_ba_gn_step's S_out and b_out and vo_ba_covariance include it (it is part of S);
 * vo_ba_residuals and vo_ba_cull do not see it.  Every sum runs in a fixed order: two runs from one
 * state agree bit for bit, and a rejected LM step still restores poses and points bit for bit.
 * The prior couples its poses pairwise, so the profile of S has a dense leading K x K block
 * triangle; the banded solver stays in use while the widened bandwidth fits it (K <= 10 keeps a
 * window of tracks of at most 10 cameras banded), the profile solver takes over otherwise.  A session
 * with a prior runs K1 and the prior's kernel as launches of their own, never inside the solve
 * launch; without one every launch is the one vo_ba_setup's session makes.
 * VO_ERR_ARG: K < 1, K > n_poses - n_fixed (or beyond 440: the prior's kernel keeps xi,
 * Lambda xi and its partial sums in 64 KiB of LDS), reserved != 0, a null array or any non-finite value.
 * VO_ERR_STATE: a communicator of more than one rank (a prior over landmark shards is not built).
 * A system that is not positive definite fails as without a prior. */
typedef struct {
  int32_t n_poses;       /* K >= 1: the prior covers free poses 0..K-1 (window cameras n_fixed..n_fixed+K-1) */
  int32_t reserved;      /* 0 */
  const double* info;    /* (6K,6K) row-major Lambda; the lower triangle is read and mirrored */
  const double* rhs;     /* (6K) eta */
  const double* poses0;  /* (K,12) linearisation poses, laid out as vo_ba_set_state */
  double cost0;
} vo_ba_pose_prior;
int vo_ba_setup_prior(vo_ctx* ctx, const vo_ba_problem* prob, const vo_ba_pose_prior* prior, uint64_t* session_out);
/* Marginalisation: the prior that a slide by n_drop cameras leaves, computed at the device-resident
 * state (after any pending landmark update).  Nothing else is written: poses, points, weights, the
 * LM log and the status word are afterwards what they were, as after vo_ba_covariance.
 * D = window cameras 0..n_drop-1 (1 <= n_drop < n_poses); P_D = the landmarks with at least one
 * active observation in D (point_marg_out[p] = 1, problem order, n_points bytes).  Marginalised are
 * all active observations of P_D's landmarks, with the session's weights and Huber scale as the
 * linearisation applies them, and the session's prior, if it has one, in full: the new prior
 * replaces the old one.  Eliminated are P_D's landmarks (the 3x3 route of every step; a frozen
 * landmark leaves the system but stays marked) and the m = max(0, n_drop - n_fixed) leading free
 * poses (a dense Cholesky Schur complement); lambda >= 0 is added to the eliminated blocks only.
 * With R = (n_poses - n_fixed) - m remaining free poses, outputs (any may be NULL):
 *   info_out (6R, 6R) row-major, symmetric bit for bit; rhs_out (6R);
 *   *n_prior_out = K: 1 + the last remaining pose the prior touches (0: none); rows and columns
 *     beyond 6K are exact zeros;
 *   poses0_out (R, 12): the current poses of the remaining free cameras;
 *   *cost0_out: the marginalised factors' cost at this state, so xi = 0 there.
 * The caller's next window drops D and P_D, sets n_fixed' = max(0, n_fixed - n_drop) and passes the
 * leading K x K blocks of info_out, with rhs_out, poses0_out and cost0_out, as its prior.
 * VO_ERR_NOT_SPD: an eliminated pose block fails its pivot test; the outputs are NaN (the mask is
 * still written) and the session stays usable.  VO_ERR_ARG: n_drop outside 1..n_poses-1, lambda
 * negative or not finite, or the panel of 6R x 6m doubles with the eliminated block does not fit
 * 160 KiB of LDS.  VO_ERR_STATE: a stale session, no state set, a communicator of more than one
 * rank, or a K1 layout without a weighted form (the observation mask acts as weights). */
int vo_ba_marginalize(vo_ctx* ctx, uint64_t session, int n_drop, double lambda, int32_t* n_prior_out, double* info_out,
                      double* rhs_out, double* poses0_out, double* cost0_out, uint8_t* point_marg_out);
/* Pose factors.  vo_ba_setup_factors is vo_ba_setup_prior with a list of 6x6 costs on window cameras:
 * unary ones (a soft anchor on one pose) and between ones (a relative motion from the front end, an
 * odometry or IMU increment, a loop constraint inside the window).
 * n_factors == 0 is vo_ba_setup_prior(prob, prior) itself, and with prior == NULL too it is
 * vo_ba_setup: the same plan, digests, launches and bits.
 * Residual.  With T = T_cw, let A = T_i T_j^-1 for a between factor and A = T_i for a unary one
 * (cam_j == -1), and Z the measurement of A.  The residual is the twist xi = log(A Z^-1), the log
 * that of the prior (the exp map's own coefficients; rotations below pi).  Every cost the API
 * reports (vo_ba_run, vo_ba_run_lm costs and trials, vo_ba_gn_step) gains sum xi^T Lambda xi over
 * the factors.
 * Linearisation, first order under the solver's update T <- exp(delta^) T (the first-order Jacobian
 * of the log is taken as the identity, exact at xi = 0, the prior's convention):
 *   xi' ~ xi + delta_i - G delta_j,   G = Ad(A) = [[R_A, [t_A]x R_A], [0, R_A]] in (rho, phi) order,
 * G evaluated at the current poses at every linearisation; a unary factor has no delta_j term.
 * Contributions to the reduced system S dc = b, by free camera:
 *   S_ii += Lambda,  S_jj += G^T Lambda G,  S_ij (row i, column j) += -Lambda G,
 *   b_i  += -Lambda xi,  b_j += G^T Lambda xi.
 * A fixed endpoint contributes nothing to S and b; a factor between two fixed cameras adds its
 * (constant) cost only.  Several factors on one pair add, in factor order.  Factors are not
 * robustified, weighted or culled; the problem's lambda and LM's are added as without them.
 * vo_ba_gn_step's S_out and b_out and vo_ba_covariance include the factors; vo_ba_residuals and
 * vo_ba_cull do not see them.  Every sum runs in a fixed order (no atomics): two runs from one state
 * agree bit for bit, and a rejected LM step restores poses and points bit for bit.
 * Solver.  A between factor on free poses f_i > f_j lowers the profile's first[f_i] to at most f_j:
 * the banded solver stays while the widened bandwidth fits it (9 blocks), the profile solver takes
 * over otherwise; factors between consecutive keyframes never widen anything.  A session with
 * factors runs K1 as a launch of its own and one more kernel between K1 and the solve launch, which
 * computes the prior's terms too when the session has both.
 * vo_ba_marginalize: a factor with an endpoint among the dropped cameras 0..n_drop-1 is marginalised
 * with the landmark terms and the old prior (it enters the masked system and cost0); every other
 * factor is left out, and the caller passes those on, re-indexed, to the next window's setup.
 * VO_ERR_ARG (no device needed): n_factors < 0; factors == NULL with n_factors > 0; cam_i outside
 * 0..n_poses-1; cam_j >= n_poses or < -1; cam_i == cam_j; a non-finite value in meas or in the lower
 * triangle of info; n_factors > VO_BA_MAX_POSE_FACTORS.  That cap bounds what a setup adds to every
 * later linearisation: three slab rows and two rhs entries per factor for K2 to sum, and one cost
 * entry per 256 factors (one workgroup of the factor kernel) that K2, the LM decision and the
 * cost-only reduction each sum serially -- 16 entries at the cap.  Orthogonality of meas and
 * definiteness of info are the caller's: an indefinite Lambda surfaces as VO_ERR_NOT_SPD, as ever.
 * VO_ERR_STATE: a communicator of more than one rank. */
#define VO_BA_MAX_POSE_FACTORS 4096
typedef struct {
  int32_t cam_i;     /* window camera 0 .. n_poses-1 */
  int32_t cam_j;     /* a second window camera, or -1: a unary factor on cam_i */
  double meas[12];   /* Z, laid out as a pose of vo_ba_set_state (R row-major, t):
                        between: the measured T_i T_j^-1;  unary: the measured T_i   (T = T_cw) */
  double info[36];   /* Lambda, 6x6 row-major in twist order (rho, phi); the lower triangle is read and mirrored */
} vo_ba_pose_factor;   /* 392 bytes */
int vo_ba_setup_factors(vo_ctx* ctx, const vo_ba_problem* prob, const vo_ba_pose_prior* prior,
                        const vo_ba_pose_factor* factors, int32_t n_factors, uint64_t* session_out);
/* One-call convenience: setup + set_state + run + get_state. */
int vo_ba_solve(vo_ctx* ctx, const vo_ba_problem* prob, double* poses, double* points,
                int iters, double* cost_out);

/* Static plan statistics (for DESIGN.md/bench): fills up to n int64 values:
 * [0] chunks [1] segments [2] slab blocks [3] reduced blocks [4] profile
 * blocks [5] track entries [6] bytes read+written per GN iteration
 * (algorithmic) [7] banded solver in use [8] first-camera groups and
 * [9] chunks the last vo_ba_setup took over from the previous window's plan (the slide)
 * [10] observations per segment the plan was packed for (1: the one-wave K1's plan);
 * [11..22] host time of the last vo_ba_setup's sections in nanoseconds: stream sync, landmark
 * order and track entries, segments, lists and chunk images, the rest of planning, plan checks,
 * image uploads, reduction profile, uploads, buffers, banded-solver tables, attributes.
 * Returns count written. */
int vo_ba_plan_stats(vo_ctx* ctx, int64_t* out, int n);

/* Diagnostic only: in a stamped build of the library (make EXTRA=-DVO_BA_STAMPS=1), K1
 * and K3 record s_memtime phase stamps; returns per-phase shader-cycle sums over
 * all workgroups of the last K1 launch (load, backsub, linobs, reduce, elim,
 * schur_pairs, write, schur_cams, then two unused slots) followed by the K3 phase
 * cycles.  With n < 0 it instead writes up to -n raw per-segment values (10 per
 * segment, the last two the absolute start and end time of that workgroup).
 * Returns the count written (0 when stamps are off). */
int vo_ba_debug_stamps(vo_ctx* ctx, uint64_t* out, int n);

/* ---- kernel timing (HIP events on the context stream) ---------------------
 * When enabled, every kernel launch is bracketed by hipEventRecord on the
 * context stream.  vo_profile_read synchronises and returns, per kernel id,
 * the summed duration in ms and the launch count, then clears the records.
 * Ids: 0 ba_lin (K1), 1 ba_reduce (K2), 2 ba_solve (K3), 3 match_pack,
 *      4 match_i8 (MFMA sweep), 5 match_f32, 6 match_merge, 7 triangulate,
 *      8 pnp_hyp, 9 pnp_score, 10 pnp_final, 11 sift_pyramid (all upsample, blur
 *      and downsample launches of one call), 12 sift_extrema (all octaves),
 *      13 sift_orient, 14 sift_select (sort keys, segmented sort, duplicate removal,
 *      retainBest, compaction), 15 sift_desc, 16 match_rerank (the float path's exact
 *      re-rank; before it had an id of its own it was timed under match_merge),
 *      17 pnp_decide, 18 pnp_hyp_tail, 19 pnp_score_tail (large batches: the replay after
 *      the first hypotheses of every frame, then the rest for the frames still looping),
 *      20 ess_hyp, 21 ess_score (both: the first slice and the rest), 22 ess_decide,
 *      23 ess_final, 24 ess_pose (essential-matrix initialisation).
 * vo_match_gated's launches take existing ids: its clears and grid build (count, scan, fill)
 * count under 3 (match_pack), its gated search and unique filter under 5 (match_f32);
 * vo_match_segment's count the same way.
 * vo_ba_run_lm's K1, K2 and K3 launches count under 0, 1 and 2 as vo_ba_run's do; its step
 * decision (ba_lm_decide, which sums the cost partials in K2's order) counts under 1 too: with
 * K2 fused into K3's launch, the default on one rank, it is the only launch there. */
#define VO_PROFILE_KERNELS 25
int vo_profile_enable(vo_ctx* ctx, int on);
int vo_profile_read(vo_ctx* ctx, double* ms_out, int64_t* counts_out);

/* Host only: groups observations by landmark (the CSR that vo_ba_problem takes) from a
 * per-observation landmark index, as the keyframe window holds it (reference
 * src/modules/vo.py:252-288 builds the BA problem from the map's observation lists):
 * point_ptr (n_points + 1) and order (n_obs, stable: observations of one landmark keep the
 * caller's order), so that obs_cam[order] / obs_uv[order] are the problem's arrays.
 * With order == NULL it only checks that the observations are already grouped
 * (nondecreasing obs_pt, one pass) and fills point_ptr: returns 1 when they are not
 * (point_ptr then unspecified; call again with an order array).
 * VO_ERR_ARG if an index is out of range. */
int vo_ba_group_by_point(int n_points, int n_obs, const int32_t* obs_pt, int32_t* order, int32_t* point_ptr);
/* Host-only: builds the static plan of `prob` without a device (planner tests,
 * capacity checks).  Fills up to n int64 values: [0] chunks [1] segments
 * [2] slab blocks [3] profile blocks [4] track entries [5] max pairs in a chunk
 * [6] max window slots in a segment [7] max window cameras in a segment
 * [8] free poses F [9] widest profile row span (blocks) [10] two-sided K3
 * layout usable [11] its rows per side m [12] separator rows s [13] bottom rows. 
 * Returns the count written, or VO_ERR_ARG (vo_last_error() says why). */
int vo_ba_plan_probe(const vo_ba_problem* prob, int target_segments, int64_t* out, int n);
/* Host only: a 64-bit FNV-1a digest of every array of the static plan (chunks, segments,
 * slab layout, pair and camera lists, profile, K3 step tables) for `prob`; it pins the plan
 * (and so every kernel's summation order) across planner changes (tests/golden).  The plan is
 * packed for ceil(n_obs / target_segments) observations per segment. */
int vo_ba_plan_digest(const vo_ba_problem* prob, int target_segments, uint64_t* digest);

/* ---- triangulation ----------------------------------- */
/* Replaces triangulate_points (reference src/modules/frontend.py:115-148):
 * cv2.triangulatePoints(P1, P2, pts1.T, pts2.T) (DLT + SVD per point, float32
 * homogeneous output), dehomogenisation in float32, depth in camera 2 > min_depth
 * (:134-135) and the cv2.projectPoints reprojection error in image 2 <
 * max_reproj_err (:139-143).  P1, P2: 3x4 row-major K @ T_cw[:3, :] (as the caller
 * forms them, :127-128); T_cw2: 3x4 row-major [R | t]; K: 3x3 row-major.  pts1,
 * pts2: n x 2 float32.  Writes the float32 triangulation of EVERY point (n x 3) and
 * its mask (n bytes, 1 = kept); the reference returns pts3d[mask], mask.
 * Host buffers; synchronous. */
int vo_triangulate(vo_ctx* ctx, const double* P1, const double* P2, const double* T_cw2,
                   const double* K, const float* pts1, const float* pts2, int n,
                   double min_depth, double max_reproj_err, float* pts3d_out, uint8_t* mask_out);
/* Device-buffer variant (points and outputs in HBM; matrices on the host); enqueued
 * on the context stream, returns without synchronising. */
int vo_triangulate_async(vo_ctx* ctx, const double* P1, const double* P2, const double* T_cw2,
                         const double* K, const float* d_pts1, const float* d_pts2, int n,
                         double min_depth, double max_reproj_err, float* d_pts3d, uint8_t* d_mask);

/* ---- PnP-RANSAC ------------------------------------- */
/* Replaces cv2.solvePnPRansac(objpts, imgpts, K, None, reprojectionError=reproj_err,
 * iterationsCount=iterations, confidence=confidence) with SOLVEPNP_ITERATIVE, as the
 * tracking step calls it (reference src/modules/vo.py:135-141; map points and
 * keypoints are float32, vo.py:130-134).  objpts: n x 3 float32, imgpts: n x 2
 * float32, K: 3x3 row-major (no distortion).  RANSAC of OpenCV 4.12: cv::RNG((uint64)-1)
 * subsets of 5 points, EPnP per subset, float32 squared reprojection error <=
 * (float)(reproj_err^2), best = first model with the most inliers (> 4), the niters
 * update of RANSACUpdateNumIters; then a Levenberg-Marquardt refinement on the
 * inliers.  n == 5: EPnP on all points, all inliers.  n < 5: failure.
 * Outputs: rvec (3), tvec (3) (the pose T_cw, Rodrigues vector), mask (n bytes, 1 =
 * inlier of the best RANSAC model), *success_out = 1/0 (solvePnPRansac's retval).
 * Host buffers; synchronous. */
int vo_pnp_ransac(vo_ctx* ctx, const float* objpts, const float* imgpts, int n, const double* K,
                  int iterations, double reproj_err, double confidence, double* rvec_out,
                  double* tvec_out, uint8_t* mask_out, int32_t* success_out);
/* Batch of frames, points in HBM: frame f owns points offsets[f]..offsets[f+1]-1 of
 * d_objpts (total x 3) / d_imgpts (total x 2); offsets is a HOST array (batch+1,
 * offsets[0] = 0).  d_pose: (batch, 6) float64 = rvec, tvec; d_mask: (total) bytes;
 * d_status: (batch, 2) int32 = success, inlier count.  Enqueued on the context stream
 * (the subsets are regenerated and uploaded only when the frame layout changes). */
int vo_pnp_ransac_batch_async(vo_ctx* ctx, const float* d_objpts, const float* d_imgpts,
                              const int32_t* offsets, int batch, const double* K, int iterations,
                              double reproj_err, double confidence, double* d_pose, uint8_t* d_mask,
                              int32_t* d_status);
/* Host only: the RANSAC subsets the cv::RNG((uint64)-1) stream gives for `count` points
 * (iterations x 5 int32), for parity tests. */
int vo_pnp_subsets(int count, int iterations, int32_t* out);

/* ---- Essential-matrix initialisation (reference src/modules/vo.py:87-101) -- */
/* Replaces cv2.findEssentialMat(pts1, pts2, K, method=RANSAC, prob, threshold): five-point
 * RANSAC over the cv::RNG((uint64)-1) subsets vo_pnp_subsets draws, Sampson error, OpenCV's
 * loop bookkeeping, no refinement.  Host arrays, synchronous.  pts1/pts2: n x 2 float32 pixels,
 * K row-major 3x3.  E_out: row-major, unit Frobenius norm (zero on failure); mask_out[n]: 1 for
 * the inliers of E.  n < 5 or no model with more than 4 inliers: *success_out = 0, mask zero.
 * The models of a subset are tried in ascending order of the eliminated unknown (DESIGN.md
 * §Essential); for n == 5 the first model is returned, not OpenCV's stack of all of them. */
int vo_essential_ransac(vo_ctx* ctx, const float* pts1, const float* pts2, int n, const double* K, int max_iters,
                        double threshold, double prob, double* E_out, uint8_t* mask_out, int32_t* success_out,
                        int32_t* inliers_out);
/* Replaces cv2.recoverPose(E, pts1, pts2, K): the first of [R1|t] [R2|t] [R1|-t] [R2|-t] with the
 * most triangulated points in front of both cameras and nearer than distance_thresh (OpenCV:
 * 50).  R_out row-major, t_out unit, mask_out[n] 0/1, *good_out the count. */
int vo_recover_pose(vo_ctx* ctx, const double* E, const float* pts1, const float* pts2, int n, const double* K,
                    double distance_thresh, double* R_out, double* t_out, uint8_t* mask_out, int32_t* good_out);

/* ---- SIFT keypoint detection (the extrema stage) ----- */
/* Replaces the keypoint detection of cv2.SIFT_create(nfeatures, contrastThreshold,
 * edgeThreshold, sigma).detectAndCompute(gray, None) (reference
 * src/modules/frontend.py:27-32,55): doubled base image, Gaussian / DoG pyramid of
 * n_layers + 3 levels per octave, 26-neighbour extrema of DoG levels 1..n_layers beyond a
 * 5-pixel border with |v| > floor(0.5 contrast / n_layers * 255), adjustLocalExtrema
 * (sub-pixel fit, contrast and edge tests): the refined extrema before orientation
 * assignment (vo_sift_detect_and_compute below runs the whole call; this stage is exposed
 * for parity tests).  img: h x w uint8 row-major.
 * Per keypoint, in (octave, candidate level, row, column) order:
 *   kp_f[8]: x, y (input-image pixels), size, response, xi, 0, 0, 0
 *   kp_i[8]: image, OpenCV's octave word (first octave -1), candidate level, level,
 *            row, column (octave pixels, after refinement), candidate row, column.
 * *count receives the number found; at most `capacity` are written.  Host buffers. */
int vo_sift_detect(vo_ctx* ctx, const uint8_t* img, int h, int w, double contrast, double edge, double sigma,
                   int n_layers, int capacity, float* kp_f, int32_t* kp_i, int32_t* count);
/* Batch of equally sized images in HBM (d_imgs: batch x h x w uint8); keypoints of all
 * images appended to d_kpf / d_kpi in no particular order, *d_count (device int32) = total
 * found.  Enqueued on the context stream. */
int vo_sift_detect_batch_async(vo_ctx* ctx, const uint8_t* d_imgs, int batch, int h, int w, double contrast,
                               double edge, double sigma, int n_layers, int capacity, float* d_kpf,
                               int32_t* d_kpi, int32_t* d_count);
/* Parity/debug: the Gaussian (g_out) and DoG (d_out) pyramids of one image in the pitched
 * layout vo_sift_layout describes (g_floats / d_floats = capacities in floats). */
int vo_sift_pyramid(vo_ctx* ctx, const uint8_t* img, int h, int w, double sigma, int n_layers, float* g_out,
                    int64_t g_floats, float* d_out, int64_t d_floats);
/* ---- SIFT detectAndCompute ------------------------- */
/* One keypoint as cv::KeyPoint holds it after detectAndCompute: pt (x, y) and size in
 * input-image pixels, angle in degrees, response, OpenCV's octave word (first octave -1);
 * image = index in the batch. */
typedef struct vo_sift_keypoint {
  float x, y, size, angle, response;
  int32_t octave, image, reserved;
} vo_sift_keypoint;
/* Replaces cv2.SIFT_create(nfeatures, contrastThreshold, edgeThreshold, sigma)
 * .detectAndCompute(gray, None) (reference src/modules/frontend.py:27-32,55; OpenCV 4.12
 * sift.dispatch.cpp / sift.simd.hpp): the detection above, then calcOrientationHist (one
 * keypoint per histogram peak >= 0.8 max), KeyPointsFilter::removeDuplicatedSorted,
 * retainBest(nfeatures) when nfeatures > 0 (every keypoint whose response is >= the
 * nfeatures-th largest), and calcSIFTDescriptor (4 x 4 x 8, clipped at 0.2, scaled to 512,
 * saturate_cast<uchar>, stored as float).  Keypoints come out in removeDuplicatedSorted's
 * order (x asc, y asc, size desc, angle asc, response desc, octave desc); OpenCV's order
 * after retainBest is implementation-defined.  capacity is the size of
 * the output buffers; the oriented keypoints considered before the nfeatures cut start at
 * that capacity and the call retries with 4x more (up to 131072 per image) when they
 * overflow, as OpenCV has no such cap.  *count = the number written; VO_ERR_ARG when more
 * than 131072 oriented keypoints or more than capacity output keypoints.  Host buffers:
 * kps[capacity], desc[capacity x 128]. */
int vo_sift_detect_and_compute(vo_ctx* ctx, const uint8_t* img, int h, int w, int nfeatures, double contrast,
                               double edge, double sigma, int n_layers, int capacity, vo_sift_keypoint* kps,
                               float* desc, int32_t* count);
/* The same call with device outputs: FeatureFrontend.process_image's SIFT branch
 * (frontend.py:51-75) keeps only k.pt and the descriptors and moves both to config.device
 * (:66-67), so the drop-in writes them straight into the caller's GPU buffers (pointers of
 * this process's HIP runtime on the context's GPU, validated before any launch: VO_ERR_ARG
 * otherwise) and only *count crosses PCIe.  d_kps[capacity], d_desc[capacity x 128]. */
int vo_sift_detect_and_compute_dev(vo_ctx* ctx, const uint8_t* img, int h, int w, int nfeatures, double contrast,
                                   double edge, double sigma, int n_layers, int capacity, vo_sift_keypoint* d_kps,
                                   float* d_desc, int32_t* count);
/* Batch of equally sized images in HBM (d_imgs: batch x h x w uint8).  Per image b:
 * d_kps[b * capacity + i], d_desc[(b * capacity + i) * 128], i < d_counts[b]
 * (d_counts[b] < 0 when a capacity overflowed: -d_counts[b] is the working capacity that
 * image asked for, a lower bound when an earlier stage was cut short).  Enqueued on the
 * context stream. */
int vo_sift_detect_and_compute_batch_async(vo_ctx* ctx, const uint8_t* d_imgs, int batch, int h, int w,
                                           int nfeatures, double contrast, double edge, double sigma,
                                           int n_layers, int capacity, vo_sift_keypoint* d_kps, float* d_desc,
                                           int32_t* d_counts);
/* Host only: [n_octaves, G floats per image, DoG floats per image] then per octave
 * [h, w, pitch, G offset, DoG offset]; returns the count of values (writes up to n). */
int vo_sift_layout(int h, int w, int n_layers, int64_t* out, int n);

/* ---- KLT tracking (sparse pyramidal Lucas-Kanade) ------------------------ */
/* Tracks n points from img0 into img1 (h x w uint8, row-major): the structure of OpenCV's
 * calcOpticalFlowPyrLK (fixed-point patches, a double 2 x 2 solve), not its bits.  Build-defined:
 * the reference has no tracker.  The contract is DESIGN.md §KLT, restated in tests/klt_ref.py;
 * every sum over a window is an integer, so results do not depend on how the device computes them.
 *   Pyramid: level l + 1 is ((w_l + 1) / 2) x ((h_l + 1) / 2), each pixel
 *   (sum_{i,j=-2..2} k_i k_j I_l(2x+i, 2y+j) + 128) >> 8 with k = 1 4 6 4 1 and indices reflected
 *   without repeating the edge.  L_eff is the largest L <= opt->levels whose level L - 1 is at
 *   least (2r+3) x (2r+3), at least 1; a level 0 smaller than that gives every point status 1.
 *   Window: (2r+1)^2 pixels with corner q = c - r (float32), iq = floor(q), inside iff
 *   0 <= iq.x <= w_l - 2r - 2 and 0 <= iq.y <= h_l - 2r - 2 (a non-finite q is outside); bilinear
 *   weights x 16384 from the fractions, intensities x 32, Scharr derivatives, all integers.
 *   Per level from L_eff - 1 down to 0: the template at p0 * 2^-l, A = sum of derivative
 *   products (int64) scaled by 2^-20, minEig and D in double; a start window outside, or
 *   minEig < min_eig or D < FLT_EPSILON, skips the level (status 1 / 2 at level 0).  Then at most
 *   max_iters steps n += (float)delta from the integer mismatch sums, stopped by
 *   |delta|^2 <= eps^2 or OpenCV's oscillation rule; a window at n outside ends the level
 *   (status 3 at level 0, also for the final n).  err = (float)(sum |J - I| / (32 (2r+1)^2)) at
 *   the final n.
 *   Options: max_err > 0 gives status 5 to err > max_err.  VO_KLT_GUESS: pts1 holds the start of
 *   n on entry.  VO_KLT_FB: every accepted point is tracked back from img1 to img0 with p0 as the
 *   guess under the same options; a back track that fails, or ends with
 *   (double)dx*dx + (double)dy*dy > (double)fb_thresh*fb_thresh from p0, gives status 4.
 *   Status: 0 tracked, 1 start window outside, 2 degenerate texture, 3 left the image,
 *   4 forward-backward check failed, 5 err above max_err, 6 non-finite p0 or guess.  pts1 of a
 *   failed point is p0 and its err 0.  *n_tracked (optional, as err) counts status 0.
 * All arrays are host arrays: pts0, pts1 (n, 2) float32 pixels (x, y), status (n), err (n).  A
 * nonzero tag keys the context's device pyramid cache (at least 4 entries, keyed by
 * (tag, h, w, levels built), least recently used evicted): on a hit the image is neither uploaded
 * nor rebuilt and may be NULL; the caller changes the tag when the pixels change, as with
 * des0_tag.  Results never depend on the cache.
 *   VO_ERR_ARG (before the context or a device is touched): opt, pts1 or status NULL, pts0 NULL
 *   with n > 0, negative n, h < 1 or w < 1, a NULL image with tag 0, win_radius outside 1..15,
 *   levels outside 1..8, max_iters outside 1..100, a non-finite or negative eps, min_eig,
 *   fb_thresh or max_err, unknown flag bits, reserved != 0.  n == 0: VO_OK, *n_tracked = 0.
 * The kernels are not in the profiler's id table (tools/klt_timing.py times the call). */
#define VO_KLT_GUESS 1   /* pts1 holds the initial guess on entry */
#define VO_KLT_FB    2   /* forward-backward check */
typedef struct {
  int32_t win_radius;  /* 1..15 */
  int32_t levels;      /* 1..8 */
  int32_t max_iters;   /* 1..100 */
  float eps, min_eig, fb_thresh, max_err;
  int32_t flags;       /* VO_KLT_GUESS | VO_KLT_FB */
  int32_t reserved;    /* 0 */
} vo_klt_options;
int vo_klt_track(vo_ctx* ctx, const uint8_t* img0, uint64_t tag0, const uint8_t* img1, uint64_t tag1, int h, int w,
                 const float* pts0, float* pts1, int n, const vo_klt_options* opt, uint8_t* status, float* err,
                 int32_t* n_tracked);
/* Parity/debug: the pyramid of one image, levels concatenated and unpitched (cap = capacity of
 * out in bytes).  Levels are built while they are at least 3 x 3 (vo_klt_layout with
 * win_radius 0); *levels_out = how many. */
int vo_klt_pyramid(vo_ctx* ctx, const uint8_t* img, int h, int w, int levels, uint8_t* out, int64_t cap,
                   int32_t* levels_out);
/* Host only: [L_eff, bytes of the pyramid] then per level [h, w, byte offset]; returns the count
 * of values (writes up to n), or VO_ERR_ARG. */
int vo_klt_layout(int h, int w, int levels, int win_radius, int64_t* out, int n);

/* ---- Corners (Shi-Tomasi minimum-eigenvalue detector) ------------------- */
/* Corners of an h x w uint8 image (row-major), strongest first and at least min_distance apart:
 * the structure of OpenCV's goodFeaturesToTrack, not its bits, plus a set of existing points to
 * keep away from.  Build-defined; the contract is DESIGN.md §Corners, restated in
 * tests/corners_ref.py.  Every sum over a block is an integer, so results do not depend on how the
 * device computes them.
 *   Image: indices outside are reflected without repeating the edge (-1 -> 1, n -> n - 2, repeated
 *   as often as needed; an extent of 1 maps everything to 0).
 *   Gradient (int32, at every pixel through the reflection):
 *   gx = (I(x+1,y-1) + 2 I(x+1,y) + I(x+1,y+1)) - (I(x-1,y-1) + 2 I(x-1,y) + I(x-1,y+1)), gy alike along y.
 *   Block sums (int32): a = sum gx^2, b = sum gx gy, c = sum gy^2 over the (2k+1)^2 block centred on
 *   the pixel, k = block_radius, the gradient field read at reflected indices.
 *   Response: q = (int64)(a-c)^2 + 4 (int64)b^2; resp = (float)(0.5 * ((double)(a+c) - sqrt((double)q))),
 *   each operation rounded once, no contraction; defined for every pixel.
 *   Candidates: rmax = max resp over the pixels whose mask byte is nonzero (all without a mask); no
 *   corners unless rmax > 0.  A pixel is a candidate iff 1 <= x <= w-2, 1 <= y <= h-2, its mask byte
 *   is nonzero, (double)resp > (double)quality * (double)rmax, and resp >= the response of each of
 *   its 8 neighbours (the mask plays no part there; ties keep both).  h < 3 or w < 3: no corners, VO_OK.
 *   Order: resp descending, ties by y*w + x ascending.
 *   Selection, d = min_distance, d2 = (double)d*(double)d: walking the candidates in that order, one
 *   is rejected iff a keep-away point (kx, ky) (float32, both finite; others are ignored) has
 *   dx*dx + dy*dy < d2 with dx = (double)x - (double)kx (double, one rounding per operation), or an
 *   already accepted corner has (double)(Dx^2 + Dy^2) < d2 (an integer); else accepted.  The walk
 *   stops at max_corners accepted.  d = 0 rejects nothing.  Hence the result for max_corners = m
 *   is the first m rows of the result for any larger limit.
 *   Output: corners (n, 2) float32 (x, y) (integers), resp (n) (optional), *n_out, in order of acceptance.
 * All arrays are host arrays.  A nonzero tag looks the image up in the context's KLT pyramid cache
 * (level 0 of an entry with that tag, h and w): on a hit img may be NULL and nothing is uploaded; on
 * a miss the image goes into scratch and no entry is created.  Results never depend on the cache.
 *   VO_ERR_ARG (before the context or a device is touched): opt, corners or n_out NULL, keep NULL
 *   with n_keep > 0, negative n_keep, h < 1 or w < 1 or h*w > 2^30, a NULL image with tag 0,
 *   max_corners outside 1..h*w, block_radius outside 1..3, quality not finite or outside (0, 1],
 *   min_distance not finite or outside 0..1024, nonzero flags or reserved.
 * The kernels are not in the profiler's id table (tools/corner_timing.py times the call). */
typedef struct {
  int32_t max_corners;   /* 1..h*w */
  int32_t block_radius;  /* 1..3: blocks of 3 x 3, 5 x 5, 7 x 7 */
  float quality;         /* finite, > 0, <= 1 */
  float min_distance;    /* finite, 0..1024 */
  int32_t flags;         /* 0 */
  int32_t reserved;      /* 0 */
} vo_corner_options;
int vo_good_features(vo_ctx* ctx, const uint8_t* img, uint64_t tag, int h, int w, const uint8_t* mask,
                     const float* keep, int n_keep, const vo_corner_options* opt, float* corners, float* resp,
                     int32_t* n_out);
/* Parity/debug: the response map, h*w float32. */
int vo_corner_response(vo_ctx* ctx, const uint8_t* img, int h, int w, int block_radius, float* out);
/* The selection rule alone over caller-supplied candidates: xy (n, 2) int32 (each coordinate within
 * +-2^24), taken in the order resp descending (-0 as +0), ties by row index; out_idx (at least
 * min(n, max_corners)) receives the accepted rows in order of acceptance.  VO_ERR_ARG also for a
 * non-finite resp, a negative or non-finite distance (or one above 1024) and max_corners < 1.
 * n == 0: VO_OK, *n_out = 0, no device touched. */
int vo_corner_select(vo_ctx* ctx, const int32_t* xy, const float* resp, int n, const float* keep, int n_keep,
                     float min_distance, int max_corners, int32_t* out_idx, int32_t* n_out);
/* Debug: the context's last vo_good_features / vo_corner_select call: [candidates, selection
 * rounds that had something to decide, corners accepted, grid cell side]. */
int vo_corner_stats(vo_ctx* ctx, int32_t out[4]);

/* ---- BRIEF (steered binary descriptor) and the Hamming matcher ------------ */
/* A 256-bit descriptor of the 31 x 31 patch around a point of an h x w uint8 image: ORB's structure
 * (intensity-centroid direction, steered BRIEF over box sums), not its bits.  Build-defined; the
 * contract is restated in tests/brief_ref.py.  Every quantity is an integer, so results do not
 * depend on how the device computes them.
 *   Direction tables C[32], S[32] (int32): for k = 0..7, C[k] = rint(16384 cos(2 pi k / 32)),
 *   S[k] = rint(16384 sin(2 pi k / 32)); for k = 8..31, C[k] = -S[k-8], S[k] = C[k-8] (a quarter turn
 *   is exact).
 *   Base pattern, 256 tests (px, py, qx, qy): a 64-bit LCG s <- s * 6364136223846793005 +
 *   1442695040888963407 (mod 2^64) from s = 0x5EED; a draw is (s >> 33) % 9 - 4; a coordinate is the
 *   sum of three consecutive draws, drawn in the order px, py, qx, qy; a test is drawn again if
 *   px^2 + py^2 > 144, qx^2 + qy^2 > 144, p == q, or the 4-tuple was already taken.
 *   Rotated pattern P[32][256][4] (int8): rx = (x C[k] - y S[k] + 8192) >> 14,
 *   ry = (x S[k] + y C[k] + 8192) >> 14, the shift arithmetic (a floor).  Every |coordinate| <= 12;
 *   P[k+8] is (-y, x) of P[k].  (csrc/brief_pattern.h, written by tools/make_brief_pattern.py.)
 *   Per point (x, y), float32:
 *   1. Status 1 (zero descriptor, bin 0) if a coordinate is not finite or |coordinate| >= 2^24;
 *      else cx = (int)rintf(x), cy = (int)rintf(y) (half to even); status 1 if cx is outside
 *      [0, w-1] or cy outside [0, h-1]; else status 0.
 *   2. Patch: I(reflect(cx+dx, w), reflect(cy+dy, h)), dx, dy in [-15, 15], the reflection of the
 *      corner detector above (total for any extent): a corner at the border is described too.
 *   3. Moments (int32): m10 = sum dx I, m01 = sum dy I over dx^2 + dy^2 <= 225 (709 pixels).
 *   4. Bin: the k maximising (int64)m10 C[k] + (int64)m01 S[k], ties to the lowest k.
 *   5. Box sums: B(u, v) = sum of the 5 x 5 patch pixels centred (u, v), |u|, |v| <= 13.
 *   6. Bit t = B(P[k][t].p) < B(P[k][t].q), strictly, stored in word t / 32 at bit t % 32 of eight
 *      uint32 words.
 * pts (n, 2), des_out (n, 8), bin_out (n, optional) and status_out (n, optional) are host arrays.
 * tag is vo_good_features' tag: level 0 of a cached KLT pyramid entry with that tag, h and w is read
 * instead of img (which may then be NULL); the cache is only read; results never depend on it.
 * n == 0: VO_OK, no device touched.  flags must be 0.
 *   VO_ERR_ARG (before the context or a device is touched): des_out NULL, pts NULL with n > 0, a
 *   NULL image with tag 0, h < 1, w < 1, h*w > 2^30, n < 0, nonzero flags.
 * The kernels are not in the profiler's id table (tools/brief_timing.py times the calls). */
int vo_brief_describe(vo_ctx* ctx, const uint8_t* img, uint64_t tag, int h, int w, const float* pts, int n, int flags,
                      uint32_t* des_out, int32_t* bin_out, uint8_t* status_out);
/* The tables: out = P as int8 [32][256][4], dir_out = C[32] then S[32].  Needs no context. */
int vo_brief_pattern(int8_t out[32 * 256 * 4], int32_t dir_out[64]);

/* Brute-force Hamming matching of binary rows: des0 (n0, words), des1 (n1, words) uint32, words in
 * 1..16; d(i, j) = sum over the words of popcount(a_w ^ b_w).
 *   Top-2 per query under keys (d, j): equal distances keep the lower j.  knn_idx (n0, 2) and
 *   knn_dist (n0, 2) (both optional) receive them, -1 and INT32_MAX where no neighbour exists.
 *   A query with fewer than two neighbours emits no pair (as vo_match_knn2_ratio).  (i, j1) is kept
 *   iff (max_dist == 0 or d1 <= max_dist) and (double)d1 < ratio * (double)d2.  With
 *   VO_MATCH_HAMMING_MUTUAL a kept pair survives iff i has the smallest key (d(i', j1), i') over all
 *   query rows i'.  Pairs come out in ascending query order: out_pairs (capacity 2 * n0 int32),
 *   out_dist (n0, optional) their distances, *out_count their number.
 *   VO_MATCH_DEVICE_PTRS: des0 and des1 are device pointers of this process's HIP runtime on the
 *   context's GPU (as in vo_match_mutual); every output is a host array.
 *   VO_ERR_ARG (before any launch; the options' and the shapes' checks need no device): opt,
 *   out_pairs or out_count NULL, a NULL array with a nonzero size, negative sizes, words outside
 *   1..16, a ratio that is not finite or negative, a negative max_dist, unknown flag bits, nonzero
 *   reserved.
 * Results do not depend on how the device splits the work: every distance is an integer. */
#define VO_MATCH_HAMMING_MUTUAL 4
typedef struct {
  double ratio;      /* finite, >= 0 */
  int32_t max_dist;  /* >= 0; 0: no limit */
  int32_t flags;     /* VO_MATCH_DEVICE_PTRS | VO_MATCH_HAMMING_MUTUAL */
  int32_t reserved;  /* 0 */
} vo_match_hamming_options;
int vo_match_hamming(vo_ctx* ctx, const uint32_t* des0, int n0, const uint32_t* des1, int n1, int words,
                     const vo_match_hamming_options* opt, int32_t* out_pairs, int32_t* out_dist, int32_t* out_count,
                     int32_t* knn_idx, int32_t* knn_dist);

/* ---- multi-GPU (landmark sharding + RCCL all-reduce) --------------------- */
/* 128-byte RCCL unique id, created on rank 0 and shared by the caller. */
int vo_comm_unique_id(char out[128]);
/* Attaches an RCCL communicator to the context (one process per GPU).  After
 * this, vo_ba_setup expects THIS rank's landmark shard: every rank passes all
 * n_poses cameras but only its own points/observations; each GN iteration
 * all-reduces the partial reduced camera system (S, b, cost) before the
 * redundant dense pose solve, so all ranks hold identical poses. */
int vo_comm_init(vo_ctx* ctx, int nranks, int rank, const char id[128]);
/* (The test-only loopback communicator is declared in vo_hip_testing.h.) */

#ifdef __cplusplus
}
#endif
#endif /* VO_HIP_H */
