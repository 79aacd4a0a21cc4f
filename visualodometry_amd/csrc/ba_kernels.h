// Arguments and host launches of the BA kernels in ba.hip (K1, K2, the profile K3, the chunk
// image copy), called by the BA engine (ba_engine.hip).  The banded K3: ba_band.h.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "ba_plan.h"
#include "ba_reduce.h"

namespace vo {

// Diagnostic build only (make EXTRA=-DVO_BA_STAMPS=1): per-phase s_memtime stamps of K1
// and the profile K3.  The product build executes none.
#ifndef VO_BA_STAMPS
#define VO_BA_STAMPS 0
#endif
constexpr bool kBaStamps = VO_BA_STAMPS != 0;
constexpr int kPhCount = 16;  // values per K1 stamp row (ba.hip kPh*)
constexpr int kS3Count = 10;  // values of the profile K3's stamp row (ba.hip kS3*)

// K1 modes: back-substitute the pending step, linearise and accumulate the Schur blocks; kRobust
// selects the Huber instantiations (LinArgs::huber > 0), the other four are the plain-cost kernels.
// kLm (Levenberg-Marquardt step control, vo_ba_run_lm): the damping is read from the device
// (LinArgs::lm_lambda) instead of LinArgs::lambda; instantiated for the two modes the LM loop
// needs it in, kAccum and kBacksub alone (the cost-only kernel uses no damping), plain and kRobust.
// kWeighted (per-observation weights, vo_ba_set_obs_weights / vo_ba_cull): the one-wave K1 reads
// sqrt(w) per observation; instantiated in ba_weights.hip for the modes a weighted session
// launches, always with kRobust (a session without Huber runs that code under a delta no whitened
// residual reaches), so the kernels above keep their code and their arguments.
enum { kBacksub = 1, kAccum = 2, kRobust = 4, kLm = 8, kWeighted = 16 };

struct LinArgs {
  int n_fixed;
  double fx, fy, cx, cy, lambda;
  const int4* chunk_hdr;  // kChunkHdr ints per chunk (BAPlan::chunk_hdr)
  const ChunkImg* chunk_img;  // BAPlan::chunk_img
  const int* slab_pos;        // BAPlan::slab_pos (window slot -> slab row)
  const int* cam_pos;         // BAPlan::cam_pos (window camera -> rhs slab row)
  const int* seg_hdr;     // kSegHdr ints per segment (BAPlan::seg_hdr)
  double* points;
  double* slab;
  double* slab_b;
  double* slab_cost;
  const double* pose_old;  // linearisation of the pending step (back-substitution)
  const double* pose_new;  // current linearisation point
  const double* dc;        // pending pose update (6 per free camera)
  const int* status;
  unsigned long long* stamps;  // diagnostic build only: per segment phase cycles
  int nseg;                    // segments
  double huber, huber2;        // Huber delta (pixels) and delta^2; read by the kRobust modes only
  const double* lm_lambda;     // the damping on the device; read by the kLm modes only
};
// One workgroup per segment (grid): the one-wave K1 of wave_chunks (1 .. kWaveMaxChunks) chunks
// per segment, or the four-wave K1 (wave_chunks = 0).
void launch_lin(const LinArgs& A, int mode, int wave_chunks, int grid, hipStream_t st);

// K2: nprof + 1 workgroups (the last sums the cost), or 1 with nprof = 0: the cost alone.
// (A.lm_lambda set: the instantiation that reads the camera damping from the device)
void launch_reduce(const ReduceArgs& A, int workgroups, hipStream_t st);

// K3: profile Cholesky solve S dc = b + pose update.
struct SolveArgs {
  int F, nprof, n_poses, n_fixed, iter_tag;
  int max_panel, max_row_span;  // most panel blocks in a column; max k - first[k]
  long lds_kf, lds_y, lds_panel, lds_pose, lds_tab;  // LDS offsets in doubles (solve_lds_layout)
  SolveTableLayout tl;
  const int* tab;      // BAPlan::solve_tab
  double* cost_out;    // if set: receives the cost of this linearisation (sys tail)
  double* sys;         // [S profile | b | cost]; factorised in place on the global path
  double* dc;          // 6F out
  const double* pose_cur;
  double* pose_next;
  int* status;
  unsigned long long* stamps;  // diagnostic build only
};

struct SolveLds {
  size_t prof, kf, y, panel, pose, tab, total;
};
constexpr size_t kSolveLdsMax = 160 * 1024 - 64;  // gfx950: 160 KiB per workgroup (+ s_fail)
// LDS image: [profile 36*nprof (LDS path)] [per column: L 21 + pad 3 | r 6 | y'/x 6]
// [y 6F] [4 private panels, 36 doubles per block] [step table ints]
inline SolveLds solve_lds_layout(bool lds_profile, int nprof, int F, int max_panel, int tab_len,
                                 int n_poses) {
  SolveLds L;
  L.prof = 0;
  L.kf = lds_profile ? 36ull * nprof : 0;
  L.y = L.kf + 36ull * F;
  L.panel = L.y + 6ull * F;
  L.pose = L.panel + 4ull * 36 * std::max(1, max_panel);
  L.tab = L.pose + 12ull * n_poses;
  L.total = L.tab * 8 + 4ull * std::max(1, tab_len);
  return L;
}
// lds_profile: the profile is LDS resident (the layout it was sized with); lds_bytes its total.
void launch_profile_solve(const SolveArgs& A, bool lds_profile, size_t lds_bytes, hipStream_t st);
void profile_solve_set_attributes(size_t lds_bytes);  // (a no-op unless the LDS size grows)

// Per-observation read-out (ba_obs_residual_kernel): the raw squared reprojection error and the
// camera-frame depth of every observation at the given state, in the problem's observation order.
struct ObsResidualArgs {
  int n_obs;
  double fx, fy, cx, cy;
  const int* obs_cam;     // problem order: camera
  const int* obs_pt;      // problem order: landmark in the plan's internal order
  const float2* obs_uv;   // problem order: measurement
  const double* poses;    // 12 per camera
  const double* points;   // 3 per landmark, internal order
  double* err2;           // n_obs out
  double* depth;          // n_obs out
};
void launch_obs_residual(const ObsResidualArgs& A, hipStream_t st);

// Step control of vo_ba_run_lm (ba_lm_decide_kernel), one launch per trial step.  Every workgroup
// sums the trial state's cost partials (slab_cost, K2's cost order) and takes the same decision
// from the log's entries of iteration k, which no workgroup of the launch writes: accepted
// (t < c) the points become the new snapshot, rejected they are restored from it and pose_next
// (the trial poses) is overwritten with pose_cur; workgroup 0 appends entry k + 1 to the log.
// k < 0: the initial cost, lambda0 and the first snapshot.  Nothing is written once *status is set.
//
// Termination (vo_ba_set_lm_stop; the kStop instantiation, launched only when a criterion is set):
// workgroup 0 also tests the decision against ftol / xtol / max_rejects (vo_hip.h) and on a stop
// writes stop[0] = k + 1, stop[1] = the reason and the status word kLmStatusStopped | (k + 1), so
// every later launch of the run goes quiet through its own status test.  A workgroup of this very
// launch that starts late may already see that word: carrying the launch's own tag it counts as
// zero there, so the workgroup still makes its copies.  ba_lm_finish, enqueued behind the last
// trial, zeroes a status word that is exactly a stop word (no failure tag, no timeout flag).
constexpr int kLmStatusStopped = 1 << 29;  // beside kBandStatusTimeout (ba_band.h); low bits: trials
enum { kLmRanAll = 0, kLmFtol = 1, kLmXtol = 2, kLmRejects = 3 };  // vo_hip.h VO_BA_LM_*
struct LmDecideArgs {
  int k, nseg, n_points, n_poses;
  double lambda0, up, down, lambda_min, lambda_max;
  const double* slab_cost;
  double* cost;        // log: accepted-state cost, iters + 1
  double* lambda;      // log: damping, iters + 1 (entry k is what iteration k's kernels read)
  double* trial;       // log: trial cost, iters
  int* accepted;       // log: decision, iters
  double* points;      // 3 per landmark: the trial state's on entry, the accepted state's on exit
  double* snap;        // the accepted state's landmarks
  const double* pose_cur;  // the accepted poses
  double* pose_next;       // the trial poses
  int* status;
  // read by the kStop instantiation only
  double ftol, xtol;   // 0: not tested
  int max_rejects;     // 0: not tested
  int n_dc;            // 6 per free camera
  const double* dc;    // the pose update K3 wrote for trial k
  int* stop;           // control words behind the log: [trials, reason]
};
int lm_decide_grid(int n_points);
void launch_lm_decide(const LmDecideArgs& A, bool stop, hipStream_t st);
void launch_lm_finish(int* status, hipStream_t st);

// Runs of consecutive chunk images copied from the previous plan's device images (ba.hip
// ba_img_copy_kernel); they travel in the arguments.
constexpr int kImgRuns = 48;
struct ImgRuns {
  int n;                    // runs in this launch
  int src[kImgRuns], dst[kImgRuns], end[kImgRuns];  // run r: chunks [end[r-1], end[r]) of the launch
};
void launch_img_copy(const uint4* prev, uint4* cur, const ImgRuns& R, int chunks, hipStream_t st);

}  // namespace vo
