// The BA engine's host arithmetic (ba_engine.hip): K2's output layout and its inverse, the
// problem-order tables of the read-outs, the chunk-image runs of a setup, reserve()'s synthetic
// window, the LM log's layout, vo_ba_run_lm's options, the host-only planning entries' plan and
// vo_ba_group_by_point's grouping.  Host only -- a plan and plain ints in,
// plain vectors out, no HIP -- so csrc/ba_tables_check.cpp runs all of it without a GPU
// (tests/test_ba_tables.py).  The tables are filled in place: the engine keeps them across
// sessions (their capacity is reused, and some are the sources of asynchronous copies).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/vo_hip.h"
#include "ba_plan.h"

namespace vo {

constexpr int kTabTranspose = 1 << 30;  // ReduceLayout::dst flag: the block is stored transposed (kRedTranspose)

// K2's output layout -- the profile [S | b | cost], or the banded K3's columns (ba_band.h
// BandArgs) --, its per-block table and the fused launch's readiness table.
struct ReduceLayout {
  std::vector<int32_t> dst, rdst;  // per profile block / free camera: offset of its 36 / 6 values in sys
  // K2's per-block table (ReduceArgs): meta, four ints a block -- slab rows [x, y), on a diagonal
  // block its camera's rhs slab entries [z, w), else -1 --, and out, two -- dst and the rhs offset
  std::vector<int32_t> meta, out;
  // the fused launch's readiness counters: the column each profile block's reducer stores into
  // (top columns j of rows i < top, then bottom column F - 1 - i at top + F - 1 - i), the cost
  // at F, and how many items each counter waits for
  std::vector<int32_t> col, col_need;
  size_t sys_len = 0;
  long cost_off = 0;
};
// Band layout: block bandwidth w, top = m + s rows eliminated top-down (ba_band.h BandSplit),
// col_stride = band_col_stride(w).
void reduce_layout(const BAPlan& P, bool band_on, int w, int top, int col_stride, ReduceLayout& L);
// sys as K2 wrote it, back to the dense symmetric S (6F x 6F) and b (6F); either may be null.
void dense_system(const BAPlan& P, const ReduceLayout& L, const double* sys, double* S_out, double* b_out);

// The problem-order observation arrays, rebuilt from the plan's internal-order copies (pt: the
// landmark in the plan's order).  The plan must have its observation order (obs_order.size() >= n_obs).
void obs_tables(const BAPlan& P, std::vector<int32_t>& cam, std::vector<int32_t>& pt, std::vector<float>& uv);
// The problem-order CSR and the problem landmark -> internal landmark map.
void csr_tables(const BAPlan& P, std::vector<int32_t>& ptr, std::vector<int32_t>& inv);
// Problem observation -> plan position.
void obs_positions(const BAPlan& P, std::vector<int32_t>& pos_of);

// The plan's chunk images as runs of consecutive chunks: taken over from the previous plan's
// chunks src .. src + count - 1, or built by this plan (src = -1).
struct ImageRun {
  int src, dst, count;
};
void image_runs(const BAPlan& P, std::vector<ImageRun>& runs);

// A synthetic window of about n_obs observations: landmark p seen by a run of consecutive
// cameras, the runs spread over the window.
struct ReserveWindow {
  std::vector<int32_t> point_ptr, obs_cam;
};
ReserveWindow reserve_window(int n_poses, int n_points, int64_t n_obs);

// The log of an LM run of n iterations, as byte offsets: cost (n + 1), lambda (n + 1), trial (n)
// doubles, then the n decisions (ints) and the two control words of a stop (trials, reason).
struct LmLog {
  int n;
  size_t cost_off() const { return 0; }
  size_t lambda_off() const { return ((size_t)n + 1) * 8; }
  size_t trial_off() const { return 2 * ((size_t)n + 1) * 8; }
  size_t accepted_off() const { return (3 * (size_t)n + 2) * 8; }
  size_t stop_off() const { return accepted_off() + std::max(1, n) * sizeof(int); }
  size_t bytes() const { return stop_off() + 2 * sizeof(int); }
  // The first n_asked iterations of the log (doubles: the bytes before accepted_off(); acc: the
  // decisions).  f: the first iteration without a verdict -- the failed one, or the first behind
  // a stop, whose cost and damping (the stopped state's) every later entry repeats; a failed
  // iteration's trial and decision and every later entry are NaN / 0.  Any output may be null.
  void decode(const double* doubles, const int* acc, int n_asked, int f, bool stopped, double* cost_out,
              double* lambda_out, double* trial_out, uint8_t* accepted_out) const;
};

// vo_ba_run_lm's options with the defaults filled in (vo_hip.h; lambda0 from the problem's
// lambda); returns the message of the first bad field, empty if none.
std::string lm_options(const vo_ba_lm_options* opt, double problem_lambda, vo_ba_lm_options& o);

// vo_ba_setup_prior's argument checks (vo_hip.h; no device needed): the message of the first bad
// field of the prior against its problem, empty if none.
std::string pose_prior_error(const vo_ba_problem* prob, const vo_ba_pose_prior* prior);

// vo_ba_setup_factors' argument checks (vo_hip.h; no device needed): the message of the first bad
// field of the factor list against its problem, empty if none.
std::string pose_factor_error(const vo_ba_problem* prob, const vo_ba_pose_factor* factors, int n_factors);
// The factors' free-camera indices (FactorRows::fi / fj, ba_plan.h build_profile): camera - n_fixed,
// -1 for a fixed camera and for a unary factor's cam_j.
void factor_free_cams(int n_fixed, const vo_ba_pose_factor* factors, int n_factors, FactorRows& rows);
// A between factor on free poses couples them: first[max] drops to at most min.
void factor_lower_first(const FactorRows& rows, std::vector<int32_t>& first);
// vo_ba_marginalize's rule: a factor is marginalised iff one of its cameras is among the dropped
// 0 .. n_drop - 1 (the factor kernel applies the same test on the device).
inline bool factor_marginalised(int cam_i, int cam_j, int n_drop) {
  return cam_i < n_drop || (cam_j >= 0 && cam_j < n_drop);
}

// A problem planned on the host alone (vo_ba_plan_digest, vo_ba_plan_probe, vo_ba_testing_plan_slide):
// build_plan, then the profile of the plan's own first[].  Returns build_plan's message, empty if
// the plan was built.
std::string plan_window(BAPlan& P, const vo_ba_problem* prob, int seg_obs, const BAPlan* prev = nullptr,
                        int seg_chunks = 1);

// vo_ba_group_by_point (vo_hip.h): the CSR point_ptr (n_points + 1) of obs_pt and, with order,
// the stable permutation that groups the observations by landmark.  Without order the input must
// be grouped already (nondecreasing): grouped tells whether it was, and point_ptr is written only
// then.  Returns the message of the first bad argument, empty if none.
std::string group_by_point(int n_points, int n_obs, const int32_t* obs_pt, int32_t* order, int32_t* point_ptr,
                           bool& grouped);

}  // namespace vo
