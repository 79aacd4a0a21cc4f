// Arguments and host launches of the observation-weight kernels in ba_weights.hip
// (vo_ba_set_obs_weights, vo_ba_cull; DESIGN.md §Observation weights and culling), called by the
// BA engine (ba_engine.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "ba_kernels.h"

namespace vo {

// The Huber delta a weighted session without a robust cost runs the kRobust code under: no
// finite whitened residual reaches it, so every scale is 1 and rho = n^2.
constexpr double kWeightedNoHuber = 1e150;

// The weighted one-wave K1: mode is kBacksub | kAccum | kLm as launch_lin takes it (kRobust and
// kWeighted are implied; A.huber > 0 always, kWeightedNoHuber for the plain cost), sqw holds
// sqrt(w) in the plan's observation order.  Returns false, launching nothing, for a layout or
// mode without a weighted instantiation (the four-wave K1, wave_chunks = 0, among them).
bool launch_lin_weighted(const LinArgs& A, const double* sqw, int mode, int wave_chunks, int grid, hipStream_t st);
bool lin_weighted_covers(int wave_chunks);

// The cull (vo_hip.h vo_ba_cull): ba_cull_obs_kernel, one lane per observation in the problem's
// order with ba_obs_residual_kernel's arithmetic, deactivates by the chi^2, depth and finiteness
// rules; ba_cull_track_kernel, one lane per landmark, then walks the landmark's CSR track and
// deactivates what is left of a track shorter than min_track.  Both write w (problem order),
// sqw_obs (problem order) and sqw_plan (plan order: obs_pos[o]) with plain stores; count[0]
// (culled) and count[1] (active afterwards) are integer atomics, zeroed before the launch.
struct CullArgs {
  int n_obs, n_points, min_track;
  double fx, fy, cx, cy, max_chi2, min_depth;
  const int* obs_cam;     // problem order: camera
  const int* obs_pt;      // problem order: landmark in the plan's internal order
  const float2* obs_uv;   // problem order: measurement
  const int* obs_pos;     // problem order: position in the plan's observation order
  const int* point_ptr;   // problem order CSR (n_points + 1)
  const double* poses;    // 12 per camera
  const double* points;   // 3 per landmark, internal order
  double* w;              // n_obs, problem order
  double* sqw_obs;        // n_obs, problem order
  double* sqw_plan;       // n_obs, plan order
  int* count;             // [culled, active]
};
void launch_cull(const CullArgs& A, hipStream_t st);

// n doubles set to v (a session's first cull starts from all ones).
void launch_fill(double* p, int n, double v, hipStream_t st);

}  // namespace vo
