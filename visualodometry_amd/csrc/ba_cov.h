// Arguments and host launches of the covariance read-out kernels in ba_cov.hip
// (vo_ba_covariance), called by the BA engine (ba_engine.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace vo {

// Pose marginals: S (K2's layout in sys) is gathered into the dense lower triangle L, factored
// over its envelope by one workgroup, and solved against the identity, one workgroup per block
// column; cov receives the whole symmetric inverse.
struct CovPoseArgs {
  int F;              // free poses; n = 6F
  const int* first;   // BAPlan::prof_first (F)
  const int* off;     // BAPlan::prof_off (F + 1)
  const int* last;    // BAPlan::prof_last (F)
  const int* dst;     // per profile block: offset of its 36 values in sys (| kRedTranspose)
  const double* sys;  // K2's output
  double* L;          // (6F, 6F) row-major; zeroed before the launch, the factor's lower triangle after it
  double* cov;        // (6F, 6F) row-major
  int* fail;          // out: 0, or 1 + the block column whose pivot test failed
};
size_t cov_solve_lds_bytes(int F);
constexpr size_t kCovSolveLdsMax = 160 * 1024;  // gfx950: LDS per workgroup
void launch_cov_factor(const CovPoseArgs& A, hipStream_t st);
void launch_cov_solve(const CovPoseArgs& A, hipStream_t st);  // reads *A.fail: nothing is written after a failure

// Landmark marginals, one lane per landmark in the problem's order.
struct CovPointArgs {
  int n_points, n_fixed, F;
  double fx, fy, cx, cy, lambda, huber, huber2;
  const int* point_ptr;   // problem order CSR (n_points + 1)
  const int* pt_inv;      // problem landmark -> the plan's internal landmark
  const int* obs_cam;     // problem order: camera
  const float2* obs_uv;   // problem order: measurement
  const double* poses;    // 12 per camera
  const double* points;   // 3 per landmark, internal order
  const double* cov;      // (6F, 6F) pose covariance
  const double* sqrt_w;   // problem order: sqrt of the observation weights; null: a session without weights
  double* out;          // 9 per landmark, problem order; NaN for a frozen landmark
};
void launch_cov_points(const CovPointArgs& A, hipStream_t st);

}  // namespace vo
