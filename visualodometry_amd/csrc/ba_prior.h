// Pose prior of the bundle adjustment (vo_ba_setup_prior, DESIGN.md §Pose prior): arguments and
// launches of ba_prior.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace vo {

// The prior over free poses 0 .. K-1: E = cost0 - 2 eta^T xi + xi^T Lambda xi, xi_f the se(3) log of
// T_f T0_f^-1.  It enters the reduced system as slab sources of its own (ba_plan.h build_profile,
// prior_k): the kernel writes Lambda's blocks to the extra slab row of every block of the leading
// triangle, eta - Lambda xi to the extra rhs row of each of its cameras and E to the cost entry
// behind the segments', and K2 (any form of it) sums them with K1's in its fixed order.
struct PriorArgs {
  int K = 0, n_fixed = 0;  // K 0: no prior
  int stage;             // write Lambda's blocks to their slab rows (a session's first launch)
  double cost0;
  const double* info;    // (6K, 6K) Lambda, symmetric (the host mirrored the lower triangle)
  const double* rhs;     // (6K) eta
  const double* poses0;  // (K, 12) linearisation poses
  const double* poses;   // (n_poses, 12) the window's current poses
  const int* blk_row;    // per block (i, j), j <= i < K, at i (i + 1) / 2 + j: its slab row
  const int* cam_row;    // per camera f < K: its rhs slab row
  double* slab;
  double* slab_b;
  double* cost;          // the prior's entry of slab_cost
  const int* status;     // a failed earlier step: nothing is written (may be null)
};

// vo_ba_marginalize (ba_prior.hip): the marking kernel's and the dense kernels' arguments.
struct MargMaskArgs {
  int n_points, n_drop;
  const int* point_ptr;   // problem-order CSR
  const int* obs_cam;     // problem order
  const int* obs_pos;     // problem observation -> plan position
  const double* sqw_obs;  // sqrt(w) in problem order, null: all ones
  double* sqw_plan;       // out: the masked sqrt(w) in plan order (0 outside P_D)
  unsigned char* mask;    // out: 1 for a landmark of P_D, problem order
};
struct MargArgs {
  int F, m;              // free poses, eliminated leading free poses
  double lambda;         // on the eliminated pose blocks
  // K2's layout of S and b (the covariance tables) and its output
  const int* first;
  const int* off;
  const int* dst;
  const int* rdst;
  const double* sys;
  double* dense;         // (6F, 6F) scratch: S, symmetric
  double* bvec;          // (6F) scratch: b
  double* info;          // out (6R, 6R), R = F - m
  double* rhs;           // out (6R)
  int* fail;             // out: 1 + the eliminated row whose pivot failed, 0: none
};
size_t marg_lds_bytes(int F, int m);
constexpr size_t kMargLdsMax = 160 * 1024;
void launch_marg_mask(const MargMaskArgs& A, hipStream_t st);
void launch_marg_gather(const MargArgs& A, hipStream_t st);
void launch_marg(const MargArgs& A, hipStream_t st);

// Pose factors (vo_ba_setup_factors, DESIGN.md §Pose factors): factor k's residual is the twist
// xi = log(A Z^-1), A = T_i T_j^-1 (between) or T_i (unary); it adds xi^T Lambda xi to the cost and,
// with G = Ad(A), Lambda / G^T Lambda G / -Lambda G to the blocks (i, i) / (j, j) / (i, j) of S and
// -Lambda xi / G^T Lambda xi to b_i / b_j, as slab sources of its own (ba_plan.h build_profile, fac).
constexpr int kFactorThreads = 256;  // one lane per factor; one cost entry per workgroup
struct FactorArgs {
  int n = 0;           // factors (0: none)
  int n_drop = 0;      // > 0 (vo_ba_marginalize): factors without a camera among 0 .. n_drop - 1 write zeros
  const int* cams;     // (2n) cam_i (n) | cam_j (n): window cameras, cam_j -1 for a unary factor
  const int* rows;     // (5n) per factor: slab rows of (i, i), (j, j), (max, min); rhs rows of i, j; -1: none
  const double* data;  // (48n) entry e of factor f at e n + f: Z (12, a pose) | Lambda (36, mirrored)
  const double* poses; // (n_poses, 12) the window's current poses
  double* slab;
  double* slab_b;
  double* cost;        // the factors' entries of slab_cost: one per workgroup
  const int* status;   // a failed earlier step: nothing is written (may be null)
};
inline int factor_blocks(int n) { return (n + kFactorThreads - 1) / kFactorThreads; }

size_t prior_lds_bytes(int K);
constexpr size_t kPriorLdsMax = 64 * 1024;
// One launch for both: workgroup 0 the prior's terms (A.K > 0), factor_blocks(F.n) more the factors'.
void launch_prior(const PriorArgs& A, const FactorArgs& F, hipStream_t st);

}  // namespace vo
