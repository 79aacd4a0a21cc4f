// Pose prior of the bundle adjustment (vo_ba_setup_prior, DESIGN.md §Pose prior).
//
//   ba_prior_kernel  once per linearisation, behind K1 and ahead of K2, one workgroup: one lane per
//                    prior pose takes xi_f = log(T_f T0_f^-1) from the device-resident poses; one
//                    the block-row matvec (Lambda xi)_r, strided partial sums in fixed order; then
//                    the slab sources of the prior -- eta - Lambda xi to the cameras' extra rhs rows,
//                    Lambda's blocks to the extra slab rows of the leading triangle (on a session's
//                    first launch only: they do not change) -- and the
//                    cost term cost0 - 2 eta^T xi + xi^T Lambda xi by lane-strided partial sums and a
//                    fixed tree.  K2 then adds them in its own fixed order (ba_plan.h build_profile).
// In the same launch, factor_blocks(n) more workgroups take a session's pose factors
// (vo_ba_setup_factors, DESIGN.md §Pose factors): one lane per factor forms A = T_i T_j^-1 (or T_i),
// xi = log(A Z^-1) by the prior's log, G = Ad(A), and writes Lambda, G^T Lambda G, -Lambda G,
// -Lambda xi and G^T Lambda xi to the factor's own slab and rhs rows; the workgroup's cost
// sum xi^T Lambda xi by a fixed tree to its own cost entry.
// Every sum runs in a fixed order; no atomics.  IEEE sqrt, division and atan2: none of this is on a
// solve's chain.
#include "ba_prior.h"

#include <algorithm>

#include "ba_math.h"
#include "ba_reduce.h"
#include "vo_common.h"

namespace vo {

namespace {

constexpr int kPriorThreads = 256;

// A = sin(th)/th, B = (1 - cos(th))/th^2, C = (th - sin(th))/th^3: se3_exp_apply's own values
// (ba_math.h: the same series below kExpSeriesTh2, the same closed forms above it), restated so
// that the log below inverts the update map it was given, and that function keeps its code.
__device__ __forceinline__ void exp_coeffs(double th2, double& A, double& B, double& C) {
  if (th2 < kExpSeriesTh2) {
    constexpr double cA[8] = {1.0, -1.0 / 6, 1.0 / 120, -1.0 / 5040, 1.0 / 362880, -1.0 / 39916800,
                              1.0 / 6227020800.0, -1.0 / 1307674368000.0};
    constexpr double cB[8] = {1.0 / 2, -1.0 / 24, 1.0 / 720, -1.0 / 40320, 1.0 / 3628800, -1.0 / 479001600,
                              1.0 / 87178291200.0, -1.0 / 20922789888000.0};
    constexpr double cC[8] = {1.0 / 6, -1.0 / 120, 1.0 / 5040, -1.0 / 362880, 1.0 / 39916800,
                              -1.0 / 6227020800.0, 1.0 / 1307674368000.0, -1.0 / 355687428096000.0};
    A = cA[7];
    B = cB[7];
    C = cC[7];
#pragma unroll
    for (int k = 6; k >= 0; --k) {
      A = __builtin_fma(A, th2, cA[k]);
      B = __builtin_fma(B, th2, cB[k]);
      C = __builtin_fma(C, th2, cC[k]);
    }
  } else {
    const double th = sqrt(th2);
    double s, c;
    sincos(th, &s, &c);
    const double it = 1.0 / th, it2 = it * it;
    A = s * it;
    B = (1.0 - c) * it2;
    C = (th - s) * (it2 * it);
  }
}

// xi = (rho, phi) with exp(xi) T0 = T (poses as vo_ba_set_state lays them out: R row-major, t):
// D = T T0^-1 = [R R0^T | t - R R0^T t0]; the axis times sin(th) from D's skew part, th by atan2
// against (tr - 1) / 2, phi = skew part / A; rho solves V(phi) rho = D's translation with the V the
// exp map builds (3x3, by cofactors).  Rotations of less than pi.
__device__ __forceinline__ void se3_log_rel(const double* T, const double* T0, double (&xi)[6]) {
  double D[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) D[3 * i + j] = T[3 * i] * T0[3 * j] + T[3 * i + 1] * T0[3 * j + 1] + T[3 * i + 2] * T0[3 * j + 2];
  const double t0 = T[9] - (D[0] * T0[9] + D[1] * T0[10] + D[2] * T0[11]);
  const double t1 = T[10] - (D[3] * T0[9] + D[4] * T0[10] + D[5] * T0[11]);
  const double t2 = T[11] - (D[6] * T0[9] + D[7] * T0[10] + D[8] * T0[11]);
  const double v0 = 0.5 * (D[7] - D[5]), v1 = 0.5 * (D[2] - D[6]), v2 = 0.5 * (D[3] - D[1]);
  const double c = 0.5 * (D[0] + D[4] + D[8] - 1.0);
  const double s = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
  const double th = atan2(s, c);
  double A, B, C;
  exp_coeffs(th * th, A, B, C);
  const double p0 = v0 / A, p1 = v1 / A, p2 = v2 / A;
  const double P[9] = {0, -p2, p1, p2, 0, -p0, -p1, p0, 0};
  double V[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double P2 = P[3 * i] * P[j] + P[3 * i + 1] * P[3 + j] + P[3 * i + 2] * P[6 + j];
      V[3 * i + j] = (i == j ? 1.0 : 0.0) + B * P[3 * i + j] + C * P2;
    }
  const double c00 = V[4] * V[8] - V[5] * V[7], c01 = V[5] * V[6] - V[3] * V[8], c02 = V[3] * V[7] - V[4] * V[6];
  const double c10 = V[2] * V[7] - V[1] * V[8], c11 = V[0] * V[8] - V[2] * V[6], c12 = V[1] * V[6] - V[0] * V[7];
  const double c20 = V[1] * V[5] - V[2] * V[4], c21 = V[2] * V[3] - V[0] * V[5], c22 = V[0] * V[4] - V[1] * V[3];
  const double det = V[0] * c00 + V[1] * c01 + V[2] * c02;
  xi[0] = (c00 * t0 + c10 * t1 + c20 * t2) / det;
  xi[1] = (c01 * t0 + c11 * t1 + c21 * t2) / det;
  xi[2] = (c02 * t0 + c12 * t1 + c22 * t2) / det;
  xi[3] = p0;
  xi[4] = p1;
  xi[5] = p2;
}

// LDS, all of it dynamic (prior_lds_bytes is the kernel's whole LDS, which setup holds against the
// 64 KiB a launch gets without an attribute): xi (6K) | Lambda xi (6K) | the matvec's partial sums
// (max(6K, kPriorThreads)) | the cost tree (kPriorThreads)
__device__ __forceinline__ void prior_terms(const PriorArgs& A, double* prior_lds) {
  const int K = A.K, n = 6 * K, tid = threadIdx.x;
  const double* __restrict__ info = A.info;
  const double* __restrict__ rhs = A.rhs;
  double* xi = prior_lds;
  double* lx = prior_lds + n;
  double* part = prior_lds + 2 * n;
  double* cpart = part + max(n, kPriorThreads);
  // Lambda's blocks (i, j), j <= i, row-major as K1 writes a window slot: once per session (nothing
  // else writes those slab rows), the loads in flight beside the logs below
  if (A.stage) {
    const int nblk = K * (K + 1) / 2;
    for (int e = tid; e < 36 * nblk; e += kPriorThreads) {
      const int b = e / 36, q = e % 36;
      int i = 0;
      while ((i + 1) * (i + 2) / 2 <= b) ++i;
      const int j = b - i * (i + 1) / 2;
      A.slab[36l * A.blk_row[b] + q] = info[(long)(6 * i + q / 6) * n + 6 * j + q % 6];
    }
  }
  if (A.status && *A.status) return;  // (uniform; behind the staging, which no failure may skip)
  for (int f = tid; f < K; f += kPriorThreads) {
    double x[6];
    se3_log_rel(A.poses + 12l * (A.n_fixed + f), A.poses0 + 12l * f, x);
#pragma unroll
    for (int a = 0; a < 6; ++a) xi[6 * f + a] = x[a];
  }
  __syncthreads();
  // (Lambda xi)_r: np lanes per row, lane (r, q) sums columns q, q + np, ... in order (Lambda is
  // symmetric, so it walks column r's rows: consecutive lanes, consecutive addresses), eight loads
  // in flight at a time as K2's row sums keep theirs (clamped index, a column past the end adds
  // +0.0); then the row's np partial sums in order
  const int np = n >= kPriorThreads ? 1 : kPriorThreads / n;
  for (int r0 = 0; r0 < n; r0 += kPriorThreads) {  // (one pass unless 6K > kPriorThreads)
    const int r = np > 1 ? tid % n : r0 + tid, q = np > 1 ? tid / n : 0;
    if (r < n && q < np) {
      double acc = 0.0;
      for (int c = q; c < n; c += 8 * np) {
        double v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = info[(long)min(c + i * np, n - 1) * n + r];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc += c + i * np < n ? v[i] * xi[min(c + i * np, n - 1)] : 0.0;
      }
      part[q * n + r] = acc;
    }
  }
  __syncthreads();
  for (int r = tid; r < n; r += kPriorThreads) {
    double acc = 0.0;
    for (int q = 0; q < np; ++q) acc += part[q * n + r];
    lx[r] = acc;
    A.slab_b[6l * A.cam_row[r / 6] + r % 6] = rhs[r] - acc;
  }
  __syncthreads();
  // the cost term: lane-strided partial sums in order, then a fixed tree
  double c = 0.0;
  for (int r = tid; r < n; r += kPriorThreads) c += xi[r] * (lx[r] - 2.0 * rhs[r]);
  cpart[tid] = c;
  __syncthreads();
  for (int m = kPriorThreads / 2; m > 0; m >>= 1) {
    if (tid < m) cpart[tid] += cpart[tid + m];
    __syncthreads();
  }
  if (tid == 0) *A.cost = A.cost0 + cpart[0];
}

// One lane per factor, everything of it in registers; the workgroup's cost by a fixed tree.
__device__ __forceinline__ void factor_terms(const FactorArgs& A, int blk, double* cpart) {
  const int tid = threadIdx.x, f = blk * kFactorThreads + tid, n = A.n;
  if (A.status && *A.status) return;  // (uniform)
  double cost = 0.0;
  if (f < n) {
    const int ci = A.cams[f], cj = A.cams[n + f];
    const int* __restrict__ rows = A.rows + 5l * f;
    const int r_ii = rows[0], r_jj = rows[1], r_ij = rows[2], rb_i = rows[3], rb_j = rows[4];
    const double* __restrict__ dat = A.data + f;
    const bool live = A.n_drop <= 0 || ci < A.n_drop || (cj >= 0 && cj < A.n_drop);
    double Z[12], L[36], T[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) Z[e] = dat[(long)e * n];
#pragma unroll
    for (int e = 0; e < 36; ++e) L[e] = live ? dat[(long)(12 + e) * n] : 0.0;
    const double* Ti = A.poses + 12l * ci;
    if (cj >= 0) {  // A = T_i T_j^-1 = [R_i R_j^T | t_i - R_A t_j]
      const double* Tj = A.poses + 12l * cj;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) T[3 * r + c] = Ti[3 * r] * Tj[3 * c] + Ti[3 * r + 1] * Tj[3 * c + 1] + Ti[3 * r + 2] * Tj[3 * c + 2];
#pragma unroll
      for (int r = 0; r < 3; ++r) T[9 + r] = Ti[9 + r] - (T[3 * r] * Tj[9] + T[3 * r + 1] * Tj[10] + T[3 * r + 2] * Tj[11]);
    } else {
#pragma unroll
      for (int e = 0; e < 12; ++e) T[e] = Ti[e];
    }
    double xi[6], lx[6];
    se3_log_rel(T, Z, xi);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      double acc = 0.0;
#pragma unroll
      for (int c = 0; c < 6; ++c) acc += L[6 * r + c] * xi[c];
      lx[r] = acc;
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) cost += xi[r] * lx[r];
    if (!live) cost = 0.0;  // (a residual that is not finite must not reach a sum it is no part of)
    if (r_ii >= 0) {
#pragma unroll
      for (int q = 0; q < 36; ++q) A.slab[36l * r_ii + q] = L[q];
#pragma unroll
      for (int r = 0; r < 6; ++r) A.slab_b[6l * rb_i + r] = live ? -lx[r] : 0.0;
    }
    if (r_jj >= 0) {
      // G = Ad(A) = [[R, [t]x R], [0, R]]; LG = Lambda G; G^T LG, its lower triangle mirrored
      const double X[9] = {0, -T[11], T[10], T[11], 0, -T[9], -T[10], T[9], 0};
      double G[36];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          G[6 * r + c] = T[3 * r + c];
          G[6 * (r + 3) + c + 3] = T[3 * r + c];
          G[6 * (r + 3) + c] = 0.0;
          G[6 * r + c + 3] = X[3 * r] * T[c] + X[3 * r + 1] * T[3 + c] + X[3 * r + 2] * T[6 + c];
        }
      double LG[36];
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          double acc = 0.0;
#pragma unroll
          for (int k = 0; k < 6; ++k) acc += L[6 * r + k] * G[6 * k + c];
          LG[6 * r + c] = acc;
        }
#pragma unroll
      for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = 0; c <= r; ++c) {
          double acc = 0.0;
#pragma unroll
          for (int k = 0; k < 6; ++k) acc += G[6 * k + r] * LG[6 * k + c];
          A.slab[36l * r_jj + 6 * r + c] = acc;
          A.slab[36l * r_jj + 6 * c + r] = acc;
        }
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) acc += G[6 * k + r] * lx[k];
        A.slab_b[6l * rb_j + r] = live ? acc : 0.0;
      }
      // block (i, j) of S is -Lambda G: stored as the layout has it, rows the later camera's
      if (r_ij >= 0) {
        const bool tr = ci < cj;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
          for (int c = 0; c < 6; ++c) A.slab[36l * r_ij + (tr ? 6 * c + r : 6 * r + c)] = -LG[6 * r + c];
      }
    }
  }
  cpart[tid] = cost;
  __syncthreads();
  for (int m = kFactorThreads / 2; m > 0; m >>= 1) {
    if (tid < m) cpart[tid] += cpart[tid + m];
    __syncthreads();
  }
  if (tid == 0) A.cost[blk] = cpart[0];
}

static_assert(kFactorThreads == kPriorThreads, "one launch: the prior's workgroup and the factors' share a block size");
__global__ __launch_bounds__(kPriorThreads) void ba_prior_kernel(PriorArgs A, FactorArgs Fa) {
  extern __shared__ __attribute__((aligned(16))) double prior_lds[];
  const int pb = A.K > 0 ? 1 : 0;
  if ((int)blockIdx.x < pb) prior_terms(A, prior_lds);
  else factor_terms(Fa, blockIdx.x - pb, prior_lds);
}

// ---- vo_ba_marginalize ---------------------------------------------------------------------
constexpr int kMargThreads = 256;
constexpr int kMargMaskThreads = 128;

// One lane per landmark (problem order): in P_D iff one of its active observations is in a dropped
// camera; then the masked sqrt(w) of all its observations at their plan positions -- the session's
// own for P_D, 0 for the rest, which K1 then leaves out by its select.
__global__ __launch_bounds__(kMargMaskThreads) void ba_marg_mask_kernel(MargMaskArgs A) {
  const int p = blockIdx.x * kMargMaskThreads + threadIdx.x;
  if (p >= A.n_points) return;
  const int o0 = A.point_ptr[p], o1 = A.point_ptr[p + 1];
  bool in = false;
  for (int o = o0; o < o1; ++o) in = in || (A.obs_cam[o] < A.n_drop && (!A.sqw_obs || A.sqw_obs[o] > 0.0));
  A.mask[p] = in ? 1 : 0;
  for (int o = o0; o < o1; ++o) A.sqw_plan[A.obs_pos[o]] = in ? (A.sqw_obs ? A.sqw_obs[o] : 1.0) : 0.0;
}

// S from K2's layout to a dense symmetric matrix (ba_cov.hip's gather, both triangles), and b.
// One lane per row of the lower triangle; the scratch was zeroed.
__global__ __launch_bounds__(kMargThreads) void ba_marg_gather_kernel(MargArgs A) {
  const int idx = blockIdx.x * kMargThreads + threadIdx.x;
  const long n = 6l * A.F;
  if (idx >= n) return;
  const int i = idx / 6, r = idx % 6;
  const int f0 = A.first[i], b0 = A.off[i];
  for (int j = f0; j <= i; ++j) {
    const int d = A.dst[b0 + j - f0];
    const double* blk = A.sys + (d & ~kRedTranspose);
    const bool tr = d & kRedTranspose;
    const int cmax = j == i ? r : 5;
    for (int c = 0; c <= cmax; ++c) {
      const double v = blk[tr ? 6 * c + r : 6 * r + c];
      A.dense[idx * n + 6 * j + c] = v;
      A.dense[(6l * j + c) * n + idx] = v;
    }
  }
  A.bvec[idx] = A.sys[A.rdst[i] + r];
}

// The Schur complement of the ne = 6m eliminated rows onto the nr = 6 (F - m) remaining ones.
// Every workgroup factors the eliminated block (+ lambda) and solves the whole panel
// Y = L^-1 [S_er | b_e] in its own LDS, in the same fixed order (so all hold the same bits and the
// same pivot verdict without a hand-off); the trailing update info = S_rr - Y^T Y, rhs = b_r - Y^T y
// is dealt by rows over the workgroups, each entry one lane's sum over the eliminated rows in order,
// the lower triangle computed and mirrored.
// LDS, all of it dynamic (marg_lds_bytes is the kernel's whole LDS): L (ne x ne) |
// Y (ne x (nr + 1), the last column y) | the pivot verdict (one slot)
__global__ __launch_bounds__(kMargThreads) void ba_marg_kernel(MargArgs A) {
  extern __shared__ __attribute__((aligned(16))) double marg_lds[];
  const int tid = threadIdx.x;
  const int ne = 6 * A.m, nr = 6 * (A.F - A.m);
  const long n = 6l * A.F;
  double* L = marg_lds;
  double* Y = marg_lds + (long)ne * ne;
  const int yw = nr + 1;
  int& s_fail = *reinterpret_cast<int*>(Y + (long)ne * yw);
  if (tid == 0) s_fail = 0;
  for (int e = tid; e < ne * ne; e += kMargThreads) {
    const int i = e / ne, j = e % ne;
    L[e] = A.dense[i * n + j] + (i == j ? A.lambda : 0.0);
  }
  __syncthreads();
  for (int j = 0; j < ne; ++j) {
    const double d = L[j * ne + j];
    const bool ok = d > 0.0 && !__builtin_isinf(d);  // (uniform: every lane reads the same value)
    if (!ok) {
      if (tid == 0) s_fail = j + 1;
      break;
    }
    const double l = sqrt(d);
    __syncthreads();  // every lane has read the pivot
    for (int i = j + tid; i < ne; i += kMargThreads) L[i * ne + j] = i == j ? l : L[i * ne + j] / l;
    __syncthreads();
    for (int e = tid; e < (ne - j - 1) * (ne - j - 1); e += kMargThreads) {
      const int i = j + 1 + e / (ne - j - 1), c = j + 1 + e % (ne - j - 1);
      if (c <= i) L[i * ne + c] -= L[i * ne + j] * L[c * ne + j];
    }
    __syncthreads();
  }
  __syncthreads();
  if (s_fail) {  // (uniform)
    if (blockIdx.x == 0 && tid == 0) *A.fail = s_fail;
    return;
  }
  // the panel: one lane per column (the remaining rows' and b's), forward substitution in order
  for (int c = tid; c < yw; c += kMargThreads) {
    for (int k = 0; k < ne; ++k) {
      double s = c < nr ? A.dense[k * n + ne + c] : A.bvec[k];
      for (int q = 0; q < k; ++q) s -= L[k * ne + q] * Y[q * yw + c];
      Y[k * yw + c] = s / L[k * ne + k];
    }
  }
  __syncthreads();
  for (int r = blockIdx.x; r < nr; r += gridDim.x) {
    for (int c = tid; c <= r; c += kMargThreads) {
      double s = A.dense[(ne + r) * n + ne + c];
      for (int k = 0; k < ne; ++k) s -= Y[k * yw + r] * Y[k * yw + c];
      A.info[(long)r * nr + c] = s;
      A.info[(long)c * nr + r] = s;
    }
    if (tid == 0) {
      double s = A.bvec[ne + r];
      for (int k = 0; k < ne; ++k) s -= Y[k * yw + r] * Y[k * yw + nr];
      A.rhs[r] = s;
    }
  }
  if (blockIdx.x == 0 && tid == 0) *A.fail = 0;
}

}  // namespace

size_t marg_lds_bytes(int F, int m) {
  const size_t ne = 6ull * m, nr = 6ull * (F - m);
  return (ne * ne + ne * (nr + 1) + 2) * sizeof(double);  // (16 bytes for the verdict: the block stays 16-byte sized)
}

void launch_marg_mask(const MargMaskArgs& A, hipStream_t st) {
  if (A.n_points <= 0) return;
  hipLaunchKernelGGL(ba_marg_mask_kernel, dim3((A.n_points + kMargMaskThreads - 1) / kMargMaskThreads),
                     dim3(kMargMaskThreads), 0, st, A);
}

void launch_marg_gather(const MargArgs& A, hipStream_t st) {
  if (A.F <= 0) return;
  hipLaunchKernelGGL(ba_marg_gather_kernel, dim3((6 * A.F + kMargThreads - 1) / kMargThreads), dim3(kMargThreads), 0,
                     st, A);
}

// The dynamic-LDS limit beyond the default 64 KiB belongs to the current device: set on every such call.
void launch_marg(const MargArgs& A, hipStream_t st) {
  if (A.F - A.m <= 0) return;
  const size_t lds = marg_lds_bytes(A.F, A.m);
  if (lds > 64 * 1024)
    VO_HIP_CHECK(hipFuncSetAttribute((const void*)ba_marg_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int grid = std::min(64, 6 * (A.F - A.m));
  hipLaunchKernelGGL(ba_marg_kernel, dim3(grid), dim3(kMargThreads), lds, st, A);
}

size_t prior_lds_bytes(int K) {
  return (12ull * K + std::max<size_t>(6ull * K, kPriorThreads) + kPriorThreads) * sizeof(double);
}

void launch_prior(const PriorArgs& A, const FactorArgs& F, hipStream_t st) {
  const int grid = (A.K > 0 ? 1 : 0) + factor_blocks(F.n);
  if (grid <= 0) return;
  const size_t lds = std::max(A.K > 0 ? prior_lds_bytes(A.K) : 0, F.n > 0 ? kFactorThreads * sizeof(double) : 0);
  hipLaunchKernelGGL(ba_prior_kernel, dim3(grid), dim3(kPriorThreads), lds, st, A, F);
}

}  // namespace vo
