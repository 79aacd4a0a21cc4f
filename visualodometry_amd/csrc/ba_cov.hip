// Covariance read-out of the bundle adjustment (vo_ba_covariance).
//
// The reduced camera system S of a linearisation (K1 + K2, ba.hip) is inverted densely:
//   ba_cov_factor_kernel  gathers S from K2's layout into a dense lower triangle and factors it,
//                         S = L L^T, by a right-looking block Cholesky over the envelope
//                         (one workgroup: the block columns are a dependent chain; every lane
//                         factors the diagonal block in registers, the panel goes through LDS,
//                         two barriers per column);
//   ba_cov_solve_kernel   one workgroup per block column J: L Y = E_J, L^T X = Y, rows >= J only;
//                         the lower triangle of S^-1 is stored and mirrored, so the matrix is
//                         symmetric bit for bit;
//   ba_cov_points_kernel  one lane per landmark in the problem's order: re-linearises the track,
//                         V (+ lambda), K1's pivot test, V^-1, and
//                         V^-1 + sum over pairs of free observations Y_o^T Sigma_{c(o) c(o')} Y_o'
//                         with Y_o = W_o V^-1, the 6x6 blocks read from the dense inverse.
// Every sum runs in a fixed order in one lane; no atomics.  IEEE sqrt and division throughout: the
// inverse amplifies rounding by the condition of S and V, and none of this is on a solve's chain.
#include "ba_cov.h"

#include "ba_math.h"
#include "ba_reduce.h"
#include "vo_common.h"

namespace vo {

namespace {

constexpr int kCovFactorThreads = 256;
constexpr int kCovSolveThreads = 64;
constexpr int kCovPointThreads = 128;
constexpr double kCovPivotRelEps = 1e-12;  // K1's point-block pivot threshold (ba_lin_wave.h kPivotRelEps)

// LDS: the current column's panel, 6 doubles per row below the diagonal block (at most 6F rows)
__global__ __launch_bounds__(kCovFactorThreads) void ba_cov_factor_kernel(CovPoseArgs A) {
  extern __shared__ __attribute__((aligned(16))) double cov_lds[];  // (no static LDS in front of it)
  const int F = A.F, tid = threadIdx.x;
  const long n = 6l * F;
  double* panel = cov_lds;
  // S from K2's layout: row 6i + r of the lower triangle, blocks first[i] .. i
  for (int idx = tid; idx < 6 * F; idx += kCovFactorThreads) {
    const int i = idx / 6, r = idx % 6;
    const int f0 = A.first[i], b0 = A.off[i];
    double* row = A.L + idx * n;
    for (int j = f0; j <= i; ++j) {
      const int d = A.dst[b0 + j - f0];
      const double* blk = A.sys + (d & ~kRedTranspose);
      const bool tr = d & kRedTranspose;
      const int cmax = j == i ? r : 5;
      for (int c = 0; c <= cmax; ++c) row[6 * j + c] = blk[tr ? 6 * c + r : 6 * r + c];
    }
  }
  __syncthreads();
  int fail = 0;
  for (int k = 0; k < F; ++k) {
    const long kk = 6l * k;
    // every lane factors the diagonal block in registers: all read the same values (the block is
    // not written between the barrier above and the one below), so the pivot verdict is uniform
    double a[21];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int c = 0; c <= i; ++c) a[P6(i, c)] = A.L[(kk + i) * n + kk + c];
    const int m = 6 * (A.last[k] - k);  // rows below the diagonal block that column k reaches
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const double d = a[P6(j, j)];
      ok = ok && d > 0.0 && !__builtin_isinf(d);
      const double l = sqrt(ok ? d : 1.0);
      a[P6(j, j)] = l;
#pragma unroll
      for (int i = j + 1; i < 6; ++i) a[P6(i, j)] /= l;
#pragma unroll
      for (int i = j + 1; i < 6; ++i)
#pragma unroll
        for (int c = j + 1; c <= i; ++c) a[P6(i, c)] -= a[P6(i, j)] * a[P6(c, j)];
    }
    if (!ok) {  // (uniform)
      fail = k + 1;
      break;
    }
    // panel: rows of L_ik = S_ik L_kk^-T, to the factor and to LDS (zero where row i starts later)
    for (int t = tid; t < m; t += kCovFactorThreads) {
      const long i = kk + 6 + t;
      double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (A.first[i / 6] <= k) {
        double* p = A.L + i * n + kk;
#pragma unroll
        for (int c = 0; c < 6; ++c) v[c] = p[c];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          double s = v[c];
#pragma unroll
          for (int q = 0; q < c; ++q) s -= a[P6(c, q)] * v[q];
          v[c] = s / a[P6(c, c)];
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) p[c] = v[c];
      }
#pragma unroll
      for (int c = 0; c < 6; ++c) panel[6 * t + c] = v[c];
    }
    __syncthreads();
    // the factored block goes to memory only behind the barrier: before it, lanes of other waves
    // may still be loading the unfactored block above.  Nothing in this kernel reads it again
    // (the solve kernel does); entry tid of the packed triangle
    if (tid < 21) {
      int i = 0;
      while (P6(i + 1, 0) <= tid) ++i;
      A.L[(kk + i) * n + kk + (tid - P6(i, 0))] = pick(a, tid);
    }
    // trailing update: S_ij -= L_ik L_jk^T over the panel's rows, lower triangle
    for (int t = tid; t < m * m; t += kCovFactorThreads) {
      const int ri = t / m, ci = t % m;
      if (ci > ri) continue;
      const long i = kk + 6 + ri, j = kk + 6 + ci;
      if (A.first[i / 6] > k || A.first[j / 6] > k) continue;
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < 6; ++q) s += panel[6 * ri + q] * panel[6 * ci + q];
      A.L[i * n + j] -= s;
    }
    __syncthreads();  // the next column reads what this one updated, and rewrites the panel
  }
  if (tid == 0) *A.fail = fail;
}

// LDS: X (6F rows of 6) | T (36)
__global__ __launch_bounds__(kCovSolveThreads) void ba_cov_solve_kernel(CovPoseArgs A) {
  extern __shared__ __attribute__((aligned(16))) double cov_lds[];  // (no static LDS in front of it)
  if (*A.fail) return;  // (uniform; the host fills the outputs)
  const int F = A.F, J = blockIdx.x, lane = threadIdx.x;
  const long n = 6l * F;
  const int r = lane / 6, c = lane % 6;
  const bool active = lane < 36;
  double* X = cov_lds;
  double* T = cov_lds + 36l * F;
  // forward: Y_I = L_II^-1 (E_I - sum_K L_IK Y_K), I = J .. F-1 (Y_I = 0 above J)
  for (int I = J; I < F; ++I) {
    // the diagonal block for the six solving lanes, in flight beside the row sums' loads
    double ld[21];
    if (lane < 6) {
      const double* Ld = A.L + (6l * I) * n + 6l * I;
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int q = 0; q <= i; ++q) ld[P6(i, q)] = Ld[i * n + q];
    }
    if (active) {
      double acc = (I == J && r == c) ? 1.0 : 0.0;
      const int K0 = max(A.first[I], J);
      const double* Lr = A.L + (6l * I + r) * n;
      for (int K = K0; K < I; ++K)
#pragma unroll
        for (int t = 0; t < 6; ++t) acc -= Lr[6 * K + t] * X[(6 * K + t) * 6 + c];
      T[lane] = acc;
    }
    __syncthreads();
    if (lane < 6) {
      double y[6];
#pragma unroll
      for (int rr = 0; rr < 6; ++rr) {
        double s = T[rr * 6 + lane];
#pragma unroll
        for (int q = 0; q < rr; ++q) s -= ld[P6(rr, q)] * y[q];
        y[rr] = s / ld[P6(rr, rr)];
      }
#pragma unroll
      for (int rr = 0; rr < 6; ++rr) X[(6 * I + rr) * 6 + lane] = y[rr];
    }
    __syncthreads();
  }
  // backward: X_I = L_II^-T (Y_I - sum_{K > I} L_KI^T X_K), I = F-1 .. J
  for (int I = F - 1; I >= J; --I) {
    // the diagonal block for the six solving lanes, in flight beside the row sums' loads
    double ld[21];
    if (lane < 6) {
      const double* Ld = A.L + (6l * I) * n + 6l * I;
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int q = 0; q <= i; ++q) ld[P6(i, q)] = Ld[i * n + q];
    }
    if (active) {
      double acc = X[(6 * I + r) * 6 + c];
      const int last = A.last[I];
      for (int K = I + 1; K <= last; ++K) {
        if (A.first[K] > I) continue;
        const double* Lk = A.L + (6l * K) * n + 6l * I + r;
#pragma unroll
        for (int t = 0; t < 6; ++t) acc -= Lk[t * n] * X[(6 * K + t) * 6 + c];
      }
      T[lane] = acc;
    }
    __syncthreads();
    if (lane < 6) {
      double x[6];
#pragma unroll
      for (int rr = 5; rr >= 0; --rr) {
        double s = T[rr * 6 + lane];
#pragma unroll
        for (int q = rr + 1; q < 6; ++q) s -= ld[P6(q, rr)] * x[q];
        x[rr] = s / ld[P6(rr, rr)];
      }
#pragma unroll
      for (int rr = 0; rr < 6; ++rr) X[(6 * I + rr) * 6 + lane] = x[rr];
    }
    __syncthreads();
    // one triangle, mirrored
    if (active && (I > J || r >= c)) {
      const double v = X[(6 * I + r) * 6 + c];
      const long i = 6l * I + r, j = 6l * J + c;
      A.cov[i * n + j] = v;
      A.cov[j * n + i] = v;
    }
  }
}

// Jacobians of observation o of a landmark at X: K1's arithmetic (ba_lin_wave.h obs_lin_w), the
// Huber scale on both.  jp: 2x3 (world point), jc: 2x6 (left twist), row-major.
template <bool kJc>
__device__ __forceinline__ void cov_obs_lin(const CovPointArgs& A, int o, int cam, double X0, double X1, double X2,
                                            double (&jp)[6], double (&jc)[12]) {
  const double* T = A.poses + 12l * cam;
  const double x = T[0] * X0 + T[1] * X1 + T[2] * X2 + T[9];
  const double y = T[3] * X0 + T[4] * X1 + T[5] * X2 + T[10];
  const double z = T[6] * X0 + T[7] * X1 + T[8] * X2 + T[11];
  const double iz = rcp_nr(z);
  double j00 = A.fx * iz, j02 = -A.fx * x * iz * iz;
  double j11 = A.fy * iz, j12 = -A.fy * y * iz * iz;
  // observation weights: K1's order (obs_lin_w) -- sqrt(w) on the residual and the Jacobians, a
  // zero weight a select, then the Huber rule on the whitened residual
  const bool weighted = A.sqrt_w != nullptr;
  const double sw = weighted ? A.sqrt_w[o] : 1.0;
  const bool on = sw > 0.0;
  if (weighted) {
    j00 = on ? j00 * sw : 0.0; j02 = on ? j02 * sw : 0.0;
    j11 = on ? j11 * sw : 0.0; j12 = on ? j12 * sw : 0.0;
  }
  if (A.huber > 0.0) {
    const float2 m = A.obs_uv[o];
    double r0 = A.fx * x * iz + A.cx - (double)m.x;
    double r1 = A.fy * y * iz + A.cy - (double)m.y;
    if (weighted) {
      r0 = on ? r0 * sw : 0.0;
      r1 = on ? r1 * sw : 0.0;
    }
    double rho;
    const double s = huber_scale(r0, r1, A.huber, A.huber2, rho);
    j00 *= s; j02 *= s; j11 *= s; j12 *= s;
  }
  jp[0] = j00 * T[0] + j02 * T[6];
  jp[1] = j00 * T[1] + j02 * T[7];
  jp[2] = j00 * T[2] + j02 * T[8];
  jp[3] = j11 * T[3] + j12 * T[6];
  jp[4] = j11 * T[4] + j12 * T[7];
  jp[5] = j11 * T[5] + j12 * T[8];
  if (kJc) {
    jc[0] = j00; jc[1] = 0.0; jc[2] = j02; jc[3] = j02 * y; jc[4] = j00 * z - j02 * x; jc[5] = -j00 * y;
    jc[6] = 0.0; jc[7] = j11; jc[8] = j12; jc[9] = j12 * y - j11 * z; jc[10] = -j12 * x; jc[11] = j11 * x;
  }
}

// Y = W V^-1 (6x3) of observation o: W = Jc^T Jp; vi = V^-1 packed (00 01 02 11 12 22).
__device__ __forceinline__ void cov_obs_y(const CovPointArgs& A, int o, int cam, double X0, double X1, double X2,
                                          const double (&vi)[6], double (&Y)[18]) {
  double jp[6], jc[12];
  cov_obs_lin<true>(A, o, cam, X0, X1, X2, jp, jc);
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const double w0 = jc[a] * jp[0] + jc[6 + a] * jp[3];
    const double w1 = jc[a] * jp[1] + jc[6 + a] * jp[4];
    const double w2 = jc[a] * jp[2] + jc[6 + a] * jp[5];
    Y[3 * a] = w0 * vi[0] + w1 * vi[1] + w2 * vi[2];
    Y[3 * a + 1] = w0 * vi[1] + w1 * vi[3] + w2 * vi[4];
    Y[3 * a + 2] = w0 * vi[2] + w1 * vi[4] + w2 * vi[5];
  }
}

// B = Ya^T Sigma_{fa fb} Yb (3x3, row-major).
__device__ __forceinline__ void cov_pair(const double* cov, long n, int fa, int fb, const double (&Ya)[18],
                                         const double (&Yb)[18], double (&B)[9]) {
#pragma unroll
  for (int e = 0; e < 9; ++e) B[e] = 0.0;
  const double* blk = cov + (6l * fa) * n + 6l * fb;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    double z0 = 0.0, z1 = 0.0, z2 = 0.0;
#pragma unroll
    for (int b = 0; b < 6; ++b) {
      const double s = blk[a * n + b];
      z0 += s * Yb[3 * b];
      z1 += s * Yb[3 * b + 1];
      z2 += s * Yb[3 * b + 2];
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      B[3 * d] += Ya[3 * a + d] * z0;
      B[3 * d + 1] += Ya[3 * a + d] * z1;
      B[3 * d + 2] += Ya[3 * a + d] * z2;
    }
  }
}

__global__ __launch_bounds__(kCovPointThreads) void ba_cov_points_kernel(CovPointArgs A) {
  const int p = blockIdx.x * kCovPointThreads + threadIdx.x;
  if (p >= A.n_points) return;
  const int o0 = A.point_ptr[p], o1 = A.point_ptr[p + 1];
  const double* Xp = A.points + 3l * A.pt_inv[p];
  const double X0 = Xp[0], X1 = Xp[1], X2 = Xp[2];
  double* out = A.out + 9l * p;
  // V in K1's order (point_block_w), its pivot test on the same values
  double v00 = 0, v01 = 0, v02 = 0, v11 = 0, v12 = 0, v22 = 0;
  for (int o = o0; o < o1; ++o) {
    double jp[6], jc[12];
    cov_obs_lin<false>(A, o, A.obs_cam[o], X0, X1, X2, jp, jc);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double a = jp[3 * k], b = jp[3 * k + 1], c = jp[3 * k + 2];
      v00 += a * a; v01 += a * b; v02 += a * c;
      v11 += b * b; v12 += b * c; v22 += c * c;
    }
  }
  v00 += A.lambda; v11 += A.lambda; v22 += A.lambda;
  const double eps = kCovPivotRelEps * (v00 + v11 + v22);
  bool ok = v00 > eps;
  const double i00 = rsq_nr(ok ? v00 : 1.0);
  const double t10 = v01 * i00, t20 = v02 * i00;
  const double d1 = v11 - t10 * t10;
  ok = ok && d1 > eps;
  const double i11 = rsq_nr(ok ? d1 : 1.0);
  const double t21 = (v12 - t20 * t10) * i11;
  const double d2 = v22 - t20 * t20 - t21 * t21;
  ok = ok && d2 > eps;
  if (!ok) {  // frozen: it left the system
    const double nan = __builtin_nan("");
#pragma unroll
    for (int e = 0; e < 9; ++e) out[e] = nan;
    return;
  }
  // V^-1 = L^-T L^-1 from the IEEE Cholesky
  double vi[6];
  {
    const double l00 = sqrt(v00), l10 = v01 / l00, l20 = v02 / l00;
    const double l11 = sqrt(v11 - l10 * l10), l21 = (v12 - l20 * l10) / l11;
    const double l22 = sqrt(v22 - l20 * l20 - l21 * l21);
    const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22;
    const double m10 = -(m11 * l10) * m00;
    const double m21 = -(m22 * l21) * m11;
    const double m20 = -(m21 * l10 + m22 * l20) * m00;
    vi[0] = m00 * m00 + m10 * m10 + m20 * m20;
    vi[1] = m10 * m11 + m20 * m21;
    vi[2] = m20 * m22;
    vi[3] = m11 * m11 + m21 * m21;
    vi[4] = m21 * m22;
    vi[5] = m22 * m22;
  }
  // acc (00 01 02 11 12 22) = V^-1 + sum_o [B_oo + sum_{o' < o} (B_oo' + B_oo'^T)], free observations
  double acc[6] = {vi[0], vi[1], vi[2], vi[3], vi[4], vi[5]};
  const long n = 6l * A.F;
  for (int o = o0; o < o1; ++o) {
    const int ca = A.obs_cam[o];
    if (ca < A.n_fixed) continue;
    double Ya[18], Yb[18], B[9];
    cov_obs_y(A, o, ca, X0, X1, X2, vi, Ya);
    cov_pair(A.cov, n, ca - A.n_fixed, ca - A.n_fixed, Ya, Ya, B);
    acc[0] += B[0]; acc[1] += B[1]; acc[2] += B[2]; acc[3] += B[4]; acc[4] += B[5]; acc[5] += B[8];
    for (int q = o0; q < o; ++q) {
      const int cb = A.obs_cam[q];
      if (cb < A.n_fixed) continue;
      cov_obs_y(A, q, cb, X0, X1, X2, vi, Yb);
      cov_pair(A.cov, n, ca - A.n_fixed, cb - A.n_fixed, Ya, Yb, B);
      acc[0] += 2.0 * B[0];
      acc[1] += B[1] + B[3];
      acc[2] += B[2] + B[6];
      acc[3] += 2.0 * B[4];
      acc[4] += B[5] + B[7];
      acc[5] += 2.0 * B[8];
    }
  }
  out[0] = acc[0]; out[1] = acc[1]; out[2] = acc[2];
  out[3] = acc[1]; out[4] = acc[3]; out[5] = acc[4];
  out[6] = acc[2]; out[7] = acc[4]; out[8] = acc[5];
}

}  // namespace

size_t cov_solve_lds_bytes(int F) { return (36ull * F + 36) * sizeof(double); }

// The two pose kernels' dynamic-LDS limit beyond the default 64 KiB (F > 226).  The attribute
// belongs to the current device, so it is set on every such call, not cached in the process.
static void cov_set_lds(size_t lds) {
  if (lds <= 64 * 1024) return;
  VO_HIP_CHECK(hipFuncSetAttribute((const void*)ba_cov_factor_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
  VO_HIP_CHECK(hipFuncSetAttribute((const void*)ba_cov_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
}

void launch_cov_factor(const CovPoseArgs& A, hipStream_t st) {
  if (A.F <= 0) return;
  const size_t lds = cov_solve_lds_bytes(A.F);  // (the panel: at most 6 (F - 1) rows of 6)
  cov_set_lds(lds);
  hipLaunchKernelGGL(ba_cov_factor_kernel, dim3(1), dim3(kCovFactorThreads), lds, st, A);
}

void launch_cov_solve(const CovPoseArgs& A, hipStream_t st) {
  if (A.F <= 0) return;
  const size_t lds = cov_solve_lds_bytes(A.F);
  cov_set_lds(lds);
  hipLaunchKernelGGL(ba_cov_solve_kernel, dim3(A.F), dim3(kCovSolveThreads), lds, st, A);
}

void launch_cov_points(const CovPointArgs& A, hipStream_t st) {
  if (A.n_points <= 0) return;
  hipLaunchKernelGGL(ba_cov_points_kernel, dim3((A.n_points + kCovPointThreads - 1) / kCovPointThreads),
                     dim3(kCovPointThreads), 0, st, A);
}

}  // namespace vo
