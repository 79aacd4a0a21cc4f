// Observation weights and device-side culling (include/vo_hip.h vo_ba_set_obs_weights,
// vo_ba_cull; DESIGN.md §Observation weights and culling), gfx950.
//
//   ba_lin_wave_w_kernel  the one-wave K1 (ba_lin_wave.h lin_wave_body) in its kWeighted modes:
//       sqrt(w) per observation from a device array in the plan's observation order.  A unit of
//       its own, so ba.hip's code object -- every K1 a session without weights launches -- is the
//       one it was.  Always the Huber code (ba_weights.h kWeightedNoHuber).
//   ba_cull_obs_kernel, ba_cull_track_kernel  the cull, two launches: the kernel boundary is what
//       orders the per-landmark walk behind the per-observation pass (nothing spins).
#include "ba_weights.h"

#include <utility>

#include "ba_lin_wave.h"

namespace vo {

namespace {

template <int MODE, int NW>
__global__ __launch_bounds__(kLinLanesWave * NW) void ba_lin_wave_w_kernel(LinArgs A, const double* __restrict__ sqw) {
  __shared__ LinWave Sw[NW];
  __shared__ int s_arrive;
  lin_wave_body<MODE, kBaStamps, NW, false>(A, Sw, &s_arrive, (int)blockIdx.x, LinGate{}, sqw);
}

template <int MODE, int... I>
bool lin_w_launch(const LinArgs& A, const double* sqw, int nw, dim3 g, hipStream_t st, std::integer_sequence<int, I...>) {
  constexpr int kMode = MODE | kRobust | kWeighted;
  return ((nw == I + 1 && (ba_lin_wave_w_kernel<kMode, I + 1><<<g, dim3(kLinLanesWave * nw), 0, st>>>(A, sqw), true)) ||
          ...);
}

constexpr int kCullThreads = 256;

// A count summed over the wave (every lane of it takes part: no lane returns early) and added to
// *dst by one integer atomic per wave: one atomic per lane on the same word serialises in L2
// (measured: 2.3 ms for cfg4's 200k landmarks).  Integer sums do not depend on the order.
__device__ __forceinline__ void wave_count(int v, int* dst) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  if ((threadIdx.x & 63) == 0 && v != 0) atomicAdd(dst, v);
}

// One lane per observation, problem order.  err2 and z: ba_obs_residual_kernel's operations in
// its order (ba.hip), so the rule below sees the bits vo_ba_residuals reports at this state.
__global__ __launch_bounds__(kCullThreads) void ba_cull_obs_kernel(CullArgs A) {
  const int o = blockIdx.x * kCullThreads + threadIdx.x;
  bool cull = false;
  if (o < A.n_obs) {
    const double w = A.w[o];
    const double* T = A.poses + 12l * A.obs_cam[o];
    const double* X = A.points + 3l * A.obs_pt[o];
    const double X0 = X[0], X1 = X[1], X2 = X[2];
    const double x = T[0] * X0 + T[1] * X1 + T[2] * X2 + T[9];
    const double y = T[3] * X0 + T[4] * X1 + T[5] * X2 + T[10];
    const double z = T[6] * X0 + T[7] * X1 + T[8] * X2 + T[11];
    const double iz = rcp_nr(z);
    const float2 m = A.obs_uv[o];
    const double r0 = A.fx * x * iz + A.cx - (double)m.x;
    const double r1 = A.fy * y * iz + A.cy - (double)m.y;
    const double err2 = r0 * r0 + r1 * r1;
    const bool finite = __builtin_isfinite(err2) && __builtin_isfinite(z);
    // (an inactive observation stays inactive and is not counted)
    cull = w > 0.0 && (!finite || (A.max_chi2 > 0.0 && w * err2 > A.max_chi2) || z <= A.min_depth);
    if (cull) {
      A.w[o] = 0.0;
      A.sqw_obs[o] = 0.0;
      A.sqw_plan[A.obs_pos[o]] = 0.0;
    }
  }
  wave_count(cull ? 1 : 0, &A.count[0]);
}

// One lane per landmark, problem order: its track is observations [point_ptr[p], point_ptr[p + 1]).
__global__ __launch_bounds__(kCullThreads) void ba_cull_track_kernel(CullArgs A) {
  const int p = blockIdx.x * kCullThreads + threadIdx.x;
  int culled = 0, kept = 0;
  if (p < A.n_points) {
    const int o0 = A.point_ptr[p], o1 = A.point_ptr[p + 1];
    int active = 0;
    for (int o = o0; o < o1; ++o) active += A.w[o] > 0.0 ? 1 : 0;
    if (A.min_track > 0 && active > 0 && active < A.min_track) {
      for (int o = o0; o < o1; ++o) {
        if (!(A.w[o] > 0.0)) continue;
        A.w[o] = 0.0;
        A.sqw_obs[o] = 0.0;
        A.sqw_plan[A.obs_pos[o]] = 0.0;
      }
      culled = active;
    } else {
      kept = active;
    }
  }
  wave_count(culled, &A.count[0]);
  wave_count(kept, &A.count[1]);
}

__global__ __launch_bounds__(kCullThreads) void ba_fill_kernel(double* __restrict__ p, int n, double v) {
  const int i = blockIdx.x * kCullThreads + threadIdx.x;
  if (i < n) p[i] = v;
}

}  // namespace

bool lin_weighted_covers(int wave_chunks) { return wave_chunks >= 1 && wave_chunks <= kWaveMaxChunks; }

bool launch_lin_weighted(const LinArgs& A, const double* sqw, int mode, int wave_chunks, int grid, hipStream_t st) {
  constexpr std::make_integer_sequence<int, kWaveMaxChunks> nws{};
  if (!lin_weighted_covers(wave_chunks) || !sqw) return false;
  const dim3 g(grid);
  switch (mode) {
    case 0: return lin_w_launch<0>(A, sqw, wave_chunks, g, st, nws);
    case kAccum: return lin_w_launch<kAccum>(A, sqw, wave_chunks, g, st, nws);
    case kBacksub: return lin_w_launch<kBacksub>(A, sqw, wave_chunks, g, st, nws);
    case kBacksub | kAccum: return lin_w_launch<kBacksub | kAccum>(A, sqw, wave_chunks, g, st, nws);
    case kLm | kAccum: return lin_w_launch<kLm | kAccum>(A, sqw, wave_chunks, g, st, nws);
    case kLm | kBacksub: return lin_w_launch<kLm | kBacksub>(A, sqw, wave_chunks, g, st, nws);
    default: return false;
  }
}

void launch_cull(const CullArgs& A, hipStream_t st) {
  if (A.n_obs <= 0) return;
  hipLaunchKernelGGL(ba_cull_obs_kernel, dim3((A.n_obs + kCullThreads - 1) / kCullThreads), dim3(kCullThreads), 0, st, A);
  if (A.n_points > 0)
    hipLaunchKernelGGL(ba_cull_track_kernel, dim3((A.n_points + kCullThreads - 1) / kCullThreads), dim3(kCullThreads), 0,
                       st, A);
}

void launch_fill(double* p, int n, double v, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(ba_fill_kernel, dim3((n + kCullThreads - 1) / kCullThreads), dim3(kCullThreads), 0, st, p, n, v);
}

}  // namespace vo
