// Sliding-window bundle adjustment: the Gauss-Newton iteration's kernels on gfx950.
//
// The reference has no BA; the problem is build-defined and
// restated on the CPU in oracle/ba_ref.py (projection model of reference
// src/modules/frontend.py:128-140, T_cw convention of src/modules/vo.py:260-261).
//
// This unit holds the BA's device code except the banded solver (ba_band.hip) and a host
// launch function per kernel (ba_kernels.h); the host engine that plans a window and enqueues
// the iterations is ba_engine.hip.  One GN iteration on the context stream:
//   K1  linearisation and Schur complement of the landmarks, per chunk of whole landmarks
//       (LDS-staged): [back-substitute the previous step's point update and apply it] ->
//       reprojection residuals + 2x6 / 2x3 Jacobians (one lane per observation) -> per track
//       entry W = Jc^T Jp and gc = Jc^T r, per landmark V = Jp^T Jp (+lambda), its 3x3
//       Cholesky L and h = L^-1 g -> Z = W L^-T, bt = -gc + Z h -> Schur blocks
//       U - Z_x Z_y^T, each (slot, row) owned by one lane and summed over a static pair list
//       in fixed order (deterministic, no atomics), written once to the segment's slab rows.
//       ba_lin_wave_kernel (every default window): one wave per chunk, a workgroup of NW
//       waves per segment of NW chunks (1 .. kWaveMaxChunks), whose blocks it combines.
//       ba_lin_kernel (only under the testing switch vo_ba_testing_k1(-1)): four waves per
//       segment, walking its chunks one after another into an LDS window.
//   K2  ba_reduce_kernel sums slab rows into the reduced camera system [S | b | cost] in fixed
//       segment order (ba_reduce.h).  A launch of its own -- or, on one rank when its
//       workgroups fit one round beside the solver, the same sums by reducer workgroups
//       inside the banded K3's launch (ba_band.hip).
//   K3  block bandwidth w <= 9 (band_supported): the banded solver (ba_band.hip).  Wider
//       (w > 9): the profile solver ba_solve_kernel here, one workgroup: right-looking 6x6-block
//       Cholesky of the profile (LDS resident when it fits) with the forward substitution
//       folded in, back substitution, and the left se(3) pose update T <- exp(dc^) T.
// The point update dp = L^-T(-h - sum Z^T dc) is applied by the next K1 (or a
// back-substitute-only K1), which recomputes the same linearisation bit for bit.
// A run of k >= 2 iterations of a window that qualifies (BAEngine::chain_ok: one rank, the fused
// full-layout launch, six-chunk segments that all fit beside the solver) is enqueued as one
// stand-alone K1, k - 1 chained launches -- solver, reducers and the NEXT iteration's K1 segments
// in one grid, the K1 workgroups doing their solve-independent loads and then waiting at a pose
// gate for the solver's publish word (ba_lin_wave.h LinGate, ba_band.hip kNext) -- and one plain
// fused launch; same kernels' arithmetic, one launch per iteration.
// Under a Huber cost (LinArgs::huber > 0, DESIGN.md §Robust cost) K1's kRobust instantiations
// scale each observation's residual and Jacobians by huber_scale (ba_math.h) where they are
// formed; the plain instantiations are untouched.  ba_obs_residual_kernel reads out the raw
// squared residual and the depth of every observation (vo_ba_residuals).
// ba_img_copy_kernel copies chunk images taken over from the previous window's plan.
#include "ba_kernels.h"

#include <atomic>
#include <utility>

#include "ba_lin_wave.h"
#include "ba_math.h"
#include "vo_common.h"

namespace vo {

namespace {

constexpr int kLinThreads = 256;
constexpr int kBsWindow = 10;  // K3 back substitution: register window of block rows

struct alignas(16) LinShared {
  ChunkImg img;  // static chunk lists (BAPlan::chunk_img), staged as one image
  int spos[kSegSlots];  // slab row of each window slot
  int cpos[kSegCams];   // rhs slab row of each window camera
  double win[kSegSlots * 36];
  double bwin[kSegCams * 6];
  double Jc[kChunkObs][12];
  double Jp[kChunkObs][6];
  double r[kChunkObs][2];
  alignas(16) double Z[kChunkTe][18];  // W, then Z = W L^-T (144-B rows, 16-B aligned)
  double bt[kChunkTe][6];  // gc, then bt = -gc + Z h
  double X[kChunkPts][3];
  double L[kChunkPts][6];  // 1/l00, l10, 1/l11, l20, l21, 1/l22
  double h[kChunkPts][3];
  double dcw[kSegCams][6];  // pending pose update of the segment's window cameras
  int te_use[kChunkTe];  // free camera and valid landmark
  int valid[kChunkPts];
  double pose_o[kSegAllCams][12];  // poses of every camera the segment sees: pending step's
  double pose_n[kSegAllCams][12];  // linearisation point (back substitution) and the new one
};
// three K1 workgroups per CU (the cfg3 plan then runs in a single round)
static_assert(sizeof(LinShared) <= 160 * 1024 / 3, "K1 LDS image");

// R1: residual and Jacobians, one lane per observation.  kRob (DESIGN.md §Robust cost): the
// Huber scale s of the raw residual multiplies r and both Jacobians (through the four projection
// derivatives every Jacobian entry is linear in), and the cost sums rho.
template <bool kRob>
__device__ __forceinline__ void lin_obs(LinShared& S, const LinArgs& A, const double (*pose)[12],
                                        int nob, double& cost) {
  for (int o = threadIdx.x; o < nob; o += kLinThreads) {
    const double* T = pose[S.img.acam[o]];
    const int q = S.img.te_pt[S.img.obs_te[o]];
    const double X0 = S.X[q][0], X1 = S.X[q][1], X2 = S.X[q][2];
    const double x = T[0] * X0 + T[1] * X1 + T[2] * X2 + T[9];
    const double y = T[3] * X0 + T[4] * X1 + T[5] * X2 + T[10];
    const double z = T[6] * X0 + T[7] * X1 + T[8] * X2 + T[11];
    const double iz = rcp_nr(z);
    const float2 m = reinterpret_cast<const float2*>(S.img.uv)[o];
    double r0 = A.fx * x * iz + A.cx - (double)m.x;
    double r1 = A.fy * y * iz + A.cy - (double)m.y;
    if constexpr (!kRob) cost += r0 * r0 + r1 * r1;
    double j00 = A.fx * iz, j02 = -A.fx * x * iz * iz;
    double j11 = A.fy * iz, j12 = -A.fy * y * iz * iz;
    if constexpr (kRob) {
      double rho;
      const double s = huber_scale(r0, r1, A.huber, A.huber2, rho);
      cost += rho;
      r0 *= s; r1 *= s;
      j00 *= s; j02 *= s; j11 *= s; j12 *= s;
    }
    S.r[o][0] = r0;
    S.r[o][1] = r1;
    double* jc = S.Jc[o];
    jc[0] = j00;
    jc[1] = 0.0;
    jc[2] = j02;
    jc[3] = j02 * y;
    jc[4] = j00 * z - j02 * x;
    jc[5] = -j00 * y;
    jc[6] = 0.0;
    jc[7] = j11;
    jc[8] = j12;
    jc[9] = j12 * y - j11 * z;
    jc[10] = -j12 * x;
    jc[11] = j11 * x;
    double* jp = S.Jp[o];
    jp[0] = j00 * T[0] + j02 * T[6];
    jp[1] = j00 * T[1] + j02 * T[7];
    jp[2] = j00 * T[2] + j02 * T[8];
    jp[3] = j11 * T[3] + j12 * T[6];
    jp[4] = j11 * T[4] + j12 * T[7];
    jp[5] = j11 * T[5] + j12 * T[8];
  }
}

// Landmark p of the chunk: V = sum Jp^T Jp (+lambda) and g = sum Jp^T r over its
// observations (S.r may hold r + Jc dc, see chunk_backsub), the pivot-tested 3x3
// Cholesky V = L L^T (same sequence as oracle/ba_ref.py point_block_valid) and
// h = L^-1 g.  l = (1/l00, l10, 1/l11, l20, l21, 1/l22).
__device__ __forceinline__ bool point_block(const LinShared& S, const LinArgs& A, int p,
                                            double (&l)[6], double (&h)[3]) {
  double v00 = 0, v01 = 0, v02 = 0, v11 = 0, v12 = 0, v22 = 0, g0 = 0, g1 = 0, g2 = 0;
  const int o0 = S.img.te_obs[S.img.pt_te[p]], o1 = S.img.te_obs[S.img.pt_te[p + 1]];
  for (int o = o0; o < o1; ++o) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double a = S.Jp[o][3 * k], b = S.Jp[o][3 * k + 1], c = S.Jp[o][3 * k + 2];
      const double rk = S.r[o][k];
      v00 += a * a; v01 += a * b; v02 += a * c;
      v11 += b * b; v12 += b * c; v22 += c * c;
      g0 += a * rk; g1 += b * rk; g2 += c * rk;
    }
  }
  v00 += A.lambda; v11 += A.lambda; v22 += A.lambda;
  // pivots by v_rsq_f64 + one Newton step (~1e-14 relative) instead of IEEE sqrt and five
  // divisions: the same pivot tests on the same values, no division on the chain
  const double eps = kPivotRelEps * (v00 + v11 + v22);
  bool ok = v00 > eps;
  const double i00 = rsq_nr(ok ? v00 : 1.0);
  const double l10 = v01 * i00, l20 = v02 * i00;
  const double d1 = v11 - l10 * l10;
  ok = ok && d1 > eps;
  const double i11 = rsq_nr(ok ? d1 : 1.0);
  const double l21 = (v12 - l20 * l10) * i11;
  const double d2 = v22 - l20 * l20 - l21 * l21;
  ok = ok && d2 > eps;
  const double i22 = rsq_nr(ok ? d2 : 1.0);
  l[0] = i00; l[1] = l10; l[2] = i11; l[3] = l20; l[4] = l21; l[5] = i22;
  h[0] = g0 * i00;
  h[1] = (g1 - l10 * h[0]) * i11;
  h[2] = (g2 - l20 * h[0] - l21 * h[1]) * i22;
  return ok;
}

// R2: per track entry W, gc; per landmark V (+lambda), pivot-tested Cholesky, h.
// The track-entry loop (threads [0, 128)) and the landmark loop (threads [128, 256)) are
// independent and run on different waves concurrently.
__device__ __forceinline__ void lin_reduce(LinShared& S, const LinArgs& A, int nte, int npt) {
  constexpr int kHalf = kLinThreads / 2;
  static_assert(kChunkTe <= kHalf && kChunkPts <= kHalf, "one track entry / landmark per thread");
  for (int t = threadIdx.x; t < nte && t < kHalf; t += kHalf) {
    double W[18], g[6];
#pragma unroll
    for (int e = 0; e < 18; ++e) W[e] = 0.0;
#pragma unroll
    for (int e = 0; e < 6; ++e) g[e] = 0.0;
    for (int o = S.img.te_obs[t]; o < S.img.te_obs[t + 1]; ++o) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const double rk = S.r[o][k];
        const double p0 = S.Jp[o][3 * k], p1 = S.Jp[o][3 * k + 1], p2 = S.Jp[o][3 * k + 2];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          const double jc = S.Jc[o][6 * k + a];
          W[3 * a] += jc * p0;
          W[3 * a + 1] += jc * p1;
          W[3 * a + 2] += jc * p2;
          g[a] += jc * rk;
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 18; ++e) S.Z[t][e] = W[e];
#pragma unroll
    for (int e = 0; e < 6; ++e) S.bt[t][e] = g[e];
  }
  for (int p = (int)threadIdx.x - kHalf; p >= 0 && p < npt; p += kHalf) {
    double l[6], h[3];
    const bool ok = point_block(S, A, p, l, h);
    S.valid[p] = ok;
#pragma unroll
    for (int e = 0; e < 6; ++e) S.L[p][e] = l[e];
    S.h[p][0] = ok ? h[0] : 0.0;
    S.h[p][1] = ok ? h[1] : 0.0;
    S.h[p][2] = ok ? h[2] : 0.0;
  }
}

// R3: Z = W L^-T and bt = -gc + Z h for track entries of valid landmarks in free
// cameras; zero otherwise (frozen landmarks leave the camera system).
__device__ __forceinline__ void lin_eliminate(LinShared& S, int nte) {
  for (int t = threadIdx.x; t < nte; t += kLinThreads) {
    const int p = S.img.te_pt[t];
    const bool use = S.valid[p] && S.img.te_lcam[t] >= 0;
    S.te_use[t] = use;
    if (!use) {
#pragma unroll
      for (int e = 0; e < 18; ++e) S.Z[t][e] = 0.0;
#pragma unroll
      for (int e = 0; e < 6; ++e) S.bt[t][e] = 0.0;
      // frozen landmark: its observations leave U too (gc was formed from Jc already)
      for (int o = S.img.te_obs[t]; o < S.img.te_obs[t + 1]; ++o)
#pragma unroll
        for (int e = 0; e < 12; ++e) S.Jc[o][e] = 0.0;
      continue;
    }
    const double i00 = S.L[p][0], l10 = S.L[p][1], i11 = S.L[p][2];
    const double l20 = S.L[p][3], l21 = S.L[p][4], i22 = S.L[p][5];
    const double h0 = S.h[p][0], h1 = S.h[p][1], h2 = S.h[p][2];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const double z0 = S.Z[t][3 * a] * i00;
      const double z1 = (S.Z[t][3 * a + 1] - l10 * z0) * i11;
      const double z2 = (S.Z[t][3 * a + 2] - l20 * z0 - l21 * z1) * i22;
      S.Z[t][3 * a] = z0;
      S.Z[t][3 * a + 1] = z1;
      S.Z[t][3 * a + 2] = z2;
      S.bt[t][a] = -S.bt[t][a] + (z0 * h0 + z1 * h1 + z2 * h2);
    }
  }
}

__device__ __forceinline__ void chunk_linearize(LinShared& S, const LinArgs& A,
                                                const double (*pose)[12], int nob,
                                                int nte, int npt, double& cost) {
  lin_obs<false>(S, A, pose, nob, cost);
  __syncthreads();
  lin_reduce(S, A, nte, npt);
  __syncthreads();
  lin_eliminate(S, nte);
  __syncthreads();
}

// Back-substitution of the pending step at its linearisation point (pose_o):
// dp = -V^-1 sum_o Jp_o^T (r_o + Jc_o dc_cam(o)) -- algebraically the Schur
// back-substitution -V^-1 (g + sum_t W_t^T dc) without forming W or Z.  V, the pivot
// test and the Cholesky are point_block's, so a landmark frozen in the pending step's
// camera system (invalid V) is not moved; fixed cameras contribute dc = 0.
// kRob: the scale s comes from the raw residual at that point, before Jc dc is added (lin_obs's
// huber_scale on the same values: the pending step's own weights), and multiplies r + Jc dc and Jp.
template <bool kRob>
__device__ __forceinline__ void chunk_backsub(LinShared& S, const LinArgs& A, int nob, int npt,
                                              int p0) {
  for (int o = threadIdx.x; o < nob; o += kLinThreads) {
    const double* T = S.pose_o[S.img.acam[o]];
    const int te = S.img.obs_te[o];
    const int q = S.img.te_pt[te];
    const double X0 = S.X[q][0], X1 = S.X[q][1], X2 = S.X[q][2];
    const double x = T[0] * X0 + T[1] * X1 + T[2] * X2 + T[9];
    const double y = T[3] * X0 + T[4] * X1 + T[5] * X2 + T[10];
    const double z = T[6] * X0 + T[7] * X1 + T[8] * X2 + T[11];
    const double iz = rcp_nr(z);
    const float2 m = reinterpret_cast<const float2*>(S.img.uv)[o];
    double r0 = A.fx * x * iz + A.cx - (double)m.x;
    double r1 = A.fy * y * iz + A.cy - (double)m.y;
    double j00 = A.fx * iz, j02 = -A.fx * x * iz * iz;
    double j11 = A.fy * iz, j12 = -A.fy * y * iz * iz;
    if constexpr (kRob) {
      double rho;
      const double s = huber_scale(r0, r1, A.huber, A.huber2, rho);
      r0 *= s; r1 *= s;
      j00 *= s; j02 *= s; j11 *= s; j12 *= s;
    }
    const int lc = S.img.te_lcam[te];
    if (lc >= 0) {  // + Jc dc (rows of lin_obs's Jc)
      const double* d = S.dcw[lc];
      r0 += j00 * d[0] + j02 * d[2] + (j02 * y) * d[3] + (j00 * z - j02 * x) * d[4] - (j00 * y) * d[5];
      r1 += j11 * d[1] + j12 * d[2] + (j12 * y - j11 * z) * d[3] - (j12 * x) * d[4] + (j11 * x) * d[5];
    }
    S.r[o][0] = r0;
    S.r[o][1] = r1;
    double* jp = S.Jp[o];
    jp[0] = j00 * T[0] + j02 * T[6];
    jp[1] = j00 * T[1] + j02 * T[7];
    jp[2] = j00 * T[2] + j02 * T[8];
    jp[3] = j11 * T[3] + j12 * T[6];
    jp[4] = j11 * T[4] + j12 * T[7];
    jp[5] = j11 * T[5] + j12 * T[8];
  }
  __syncthreads();
  for (int p = threadIdx.x; p < npt; p += kLinThreads) {
    double l[6], h[3];
    if (!point_block(S, A, p, l, h)) continue;
    const double x2 = -h[2] * l[5];
    const double x1 = (-h[1] - l[4] * x2) * l[2];
    const double x0 = (-h[0] - l[1] * x1 - l[3] * x2) * l[0];
    S.X[p][0] += x0;
    S.X[p][1] += x1;
    S.X[p][2] += x2;
    A.points[3l * (p0 + p)] = S.X[p][0];
    A.points[3l * (p0 + p) + 1] = S.X[p][1];
    A.points[3l * (p0 + p) + 2] = S.X[p][2];
  }
}

// Lanes per Schur item: the largest power of two <= 8 that keeps every item's parts in
// one pass of the workgroup (parts of an item are adjacent lanes of one wave).
__device__ __forceinline__ int parts_for(int items) {
  return items * 8 <= kLinThreads ? 8 : items * 4 <= kLinThreads ? 4 : items * 2 <= kLinThreads ? 2 : 1;
}

template <int Ctrl>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), Ctrl, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), Ctrl, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}

// Sum of the np (2, 4 or 8) adjacent lanes' values, valid in the first lane of each
// group: a fixed butterfly (xor 1, xor 2 within quads, then row_shl:4), so the order of
// the additions never depends on timing.  Every lane of the wave must execute it.
__device__ __forceinline__ double sum_parts(double v, int np) {
  v += dpp_f64<0xB1>(v);               // quad_perm [1,0,3,2]
  if (np >= 4) v += dpp_f64<0x4E>(v);  // quad_perm [2,3,0,1]
  if (np >= 8) v += dpp_f64<0x104>(v); // row_shl:4 (lane 8g + 0 reads 8g + 4)
  return v;
}

// The same butterfly with a per-lane group width 2^lg (0..3): groups are aligned to their
// width, so each step only ever combines lanes of one group; lanes of narrower groups keep
// their value (select).  Every lane of the wave must execute it.
__device__ __forceinline__ double sum_parts_lane(double v, int lg) {
  const double a = dpp_f64<0xB1>(v);
  v = lg >= 1 ? v + a : v;
  const double b = dpp_f64<0x4E>(v);
  v = lg >= 2 ? v + b : v;
  const double c = dpp_f64<0x104>(v);
  return lg >= 3 ? v + c : v;
}

// Diagnostic build (VO_BA_STAMPS=1): thread 0 accumulates s_memtime deltas per
// phase; the production instantiation has kStamp = false and executes none.
// dst[i] = src[i] + add, i < n, by the workgroup: U loads per thread issued before
// any store; loads are unconditional (clamped index) so none is sunk into a branch.
template <typename T, int U, typename Src, typename V>
__device__ __forceinline__ void stage(T* dst, const Src* __restrict__ src, int n, V add) {
  if (n <= 0) return;
  for (int e = threadIdx.x; e < n; e += U * kLinThreads) {
    Src a[U];
#pragma unroll
    for (int u = 0; u < U; ++u) a[u] = src[min(e + u * kLinThreads, n - 1)];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (e + u * kLinThreads < n) dst[e + u * kLinThreads] = (T)(a[u] + add);
  }
}


template <int MODE, bool kStamp>
__global__ __launch_bounds__(kLinThreads, 3) void ba_lin_kernel(LinArgs A) {  // 3 per CU: <= 168 VGPRs
  __shared__ LinShared S;
  Stamper<kStamp> st;
  st.start();
  constexpr bool kRob = (MODE & kRobust) != 0;
  // step control: the damping of this linearisation (or of the step being back-substituted) is
  // on the device; every later read of A.lambda sees it
  if constexpr ((MODE & kLm) != 0) A.lambda = *A.lm_lambda;
  const int seg = blockIdx.x, tid = threadIdx.x;
  // one load level: the status word, the segment header (uniform) and this thread's
  // camera ids (fixed offsets in the header); then poses and the pending update
  const int* SH = A.seg_hdr + (long)kSegHdr * seg;
  const int4* SH4 = reinterpret_cast<const int4*>(SH);
  const int16_t* SH16 = reinterpret_cast<const int16_t*>(SH);
  const int stat = A.status ? *A.status : 0;
  const int4 g0 = SH4[0], g1 = SH4[1];
  int4 h0 = SH4[8], h1 = SH4[9], h2 = SH4[10], h3 = SH4[11];  // first chunk's header
  const int i_acam = SH16[16 + min(tid / 12, kSegAllCams - 1)];
  const int i_wcam = SH16[32 + min(tid / 6, kSegCams - 1)];
  if (stat) return;  // a previous solve failed: state frozen
  const int nslots = g0.x, slot_off = g0.y, cam0 = g0.z, ncams = g0.w, na = g1.x;
  const int ch0 = g1.y, ch1 = g1.z;
  static_assert(12 * kSegAllCams <= kLinThreads && 6 * kSegCams <= kLinThreads,
                "one pose / update element per thread");
  if (MODE & kBacksub)
    if (tid < ncams * 6) S.dcw[tid / 6][tid % 6] = A.dc[6l * i_wcam + tid % 6];
  if (tid < 12 * na) {  // poses of the segment's cameras, once per segment
    const long g = 12l * i_acam + tid % 12;
    S.pose_n[tid / 12][tid % 12] = A.pose_new[g];
    if (MODE & kBacksub) S.pose_o[tid / 12][tid % 12] = A.pose_old[g];
  }
  if (MODE & kAccum) {
    for (int e = tid; e < nslots * 36; e += kLinThreads) S.win[e] = 0.0;
    for (int e = tid; e < ncams * 6; e += kLinThreads) S.bwin[e] = 0.0;
    if (tid < nslots) S.spos[tid] = A.slab_pos[slot_off + tid];
    if (tid < ncams) S.cpos[tid] = A.cam_pos[cam0 + tid];
  }
  double cost = 0.0;
  st.count(kPhSlots, nslots);
  st.count(kPhCams, ncams);
  // staging of a chunk: one 16-byte load of its image and of its landmark positions
  // (state) per thread, issued one chunk ahead (the next chunk's landmarks are disjoint from
  // the ones this chunk's back substitution writes); headers are read two chunks ahead
  constexpr int kImgVec = (int)(sizeof(ChunkImg) / 16);
  static_assert(kImgVec <= kLinThreads && 3 * kChunkPts <= kLinThreads, "one staging element per thread");
  const int i0 = tid;
  auto stage_img = [&](int c) { return reinterpret_cast<const uint4*>(A.chunk_img + c)[min(tid, kImgVec - 1)]; };
  auto stage_x = [&](const int4& hp) { return A.points[3l * hp.x + min(i0, max(3 * hp.y - 1, 0))]; };
  uint4 v_img = stage_img(ch0);
  double v_x = stage_x(h1);
  int4 n0, n1, n2, n3;  // the next chunk's header
  {
    const int chn = min(ch0 + 1, ch1 - 1);
    n0 = A.chunk_hdr[4l * chn];
    n1 = A.chunk_hdr[4l * chn + 1];
    n2 = A.chunk_hdr[4l * chn + 2];
    n3 = A.chunk_hdr[4l * chn + 3];
  }
  for (int ch = ch0; ch < ch1; ++ch) {
    const int chn = min(ch + 1, ch1 - 1), chn2 = min(ch + 2, ch1 - 1);
    const int4 m0 = A.chunk_hdr[4l * chn2], m1 = A.chunk_hdr[4l * chn2 + 1], m2 = A.chunk_hdr[4l * chn2 + 2],
               m3 = A.chunk_hdr[4l * chn2 + 3];
    const uint4 w_img = stage_img(chn);
    const double w_x = stage_x(n1);
    const int nob = h0.y, nte = h0.w, p0 = h1.x, npt = h1.y, e0 = h2.x, e1 = h2.y;
    st.count(kPhObs, nob);
    st.count(kPhTe, nte);
    st.count(kPhPts, npt);
    st.count(kPhPairs, e1 - e0);
    auto rotate = [&]() {
      h0 = n0;
      h1 = n1;
      h2 = n2;
      h3 = n3;
      n0 = m0;
      n1 = m1;
      n2 = m2;
      n3 = m3;
      v_img = w_img;
      v_x = w_x;
    };
    __syncthreads();  // previous chunk fully consumed
    if (tid < kImgVec) reinterpret_cast<uint4*>(&S.img)[tid] = v_img;
    if (i0 < 3 * npt) (&S.X[0][0])[i0] = v_x;
    __syncthreads();
    st.mark(kPhLoad);

    if (MODE & kBacksub) {
      chunk_backsub<kRob>(S, A, nob, npt, p0);
      __syncthreads();
      st.mark(kPhBacksub);
    }

    if (!(MODE & kAccum)) {
      lin_obs<kRob>(S, A, S.pose_n, nob, cost);  // cost at the updated state
      rotate();
      continue;
    }
    lin_obs<kRob>(S, A, S.pose_n, nob, cost);
    __syncthreads();
    st.mark(kPhLinObs);
    lin_reduce(S, A, nte, npt);
    __syncthreads();
    st.mark(kPhReduce);
    lin_eliminate(S, nte);
    __syncthreads();
    st.mark(kPhElim);

    // R4: Schur blocks into the window.  Item (slot, row a) sums its slot's pair list of
    // this chunk; with few slots (narrow segments: two cameras, many two-view landmarks)
    // an item's list is split over np lanes (pairs e0 + part + j np) whose partial rows
    // are combined by a fixed DPP butterfly -- deterministic, no LDS scratch.  Unrolled by
    // two with two register sets: pair j+2's Z rows are fetched (16-byte LDS reads,
    // indices read two pairs ahead, clamped -- no branches) while pair j+1's 18 FMAs run.
    {
      // the chunk's active slots on balanced lanes (ChunkImg::abase / anp): lane tid -> entry
      // si (binary search over the lane bases), row a, part of 2^lgp
      // (a chunk with more than 42 active slots takes a second pass of one lane per row item)
      static_assert(kLinLanes == kLinThreads, "planner lane budget = K1 workgroup");
      const int nas = h3.z, lanes = S.img.abase[nas];
      for (int base = 0; base < lanes; base += kLinThreads) {
      const int t = base + tid;
      int si = 0;
#pragma unroll
      for (int st = 32; st > 0; st >>= 1)
        if (si + st < nas && S.img.abase[si + st] <= t) si += st;
      const bool live = t < lanes;
      const int lgp = live ? S.img.anp[si] : 0, np = 1 << lgp;
      const int off = t - S.img.abase[si], a = off >> lgp, part = off & (np - 1);
      const int s = live ? S.img.aslot[si] : 0;
        double out[6] = {0, 0, 0, 0, 0, 0};
        const int e0 = live ? S.img.slotp[si] + part : 0, e1 = live ? S.img.slotp[si] + S.img.apcnt[si] : 0;
        if (e0 < e1) {
          auto zrow = [&](int pr, double (&za)[3], double2 (&zy)[9]) {
            const double2* py = reinterpret_cast<const double2*>(S.Z[pr >> 8]);
#pragma unroll
            for (int k = 0; k < 9; ++k) zy[k] = py[k];
            const double* px = &S.Z[pr & 255][3 * a];
            za[0] = px[0];
            za[1] = px[1];
            za[2] = px[2];
          };
          auto accum = [&](const double (&za)[3], const double2 (&zy)[9]) {
            const double* zf = reinterpret_cast<const double*>(zy);
#pragma unroll
            for (int c = 0; c < 6; ++c)
              out[c] -= za[0] * zf[3 * c] + za[1] * zf[3 * c + 1] + za[2] * zf[3 * c + 2];
          };
          const int n = (e1 - e0 + np - 1) / np;  // this part's pairs
          auto pid = [&](int j) { return (int)S.img.pairs[e0 + min(j, n - 1) * np]; };
          double zaA[3], zaB[3];
          double2 zyA[9], zyB[9];
          zrow(pid(0), zaA, zyA);
          zrow(pid(1), zaB, zyB);
          int pc = pid(2), pd = pid(3);
          int j = 0;
          for (; j + 2 <= n; j += 2) {
            const int pe = pid(j + 4), pf = pid(j + 5);
            accum(zaA, zyA);
            zrow(pc, zaA, zyA);
            accum(zaB, zyB);
            zrow(pd, zaB, zyB);
            pc = pe;
            pd = pf;
          }
          if (j < n) accum(zaA, zyA);
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) out[c] = sum_parts_lane(out[c], lgp);
        if (live && part == 0)
#pragma unroll
          for (int c = 0; c < 6; ++c) S.win[36 * s + 6 * a + c] += out[c];
      }
    }
    st.mark(kPhSchur);
    __syncthreads();  // the diagonal slots receive U below
    // per window camera c, row a: U_c row a = sum over its observations of Jc^T Jc
    // (static observation list, indices read ahead) and b_c[a] = sum of bt over its
    // track entries; split over np lanes like the pairs when the window is narrow
    {
      const int items = h3.w * 6;  // the chunk's active cameras (ChunkImg::acid)
      const int np = parts_for(items);
      for (int base = 0; base < items * np; base += kLinThreads) {
        const int idx = base + tid, item = idx / np, part = idx % np;
        const int ci = item / 6, a = item - 6 * (item / 6);
        const int c = item < items ? S.img.acid[ci] : 0;
        double out[6] = {0, 0, 0, 0, 0, 0};
        double acc = 0.0;
        if (item < items) {
          const int q0 = S.img.camop[ci] + part, q1 = S.img.camop[ci + 1];
          if (q1 > q0) {
            const int ql = q1 - 1;
            int on = S.img.camol[q0];
            for (int q = q0; q < q1; q += np) {
              const int o = on;
              on = S.img.camol[min(q + np, ql)];
              const double2* jr = reinterpret_cast<const double2*>(S.Jc[o]);
              double j[12];
#pragma unroll
              for (int k = 0; k < 6; ++k) {
                const double2 v = jr[k];
                j[2 * k] = v.x;
                j[2 * k + 1] = v.y;
              }
              const double ja0 = S.Jc[o][a], ja1 = S.Jc[o][6 + a];
#pragma unroll
              for (int cc = 0; cc < 6; ++cc) out[cc] += ja0 * j[cc] + ja1 * j[6 + cc];
            }
          }
          const int e0 = S.img.camp[ci] + part, e1 = S.img.camp[ci + 1];
          if (e1 > e0) {
            const int el = e1 - 1;
            int xn = S.img.caml[e0];
            for (int e = e0; e < e1; e += np) {
              const int x = xn;
              xn = S.img.caml[min(e + np, el)];
              acc += S.bt[x][a];
            }
          }
        }
        if (np > 1) {
#pragma unroll
          for (int cc = 0; cc < 6; ++cc) out[cc] = sum_parts(out[cc], np);
          acc = sum_parts(acc, np);
        }
        if (item < items && part == 0) {
          S.bwin[6 * c + a] += acc;
          double* w = &S.win[36 * S.img.dslot[ci] + 6 * a];
#pragma unroll
          for (int cc = 0; cc < 6; ++cc) w[cc] += out[cc];
        }
      }
    }
    st.mark(kPhSchurU);
    rotate();
  }
  __syncthreads();
  if (MODE & kAccum) {  // window slots to their profile-major slab rows (K2 reads them in order)
    for (int e = tid; e < nslots * 36; e += kLinThreads) A.slab[36l * S.spos[e / 36] + e % 36] = S.win[e];
    for (int e = tid; e < ncams * 6; e += kLinThreads) A.slab_b[6l * S.cpos[e / 6] + e % 6] = S.bwin[e];
  }
  // segment cost: a fixed xor butterfly inside each wave, then the four wave sums in order
  // (deterministic; one barrier instead of a nine-barrier LDS tree)
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) cost += __shfl_xor(cost, m, 64);
  double* red = &S.Z[0][0];  // Z is dead after the last chunk: reuse it for the cost
  if ((tid & 63) == 0) red[tid >> 6] = cost;
  __syncthreads();
  if (tid == 0) {
    double c = 0.0;
    for (int w = 0; w < kLinThreads / 64; ++w) c += red[w];
    A.slab_cost[seg] = c;
  }
  st.mark(kPhWrite);
  st.flush(A.stamps);
}

// ---- K1, one wave per chunk (plans of one chunk per segment) --------------------------
// A segment is one chunk and one 64-lane workgroup: every phase of the chunk runs on one
// wave (a workgroup barrier is then only the LDS wait), and six such workgroups share a CU,
// so all of cfg3's chunks run at once instead of three four-wave workgroups per CU walking
// two chunks each behind nine barriers a chunk.  The LDS image is ~25.5 KB: the track
// entries' Z | bt region doubles as the observations' Jp | r during the linearisation and as
// the back substitution's pose_o | dc; the camera blocks U and the rhs are summed by the
// diagonal slots' lanes over their pairs' observations (a diagonal slot's pairs are exactly
// its camera's track entries), so every window item is finished in registers and written to
// its slab row once.
// The body, its LDS image and its helpers are in ba_lin_wave.h (lin_wave_body); the fused
// launch's chained instantiation (ba_band.hip) runs the same body behind its pose gate.
template <int MODE, bool kStamp, int NW>
__global__ __launch_bounds__(kLinLanesWave * NW) void ba_lin_wave_kernel(LinArgs A) {
  __shared__ LinWave Sw[NW];
  __shared__ int s_arrive;
  lin_wave_body<MODE, kStamp, NW, false>(A, Sw, &s_arrive, (int)blockIdx.x, LinGate{});
}

// K2: fixed-order reduction of the slabs into [S profile | b | cost] (ReduceArgs, sum_rows:
// ba_reduce.h).

// One workgroup per profile block: 14 strided partial sums per S entry (16-byte loads) and, on
// a diagonal block, 42 per rhs entry of that camera, combined in fixed order (the result is
// bitwise reproducible).  The last workgroup sums the cost.  Every load of a
// workgroup is issued before the status test (a failed earlier step: nothing is written).
__global__ __launch_bounds__(kRedThreads) void ba_reduce_kernel(ReduceArgs A) {
  __shared__ __attribute__((aligned(16))) double part[kRedSParts * 36];
  __shared__ double partb[kRedBParts * 6];
  const int blk = blockIdx.x, tid = threadIdx.x;
  if (blk < A.nprof) {
    const int4 m = A.meta[blk];
    const int2 o = A.out[blk];
    const int failed = A.status ? *A.status : 0;
    const bool diag = m.z >= 0;
    double2 ps = make_double2(0.0, 0.0);
    double pb = 0.0;
    if (tid < kRedSParts * 18) ps = sum_rows2(A.slab, m.x, m.y, tid / 18, kRedSParts, tid % 18);
    if (diag && tid < kRedBParts * 6) pb = sum_rows<6>(A.slab_b, m.z, m.w, tid / 6, kRedBParts, tid % 6);
    if (failed) return;  // uniform
    if (tid < kRedSParts * 18) reinterpret_cast<double2*>(part)[tid] = ps;
    if (tid < kRedBParts * 6) partb[tid] = pb;
    __syncthreads();
    if (tid < 36) {
      double acc = 0.0;
#pragma unroll
      for (int q = 0; q < kRedSParts; ++q) acc += part[36 * q + tid];
      if (diag && tid % 7 == 0) acc += A.lambda;
      A.sys[(o.x & ~kRedTranspose) + ((o.x & kRedTranspose) ? 6 * (tid % 6) + tid / 6 : tid)] = acc;
    } else if (diag && tid >= 64 && tid < 70) {  // another wave: the rhs sum beside the S sum
      const int e = tid - 64;
      double acc = 0.0;
      for (int q = 0; q < kRedBParts; ++q) acc += partb[6 * q + e];
      A.sys[o.y + e] = acc;
    }
    return;
  }
  // cost: fixed-order lane-strided partial sums, then a fixed tree over the 256 lanes
  double c = 0.0;
  if (A.nseg > 0) {  // lane-strided, in order, every load of a batch in flight (sum_rows)
    for (int s = tid; s < A.nseg; s += 4 * kRedThreads) {
      double v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = A.slab_cost[min(s + i * kRedThreads, A.nseg - 1)];
#pragma unroll
      for (int i = 0; i < 4; ++i) c += s + i * kRedThreads < A.nseg ? v[i] : 0.0;
    }
  }
  if (A.status && *A.status) return;
  __shared__ double cpart[kRedThreads];
  cpart[tid] = c;
  __syncthreads();
  for (int m = kRedThreads / 2; m > 0; m >>= 1) {
    if (tid < m) cpart[tid] += cpart[tid + m];
    __syncthreads();
  }
  if (tid == 0) A.sys[A.cost_off] = cpart[0];
}


// K3.  Right-looking 6x6-block Cholesky of the profile of S with the forward
// substitution folded in, then back substitution and the pose update; one
// workgroup of four waves, one barrier per block column k:
//   every wave   reads D_k, factors it in registers (L_kk, 1/diag) and computes the
//                WHOLE panel L_ik = S_ik L_kk^-T (one lane per row) into its own
//                private LDS copy -- so the trailing update below needs no barrier;
//   trailing     S_ij -= L_ik L_jk^T over the panel's lower block triangle (this
//                includes D_{k+1}), one lane per (block, row), rows interleaved over
//                the waves, each reading only its own wave's panel copy;
//   wave 1       y_i -= L_ik y'_k with y'_k = L_kk^-1 y_k;
//   wave 2       keeps L_kk, 1/diag and y'_k for the back substitution;
//   wave 3       (next column) writes the panel into the profile blocks (i, k).
// The per-column panel rows and trailing blocks come from the host-built step
// table (BAPlan::solve_tab), staged in LDS with the profile.
enum { kS3Setup = 0, kS3Factor, kS3Backsub, kS3Tail, kS3Data, kS3Chol, kS3Panel, kS3Trail, kS3Barrier, kS3Mid, kS3End };
static_assert(kS3End == kS3Count, "profile K3 stamp row (ba_kernels.h)");

// dst[i] = src[i], i < n: U loads in flight per thread.  Loads and stores are
// unconditional with a clamped index (an out-of-range slot rewrites dst[n-1] with
// src[n-1]): a predicated load is sunk into its store's branch and serialises.
template <typename T, int U>
__device__ __forceinline__ void copy_in(T* dst, const T* __restrict__ src, int n, int tid, int nthr) {
  if (n <= 0) return;
  for (int e = tid; e < n; e += U * nthr) {
    T a[U];
#pragma unroll
    for (int u = 0; u < U; ++u) a[u] = src[min(e + u * nthr, n - 1)];
#pragma unroll
    for (int u = 0; u < U; ++u) dst[min(e + u * nthr, n - 1)] = a[u];
  }
}

template <bool kLds, bool kStamp, int NW>
__global__ __launch_bounds__(64 * NW) void ba_solve_kernel(SolveArgs A) {
  constexpr int kThr = 64 * NW;
  constexpr int wY = NW > 1 ? 1 : 0, wK = NW > 2 ? 2 : NW - 1, wC = NW - 1;  // role waves
  unsigned long long st_t = 0, st_acc[kS3Count] = {};
  auto mark = [&](int ph) {
    if (kStamp && threadIdx.x == 0) {
      const unsigned long long n = __builtin_amdgcn_s_memtime();
      if (st_t) st_acc[ph] += n - st_t;
      st_t = n;
    }
  };
  mark(0);
  // stamped build only: wait for outstanding LDS / a VALU result before a stamp
  auto settle = [&](double v) {
    if (kStamp) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      (void)__builtin_amdgcn_readfirstlane(__double2hiint(v));
    }
  };
  extern __shared__ __attribute__((aligned(16))) double dyn[];
  __shared__ int s_fail;
  const int tid = threadIdx.x, F = A.F;
  const int wave = tid >> 6, lane = tid & 63;
  const bool prior_fail = A.status && *A.status;
  double* Sm = kLds ? dyn : A.sys;
  double* kf = dyn + A.lds_kf;       // 36 per column
  double* y = dyn + A.lds_y;         // 6F
  double* Pw = dyn + A.lds_panel + 36l * A.max_panel * wave;  // this wave's panel copy
  int* tab = reinterpret_cast<int*>(dyn + A.lds_tab);
  const int* t_diag = tab + A.tl.diag;
  const int* t_off = tab + A.tl.off;
  const int* t_first = tab + A.tl.first;
  const int* t_sptr = tab + A.tl.step_ptr;
  const int* t_pi = tab + A.tl.panel_i;
  const int* t_pblk = tab + A.tl.panel_blk;
  const int* t_iptr = tab + A.tl.item_ptr;
  const int* t_iblk = tab + A.tl.item_blk;
  const int* t_iq = tab + A.tl.item_q;
  if (tid == 0) {
    s_fail = prior_fail ? 1 : 0;
    if (A.cost_out) *A.cost_out = A.sys[36l * A.nprof + 6l * F];
  }
  if (!prior_fail) {
    // global -> LDS, every load of a batch in flight before the stores
    if (kLds) copy_in<double2, 16>(reinterpret_cast<double2*>(Sm), reinterpret_cast<const double2*>(A.sys),
                                   18 * A.nprof, tid, kThr);
    copy_in<double, 4>(y, A.sys + 36l * A.nprof, 6 * F, tid, kThr);
    copy_in<int, 8>(tab, A.tab, A.tl.len, tid, kThr);
  }
  double* pose_l = dyn + A.lds_pose;  // current poses, staged early for the tail
  copy_in<double, 4>(pose_l, A.pose_cur, 12 * A.n_poses, tid, kThr);
  __syncthreads();
  mark(kS3Setup);

  auto ld6 = [](const double* p, double (&v)[6]) {
    const double2* q = reinterpret_cast<const double2*>(p);
    const double2 a0 = q[0], a1 = q[1], a2 = q[2];
    v[0] = a0.x; v[1] = a0.y; v[2] = a1.x; v[3] = a1.y; v[4] = a2.x; v[5] = a2.y;
  };
  auto st6 = [](double* p, const double (&v)[6]) {
    double2* q = reinterpret_cast<double2*>(p);
    q[0] = make_double2(v[0], v[1]);
    q[1] = make_double2(v[2], v[3]);
    q[2] = make_double2(v[4], v[5]);
  };
  auto dot6 = [](const double (&u)[6], const double* w) {
    const double2* q = reinterpret_cast<const double2*>(w);
    const double2 a0 = q[0], a1 = q[1], a2 = q[2];
    return u[0] * a0.x + u[1] * a0.y + u[2] * a1.x + u[3] * a1.y + u[4] * a2.x + u[5] * a2.y;
  };

  // Per-column descriptors from the static step table, loaded one column ahead so
  // that after each barrier only the data loads (one LDS round trip) precede chol6.
  struct Desc {
    int p0, nb, i0, nt, diag, pblk, pi, blk0, q0;
  };
  const int tfi = lane * NW + wave;  // this lane's first trailing (block, row) item
  auto desc1 = [&](int k, Desc& d) {
    d.p0 = t_sptr[k];
    d.nb = t_sptr[k + 1] - d.p0;
    d.i0 = t_iptr[k];
    d.nt = 6 * (t_iptr[k + 1] - d.i0);
    d.diag = t_diag[k];
  };
  auto desc2 = [&](Desc& d) {
    d.pblk = d.pi = d.blk0 = d.q0 = 0;
    if (lane < 6 * d.nb) {
      d.pblk = t_pblk[d.p0 + lane / 6];
      d.pi = t_pi[d.p0 + lane / 6];
    }
    if (tfi < d.nt) {
      d.blk0 = t_iblk[d.i0 + tfi / 6];
      d.q0 = t_iq[d.i0 + tfi / 6];
    }
  };
  Desc cur{}, nxt{};
  if (F > 0 && !prior_fail) {
    desc1(0, cur);
    desc2(cur);
  }
  bool bad = false;
  bool prev_row = false;
  int prev_blk = 0, prev_p0 = 0, prev_nb = 0;
  double sv[6] = {0, 0, 0, 0, 0, 0};
  for (int k = 0; k < F && !prior_fail; ++k) {
    // wave 3: its previous panel row (still in registers) -> profile block (i, k-1), for
    // the back substitution; nobody touches blocks (i, k-1) from column k on
    if (wave == wC) {
      if (prev_row) st6(Sm + 36l * prev_blk + 6 * (lane % 6), sv);
      for (int r = lane + 64; r < 6 * prev_nb; r += 64) {
        double v[6];
        ld6(Pw + 6 * r, v);
        st6(Sm + 36l * t_pblk[prev_p0 + r / 6] + 6 * (r % 6), v);
      }
    }
    // data loads of column k
    double L[21], r[6], yk[6], s0[6];
    {
      const double* D = Sm + 36l * cur.diag;
      double dr[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        ld6(D + 6 * i, dr);
#pragma unroll
        for (int c = 0; c <= i; ++c) L[P6(i, c)] = dr[c];
      }
    }
    ld6(y + 6 * k, yk);
    const bool prow = lane < 6 * cur.nb;
    if (prow) ld6(Sm + 36l * cur.pblk + 6 * (lane % 6), sv);
    if (tfi < cur.nt) ld6(Sm + 36l * cur.blk0 + 6 * (tfi % 6), s0);
    if (k + 1 < F) desc1(k + 1, nxt);
    settle(L[0] + sv[0] + s0[0] + yk[0]);
    mark(kS3Data);
    const bool ok = chol6(L, r);
    settle(r[5]);
    mark(kS3Chol);
    if (wave == wY || wave == wK) fwd6(L, r, yk);  // y'_k: wave 1 updates y, wave 2 keeps it
    if (wave == wK && lane == 0)
      bad = bad || !ok || !isfinite(yk[0] + yk[1] + yk[2] + yk[3] + yk[4] + yk[5]);
    // panel (every wave, its own copy); wave 1 also updates y
    if (prow) {
      fwd6(L, r, sv);
      st6(Pw + 6 * lane, sv);
      if (wave == wY) y[6 * cur.pi + lane % 6] -= sv[0] * yk[0] + sv[1] * yk[1] + sv[2] * yk[2] +
                                                 sv[3] * yk[3] + sv[4] * yk[4] + sv[5] * yk[5];
    }
    for (int rr = lane + 64; rr < 6 * cur.nb; rr += 64) {  // panels wider than 10 blocks
      double v[6];
      ld6(Sm + 36l * t_pblk[cur.p0 + rr / 6] + 6 * (rr % 6), v);
      fwd6(L, r, v);
      st6(Pw + 6 * rr, v);
      if (wave == wY) y[6 * t_pi[cur.p0 + rr / 6] + rr % 6] -= v[0] * yk[0] + v[1] * yk[1] + v[2] * yk[2] +
                                                               v[3] * yk[3] + v[4] * yk[4] + v[5] * yk[5];
    }
    if (wave == wK && lane == 0) {
      double* o = kf + 36l * k;
#pragma unroll
      for (int e = 0; e < 20; e += 2) reinterpret_cast<double2*>(o)[e / 2] = make_double2(L[e], L[e + 1]);
      reinterpret_cast<double2*>(o)[10] = make_double2(L[20], 0.0);
      st6(o + 24, r);
      st6(o + 30, yk);
    }
    wave_sync<true>();
    settle(sv[5]);
    mark(kS3Panel);
    // trailing update from this wave's panel copy
    for (int t = tfi; t < cur.nt; t += kThr) {
      double s[6];
      int blk, q;
      if (t == tfi) {
#pragma unroll
        for (int c = 0; c < 6; ++c) s[c] = s0[c];
        blk = cur.blk0;
        q = cur.q0;
      } else {
        blk = t_iblk[cur.i0 + t / 6];
        q = t_iq[cur.i0 + t / 6];
        ld6(Sm + 36l * blk + 6 * (t % 6), s);
      }
      const int rr = t % 6;
      double a[6];
      ld6(Pw + 36 * (q & 0xffff) + 6 * rr, a);
      const double* B = Pw + 36 * (q >> 16);
#pragma unroll
      for (int c = 0; c < 6; ++c) s[c] -= dot6(a, B + 6 * c);
      st6(Sm + 36l * blk + 6 * rr, s);
    }
    settle(0.0);
    mark(kS3Trail);
    if (k + 1 < F) desc2(nxt);  // static table: its latency hides in the barrier wait
    prev_row = prow;
    prev_blk = cur.pblk;
    prev_p0 = cur.p0;
    prev_nb = cur.nb;
    cur = nxt;
    __syncthreads();
    mark(kS3Barrier);
  }
  if (wave == wK && lane == 0 && bad) s_fail = 1;
  __syncthreads();
  mark(kS3Factor);
  // Back substitution L^T x = y' on wave 0.
  if (!s_fail && wave == 0) {
    if (A.max_row_span < kBsWindow) {
      // Register-resident form (every row of L spans < kBsWindow blocks).  Lane
      // (g, c), g < kBsWindow, c < 6, accumulates component c of y'_j for the one block
      // row j = g (mod kBsWindow) inside the window [k - kBsWindow, k - 1] of step k.
      // Step k: y_k (group k mod W) -> 12 readlanes -> x_k = L_kk^-T y_k in every lane
      // -> each lane subtracts (L_kj^T x_k)_c for its j in row k.  L_kk, 1/diag, the
      // L_kj columns and the entering y'_{k-W} come from LDS one step ahead.
      constexpr int W = kBsWindow;
      const int g = lane / 6, c = lane % 6;
      const bool act = lane < 6 * W;
      auto jj_of = [&](int k) {  // block row of group g in the window of step k
        const int m = ((k - 1 - g) % W + W) % W;
        return k - 1 - m;
      };
      auto load_L = [&](int k, double (&Lk)[21], double (&rk)[6]) {
        const double* o = kf + 36l * k;
#pragma unroll
        for (int e2 = 0; e2 < 20; e2 += 2) {
          const double2 v = reinterpret_cast<const double2*>(o)[e2 / 2];
          Lk[e2] = v.x;
          Lk[e2 + 1] = v.y;
        }
        Lk[20] = o[20];
        ld6(o + 24, rk);
      };
      // column c of block (k, jj_of(k)) or 0; (fk, ok) = (first[k], off[k]) were read a step
      // earlier.  Loads are unconditional (clamped addresses, select afterwards): a load
      // under a branch makes the waitcnt pass drain every outstanding prefetch.
      auto load_col = [&](int k, int fk, int okk, double (&col)[6]) {
        const int jj = jj_of(k);
        const bool on = act && jj >= fk && jj < k;
        const double* b = Sm + 36l * (on ? okk + jj - fk : 0) + c;
#pragma unroll
        for (int rr = 0; rr < 6; ++rr) {
          const double v = b[6 * rr];
          col[rr] = on ? v : 0.0;
        }
      };
      double acc = 0.0;
      {
        const int jj = jj_of(F);
        if (act && jj >= 0) acc = kf[36l * jj + 30 + c];
      }
      // Two register sets used alternately (the loop is unrolled by two), so the
      // prefetched operands are never copied (each VALU op costs a wave 4 cycles).
      struct Ops {
        double L[21], r[6], col[6];
        int f, o;  // first[], off[] of the step after the one these operands serve
      };
      Ops s0, s1;
      load_L(F - 1, s0.L, s0.r);
      load_col(F - 1, t_first[F - 1], t_off[F - 1], s0.col);
      s0.f = t_first[F >= 2 ? F - 2 : 0];
      s0.o = t_off[F >= 2 ? F - 2 : 0];
      auto step = [&](int k, Ops& cur, Ops& nxt) {
        const int kn = k > 0 ? k - 1 : 0, kn2 = k > 1 ? k - 2 : 0;
        nxt.f = t_first[kn2];
        nxt.o = t_off[kn2];
        load_L(kn, nxt.L, nxt.r);
        load_col(kn, cur.f, cur.o, nxt.col);
        const int ent = k - W;  // block row entering the window of step k
        const double init_v = kf[36l * (ent >= 0 ? ent : 0) + 30 + c];
        const double init = ent >= 0 ? init_v : 0.0;
        const int src = 6 * (k % W);
        double x[6];
#pragma unroll
        for (int cc = 0; cc < 6; ++cc) {
          const int lo = __builtin_amdgcn_readlane(__double2loint(acc), src + cc);
          const int hi = __builtin_amdgcn_readlane(__double2hiint(acc), src + cc);
          x[cc] = __hiloint2double(hi, lo);
        }
        bwd6(cur.L, cur.r, x);
        if (lane == 0) st6(kf + 36l * k + 30, x);
        if (g == k % W) acc = init;
        acc -= cur.col[0] * x[0] + cur.col[1] * x[1] + cur.col[2] * x[2] + cur.col[3] * x[3] +
               cur.col[4] * x[4] + cur.col[5] * x[5];
      };
      int k = F - 1;
      for (; k >= 1; k -= 2) {
        step(k, s0, s1);
        step(k - 1, s1, s0);
      }
      if (k == 0) step(0, s0, s1);
    } else {
      // Wide rows: x_k, then y'_j -= L_kj^T x_k through LDS, one lane per (block, column).
      for (int k = F - 1; k >= 0; --k) {
        const double* o = kf + 36l * k;
        double Lk[21], rk[6], x[6];
#pragma unroll
        for (int e2 = 0; e2 < 20; e2 += 2) {
          const double2 v = reinterpret_cast<const double2*>(o)[e2 / 2];
          Lk[e2] = v.x;
          Lk[e2 + 1] = v.y;
        }
        Lk[20] = o[20];
        ld6(o + 24, rk);
        ld6(o + 30, x);
        bwd6(Lk, rk, x);
        const int fk = t_first[k], ok_ = t_off[k];
        wave_sync<true>();
        if (lane == 0) st6(kf + 36l * k + 30, x);
        for (int t = lane; t < 6 * (k - fk); t += 64) {
          const int jj = fk + t / 6, cc = t % 6;
          const double* Lkj = Sm + 36l * (ok_ + jj - fk);
          double a = 0.0;
#pragma unroll
          for (int rr = 0; rr < 6; ++rr) a += Lkj[6 * rr + cc] * x[rr];
          kf[36l * jj + 30 + cc] -= a;
        }
        wave_sync<true>();
      }
    }
  }
  __syncthreads();
  mark(kS3Backsub);
  const bool failed = s_fail != 0;
  for (int e = tid; e < 6 * F; e += kThr) A.dc[e] = failed ? 0.0 : kf[36l * (e / 6) + 30 + e % 6];
  for (int c = tid; c < A.n_poses; c += kThr) {
    const double* T = pose_l + 12 * c;
    double* out = A.pose_next + 12 * c;
    if (failed || c < A.n_fixed) {
      for (int e = 0; e < 12; ++e) out[e] = T[e];
    } else {
      const double* d6 = kf + 36l * (c - A.n_fixed) + 30;
      double d[6];
      for (int e = 0; e < 6; ++e) d[e] = d6[e];
      se3_exp_apply(d, T, out);
    }
  }
  if (tid == 0 && failed && !prior_fail) *A.status = A.iter_tag;
  mark(kS3Tail);
  if (kStamp && tid == 0 && A.stamps)
    for (int k = 0; k < kS3Count; ++k) A.stamps[k] = st_acc[k];
}


// Chunk images taken over from the previous plan: runs of consecutive chunks copied on the
// device by a kernel (hipMemcpyAsync device-to-device went through a copy engine at ~12 GB/s on
// some boxes: 0.36-0.45 ms for a slid cfg3 window's 3.5 MB).  The runs travel in the arguments.
__global__ __launch_bounds__(64) void ba_img_copy_kernel(const uint4* __restrict__ prev, uint4* __restrict__ cur,
                                                          ImgRuns R) {
  constexpr int kVec = (int)(sizeof(ChunkImg) / 16);
  const int b = blockIdx.x;
  int r = 0;
  while (r + 1 < R.n && R.end[r] <= b) ++r;  // uniform
  const int off = b - (r ? R.end[r - 1] : 0);
  const uint4* s = prev + (long)(R.src[r] + off) * kVec;
  uint4* d = cur + (long)(R.dst[r] + off) * kVec;
  uint4 v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = s[min((int)threadIdx.x + 64 * k, kVec - 1)];
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if ((int)threadIdx.x + 64 * k < kVec) d[threadIdx.x + 64 * k] = v[k];
}
static_assert(sizeof(ChunkImg) / 16 <= 192, "three 16-byte pieces per lane");

// The read-out of vo_ba_residuals: one lane per observation in the problem's order; K1's
// projection arithmetic (lin_obs: the same operation order, rcp_nr), unweighted.  A template, so
// that it is emitted where it is instantiated (launch_obs_residual, the end of this unit), behind
// every K1 instantiation, so the plain K1 kernels keep the place in the code object they had
// before this kernel existed.  An observation, not a law: emitted ahead of them, two benchmark
// jobs of three runs read 0.0-0.1 % lower, which is about the run-to-run spread (DESIGN.md
// §Robust cost); a later kernel placed ahead of K1 changes the layout again and should be
// measured the same way.
template <int kThreads>
__global__ __launch_bounds__(kThreads) void ba_obs_residual_kernel(ObsResidualArgs A) {
  const int o = blockIdx.x * kThreads + threadIdx.x;
  if (o >= A.n_obs) return;
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
  A.err2[o] = r0 * r0 + r1 * r1;
  A.depth[o] = z;
}

// ---- host launches (ba_kernels.h) ---------------------------------------------------------
// K1 of one mode: the one-wave kernel of nw = 1 .. kWaveMaxChunks chunks per segment, else
// (nw = 0) the four-wave kernel.
template <int MODE, int... I>
void lin_launch(const LinArgs& A, int nw, dim3 g, hipStream_t st, std::integer_sequence<int, I...>) {
  const bool wave = ((nw == I + 1 &&
                      (ba_lin_wave_kernel<MODE, kBaStamps, I + 1><<<g, dim3(kLinLanesWave * nw), 0, st>>>(A), true)) ||
                     ...);
  if (!wave) ba_lin_kernel<MODE, kBaStamps><<<g, dim3(kLinThreads), 0, st>>>(A);
}

template <bool kLds>
void solve_launch(const SolveArgs& A, size_t lds_bytes, hipStream_t st) {
  hipLaunchKernelGGL((ba_solve_kernel<kLds, kBaStamps, 4>), dim3(1), dim3(256), lds_bytes, st, A);
}
// the kernel's dynamic-LDS limit, raised only when a window needs more than any before it
// (a process-wide attribute of the kernel)
template <bool kL>
void set_solve_lds(int lds) {
  static std::atomic<int> set{-1};
  int cur = set.load(std::memory_order_relaxed);
  if (lds <= cur) return;
  VO_HIP_CHECK(hipFuncSetAttribute((const void*)ba_solve_kernel<kL, kBaStamps, 4>,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  while (cur < lds && !set.compare_exchange_weak(cur, lds, std::memory_order_relaxed)) {
  }
}

// the step-control (kLm) instantiations, launched from the end of this unit
void launch_lin_lm(const LinArgs& A, int mode, int wave_chunks, int grid, hipStream_t st);
void launch_reduce_lm(const ReduceArgs& A, int workgroups, hipStream_t st);

}  // namespace

void launch_lin(const LinArgs& A, int mode, int wave_chunks, int grid, hipStream_t st) {
  constexpr std::make_integer_sequence<int, kWaveMaxChunks> nws{};
  if (mode & kLm) return launch_lin_lm(A, mode, wave_chunks, grid, st);
  switch (mode) {
    case kAccum: lin_launch<kAccum>(A, wave_chunks, dim3(grid), st, nws); break;
    case kBacksub | kAccum: lin_launch<kBacksub | kAccum>(A, wave_chunks, dim3(grid), st, nws); break;
    case kBacksub: lin_launch<kBacksub>(A, wave_chunks, dim3(grid), st, nws); break;
    case 0: lin_launch<0>(A, wave_chunks, dim3(grid), st, nws); break;
    // the Huber variants (A.huber > 0): instantiations of their own, the ones above keep their code
    case kRobust | kAccum: lin_launch<kRobust | kAccum>(A, wave_chunks, dim3(grid), st, nws); break;
    case kRobust | kBacksub | kAccum:
      lin_launch<kRobust | kBacksub | kAccum>(A, wave_chunks, dim3(grid), st, nws);
      break;
    case kRobust | kBacksub: lin_launch<kRobust | kBacksub>(A, wave_chunks, dim3(grid), st, nws); break;
    default: lin_launch<kRobust>(A, wave_chunks, dim3(grid), st, nws); break;
  }
}

void launch_reduce(const ReduceArgs& A, int workgroups, hipStream_t st) {
  if (A.lm_lambda) return launch_reduce_lm(A, workgroups, st);
  hipLaunchKernelGGL(ba_reduce_kernel, dim3(workgroups), dim3(kRedThreads), 0, st, A);
}

void launch_profile_solve(const SolveArgs& A, bool lds_profile, size_t lds_bytes, hipStream_t st) {
  if (lds_profile) solve_launch<true>(A, lds_bytes, st);
  else solve_launch<false>(A, lds_bytes, st);
}

void profile_solve_set_attributes(size_t lds_bytes) {
  set_solve_lds<true>((int)lds_bytes);
  set_solve_lds<false>((int)lds_bytes);
}

void launch_img_copy(const uint4* prev, uint4* cur, const ImgRuns& R, int chunks, hipStream_t st) {
  hipLaunchKernelGGL(ba_img_copy_kernel, dim3(chunks), dim3(64), 0, st, prev, cur, R);
}

// (last: the read-out kernel is instantiated here, see ba_obs_residual_kernel)
void launch_obs_residual(const ObsResidualArgs& A, hipStream_t st) {
  constexpr int kThreads = 256;
  if (A.n_obs <= 0) return;
  hipLaunchKernelGGL(ba_obs_residual_kernel<kThreads>, dim3((A.n_obs + kThreads - 1) / kThreads), dim3(kThreads), 0,
                     st, A);
}

// ---- Levenberg-Marquardt step control (vo_ba_run_lm, DESIGN.md §Step control) --------------
// Everything below is emitted behind the kernels above (templates instantiated here), so those
// keep their place in the code object (see the note at ba_obs_residual_kernel).
namespace {

// K2 with the camera damping read from the device (ReduceArgs::lm_lambda): ba_reduce_kernel's
// loads, partition and summation order restated, as in the fused launch's reducers
// (ba_band.hip band_reduce_wg), so all three give sys the same bits for the same damping.  A
// kernel of its own, not a shared inlined body: with one, ba_reduce_kernel's code changed (its
// status test went from a scalar to a vector load), and the GN path keeps its kernels as they are.
template <int kThreads>
__global__ __launch_bounds__(kThreads) void ba_reduce_lm_kernel(ReduceArgs A) {
  static_assert(kThreads == kRedThreads, "K2's partition");
  __shared__ __attribute__((aligned(16))) double part[kRedSParts * 36];
  __shared__ double partb[kRedBParts * 6];
  const int blk = blockIdx.x, tid = threadIdx.x;
  if (blk < A.nprof) {
    const int4 m = A.meta[blk];
    const int2 o = A.out[blk];
    const int failed = A.status ? *A.status : 0;
    const bool diag = m.z >= 0;
    double2 ps = make_double2(0.0, 0.0);
    double pb = 0.0;
    if (tid < kRedSParts * 18) ps = sum_rows2(A.slab, m.x, m.y, tid / 18, kRedSParts, tid % 18);
    if (diag && tid < kRedBParts * 6) pb = sum_rows<6>(A.slab_b, m.z, m.w, tid / 6, kRedBParts, tid % 6);
    if (failed) return;  // uniform
    if (tid < kRedSParts * 18) reinterpret_cast<double2*>(part)[tid] = ps;
    if (tid < kRedBParts * 6) partb[tid] = pb;
    __syncthreads();
    if (tid < 36) {
      double acc = 0.0;
#pragma unroll
      for (int q = 0; q < kRedSParts; ++q) acc += part[36 * q + tid];
      if (diag && tid % 7 == 0) acc += *A.lm_lambda;
      A.sys[(o.x & ~kRedTranspose) + ((o.x & kRedTranspose) ? 6 * (tid % 6) + tid / 6 : tid)] = acc;
    } else if (diag && tid >= 64 && tid < 70) {  // another wave: the rhs sum beside the S sum
      const int e = tid - 64;
      double acc = 0.0;
      for (int q = 0; q < kRedBParts; ++q) acc += partb[6 * q + e];
      A.sys[o.y + e] = acc;
    }
    return;
  }
  // cost: fixed-order lane-strided partial sums, then a fixed tree over the 256 lanes
  double c = 0.0;
  if (A.nseg > 0) {  // lane-strided, in order, every load of a batch in flight (sum_rows)
    for (int s = tid; s < A.nseg; s += 4 * kRedThreads) {
      double v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = A.slab_cost[min(s + i * kRedThreads, A.nseg - 1)];
#pragma unroll
      for (int i = 0; i < 4; ++i) c += s + i * kRedThreads < A.nseg ? v[i] : 0.0;
    }
  }
  if (A.status && *A.status) return;
  __shared__ double cpart[kRedThreads];
  cpart[tid] = c;
  __syncthreads();
  for (int m = kRedThreads / 2; m > 0; m >>= 1) {
    if (tid < m) cpart[tid] += cpart[tid + m];
    __syncthreads();
  }
  if (tid == 0) A.sys[A.cost_off] = cpart[0];
}

// The decision of one trial step (LmDecideArgs, ba_kernels.h).  The cost is summed exactly as
// K2's cost item sums it (lane-strided batches of four, then the tree over kRedThreads lanes), in
// every workgroup, so all of them hold the same bits and the same decision without a hand-off;
// the log entries read (k) and written (k + 1; trial and accepted at k) are different words.
// kStop: the termination tests in workgroup 0 (LmDecideArgs); without it, the loop that never stops.
template <int kThreads, bool kStop>
__global__ __launch_bounds__(kThreads) void ba_lm_decide_kernel(LmDecideArgs A) {
  static_assert(kThreads == kRedThreads, "K2's cost order");
  __shared__ double cpart[kThreads];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < A.nseg; i += 4 * kThreads) {
    double v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = A.slab_cost[min(i + u * kThreads, A.nseg - 1)];
#pragma unroll
    for (int u = 0; u < 4; ++u) s += i + u * kThreads < A.nseg ? v[u] : 0.0;
  }
  if constexpr (kStop) {
    // this launch's own stop (workgroup 0 was faster) is no earlier failure: the copies are made
    const int w = *A.status;
    if (w != 0 && w != (kLmStatusStopped | (A.k + 1))) return;
  } else {
    if (*A.status) return;  // a failed solve: the state stays the last accepted one (uniform)
  }
  cpart[tid] = s;
  __syncthreads();
  for (int m = kThreads / 2; m > 0; m >>= 1) {
    if (tid < m) cpart[tid] += cpart[tid + m];
    __syncthreads();
  }
  const double t = cpart[0];
  const bool init = A.k < 0;
  const double c = init ? 0.0 : A.cost[A.k];
  const double lam = init ? A.lambda0 : A.lambda[A.k];
  const bool acc = init || t < c;  // false for a NaN or +inf trial cost
  // accepted: the landmarks become the snapshot; rejected: they and the poses are restored
  const long n = 3l * A.n_points, stride = (long)gridDim.x * kThreads, i0 = (long)blockIdx.x * kThreads + tid;
  const double* src = acc ? A.points : A.snap;
  double* dst = acc ? A.snap : A.points;
  for (long i = i0; i < n; i += stride) dst[i] = src[i];
  if (!acc)
    for (long i = i0; i < 12l * A.n_poses; i += stride) A.pose_next[i] = A.pose_cur[i];
  if (blockIdx.x == 0 && tid == 0) {
    if (init) {
      A.cost[0] = t;
      A.lambda[0] = lam;
    } else {
      double l = lam * (acc ? A.down : A.up);
      if (acc && l < A.lambda_min) l = A.lambda_min;
      if (!acc && l > A.lambda_max) l = A.lambda_max;
      A.trial[A.k] = t;
      A.accepted[A.k] = acc ? 1 : 0;
      A.cost[A.k + 1] = acc ? t : c;
      A.lambda[A.k + 1] = l;
    }
  }
  if constexpr (kStop) {
    if (blockIdx.x != 0) return;
    if (init) {
      if (tid == 0) A.stop[0] = A.stop[1] = 0;
      return;
    }
    int reason = kLmRanAll;  // (every branch below is uniform over the workgroup)
    if (acc) {
      if (A.ftol > 0.0 && (c - t) <= A.ftol * c) {
        reason = kLmFtol;
      } else if (A.xtol > 0.0) {
        double m = 0.0;
        for (int i = tid; i < A.n_dc; i += kThreads) m = fmax(m, fabs(A.dc[i]));
        __syncthreads();  // every thread has read the cost sum
        cpart[tid] = m;
        __syncthreads();
        for (int h = kThreads / 2; h > 0; h >>= 1) {
          if (tid < h) cpart[tid] = fmax(cpart[tid], cpart[tid + h]);
          __syncthreads();
        }
        if (cpart[0] <= A.xtol) reason = kLmXtol;
      }
    } else if (A.max_rejects > 0) {
      // consecutive rejections, this one included: the decisions earlier launches logged
      int rej = 1;
      for (int j = A.k - 1; j >= 0 && rej < A.max_rejects && A.accepted[j] == 0; --j) ++rej;
      if (rej >= A.max_rejects) reason = kLmRejects;
    }
    if (tid == 0 && reason != kLmRanAll) {
      A.stop[0] = A.k + 1;
      A.stop[1] = reason;
      *A.status = kLmStatusStopped | (A.k + 1);
    }
  }
}

// End of a run with a termination criterion: a status word that is exactly a stop word goes back
// to zero, so the next run starts as after any successful one; a failure tag, or a stop word a
// later fused launch added its timeout flag to, stays for the host to report.  (A template only so
// that it is emitted where it is instantiated, behind every earlier kernel of the code object.)
template <int kThreads>
__global__ __launch_bounds__(kThreads) void ba_lm_finish_kernel(int* status) {
  if (threadIdx.x != 0) return;
  const int w = *status;
  if ((w & ~(kLmStatusStopped - 1)) == kLmStatusStopped) *status = 0;  // the flag and a trial count below it
}

void launch_lin_lm(const LinArgs& A, int mode, int wave_chunks, int grid, hipStream_t st) {
  constexpr std::make_integer_sequence<int, kWaveMaxChunks> nws{};
  switch (mode) {
    case kLm | kAccum: lin_launch<kLm | kAccum>(A, wave_chunks, dim3(grid), st, nws); break;
    case kLm | kBacksub: lin_launch<kLm | kBacksub>(A, wave_chunks, dim3(grid), st, nws); break;
    case kLm | kRobust | kAccum: lin_launch<kLm | kRobust | kAccum>(A, wave_chunks, dim3(grid), st, nws); break;
    case kLm | kRobust | kBacksub: lin_launch<kLm | kRobust | kBacksub>(A, wave_chunks, dim3(grid), st, nws); break;
    default: VO_REQUIRE(false, VO_ERR_STATE, "K1: no step-control instantiation of mode %d", mode);
  }
}

void launch_reduce_lm(const ReduceArgs& A, int workgroups, hipStream_t st) {
  hipLaunchKernelGGL(ba_reduce_lm_kernel<kRedThreads>, dim3(workgroups), dim3(kRedThreads), 0, st, A);
}

}  // namespace

int lm_decide_grid(int n_points) {
  return (int)std::min<long>(128, std::max<long>(1, (3l * n_points + 4 * kRedThreads - 1) / (4 * kRedThreads)));
}

void launch_lm_decide(const LmDecideArgs& A, bool stop, hipStream_t st) {
  const dim3 grid(lm_decide_grid(A.n_points));
  if (!stop) hipLaunchKernelGGL((ba_lm_decide_kernel<kRedThreads, false>), grid, dim3(kRedThreads), 0, st, A);
  else hipLaunchKernelGGL((ba_lm_decide_kernel<kRedThreads, true>), grid, dim3(kRedThreads), 0, st, A);
}

void launch_lm_finish(int* status, hipStream_t st) {
  hipLaunchKernelGGL(ba_lm_finish_kernel<64>, dim3(1), dim3(64), 0, st, status);
}

}  // namespace vo
