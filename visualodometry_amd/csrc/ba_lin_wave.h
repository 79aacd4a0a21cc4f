// The one-wave K1 (ba_lin_wave_kernel) as a device function: its LDS image, its helpers and its
// body, shared by the stand-alone kernels in ba.hip and by the chained instantiation of the fused
// K2 + K3 launch in ba_band.hip, which runs the next iteration's K1 segments behind a pose gate.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <utility>

#include "ba_kernels.h"
#include "ba_math.h"
#include "vo_common.h"

namespace vo {

namespace {

constexpr double kPivotRelEps = 1e-12;  // == oracle/ba_ref.py PIVOT_REL_EPS

enum { kPhLoad = 0, kPhBacksub, kPhLinObs, kPhReduce, kPhElim, kPhSchur, kPhWrite, kPhSchurU, kPhT0, kPhT1,
       // per-segment work counts (cost-model fitting): observations, track entries,
       // landmarks, pair-list entries, window slots, window cameras
       kPhObs, kPhTe, kPhPts, kPhPairs, kPhSlots, kPhCams, kPhEnd };
static_assert(kPhEnd == kPhCount, "K1 stamp row (ba_kernels.h)");
template <bool kStamp>
struct Stamper {
  // the stamping lane (thread 0, or lane 0 of each one-wave segment) and its output row;
  // s_memtime counts per XCD (clocks of different XCDs are unrelated), so the row's
  // window-camera count carries the XCD id in bits 24..31 (and the wave's SIMD id in bits 32..33)
  unsigned long long t = 0, acc[kPhCount] = {};
  bool lead = false;
  int row = 0;
  __device__ __forceinline__ void start(bool ld, int r) {
    lead = kStamp && ld;
    row = r;
    if (lead) {
      acc[kPhT0] = t = __builtin_amdgcn_s_memtime();
      unsigned xcc;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
      // HW_ID (hwreg 4) bits 4..5: the SIMD this wave runs on, kept in bits 32..33
      const unsigned simd = __builtin_amdgcn_s_getreg(4 | (4 << 6) | ((2 - 1) << 11));
      acc[kPhCams] = (unsigned long long)xcc << 24 | (unsigned long long)simd << 32;
    }
  }
  __device__ __forceinline__ void start() { start(threadIdx.x == 0, blockIdx.x); }
  __device__ __forceinline__ void mark(int ph) {
    if (lead) {
      const unsigned long long n = __builtin_amdgcn_s_memtime();
      acc[ph] += n - t;
      t = n;
    }
  }
  __device__ __forceinline__ void count(int k, int v) {
    if (lead) acc[k] += (unsigned long long)v;
  }
  __device__ __forceinline__ void flush(unsigned long long* out) {
    if (lead) acc[kPhT1] = __builtin_amdgcn_s_memtime();  // absolute
    if (lead && out)
      for (int k = 0; k < kPhCount; ++k) out[(long)row * kPhCount + k] = acc[k];
  }
};

// Z rows of 18 doubles (36 dwords: the rows start on 16 different 4-bank offsets of gfx950's
// 64 banks, so a ds_read_b128 of 16 lanes on random rows rarely conflicts; a 24-double row of
// Z | bt started on 4 offsets only, a 4-way conflict on every Schur load)
// The one-wave K1's phase boundary: its workgroup is one wave, whose LDS operations complete
// in order, so a phase only needs its LDS writes done and the compiler kept from moving LDS
// accesses across (no s_barrier; and no workgroup fence, which would also wait for every
// outstanding global store: the back substitution's points and the slab rows).
__device__ __forceinline__ void lds_sync_wave() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

constexpr int kZbStride = 18;                  // doubles per track entry's Z row
constexpr int kZbR = 6 * kChunkObs;            // r (2 per observation) after Jp (6 per observation)
constexpr int kZbDc = kZbR + 2 * kChunkObs;    // back substitution: dc of the window cameras
constexpr int kZbPoseO = kZbDc + 6 * kSegCams; // back substitution: poses of the pending step
static_assert(kZbPoseO + 12 * kSegAllCams <= kChunkTe * kZbStride, "Zb region aliases");

struct alignas(16) LinWave {
  ChunkImg img;
  int spos[kSegSlots];
  int cpos[kSegCams];
  alignas(16) double Jc[kChunkObs][10];  // compressed camera Jacobian rows (jc_load)
  alignas(16) double zb[kChunkTe * kZbStride];
  alignas(16) double bt[kChunkTe][6];
  double X[kChunkPts][3];
  double L[kChunkPts][6];  // 1/l00, l10, 1/l11, l20, l21, 1/l22
  double h[kChunkPts][3];
  alignas(16) double pose_n[kSegAllCams][12];  // after the linearisation: the chunk's b sums by window camera
  uint8_t valid[kChunkPts];
  // segments of several chunks (one wave each): per window slot the scratch row of this chunk's
  // block (0xFF: not active here), per window camera whether the chunk has its b, the cost
  uint8_t srow[kSegSlots];
  uint8_t crow[kSegCams];
  double wcost;
};
// six per CU (cfg3's 1362 chunks in one round on 256 CUs); segments of two chunks: three
// workgroups of two waves, of three chunks: two of three
constexpr int kWaveSegsPerCu = 6;
static_assert(sizeof(LinWave) <= 160 * 1024 / kWaveSegsPerCu, "one-wave K1 LDS image");
static_assert(kWaveMaxChunks <= 8 && kWaveMaxChunks * sizeof(LinWave) <= 160 * 1024 &&
                  kWaveItems * 36 * sizeof(double) <= 2176 * sizeof(double),
              "the chunks of a segment fit one CU; every item's block fits the scratch rows");

// point_block over the Zb region's Jp | r (same operation order)
__device__ __forceinline__ bool point_block_w(const LinWave& S, double lambda, int p, double (&l)[6],
                                              double (&h)[3]) {
  double v00 = 0, v01 = 0, v02 = 0, v11 = 0, v12 = 0, v22 = 0, g0 = 0, g1 = 0, g2 = 0;
  const int o0 = S.img.pt_obs[p], o1 = S.img.pt_obs[p + 1];
  for (int o = o0; o < o1; ++o) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double a = S.zb[6 * o + 3 * k], b = S.zb[6 * o + 3 * k + 1], c = S.zb[6 * o + 3 * k + 2];
      const double rk = S.zb[kZbR + 2 * o + k];
      v00 += a * a; v01 += a * b; v02 += a * c;
      v11 += b * b; v12 += b * c; v22 += c * c;
      g0 += a * rk; g1 += b * rk; g2 += c * rk;
    }
  }
  v00 += lambda; v11 += lambda; v22 += lambda;
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

// Residual and Jacobians of observation o at pose T (lin_obs / chunk_backsub arithmetic);
// r and Jp into the Zb region, Jc (kJc) into S.Jc.  The back substitution (kBack) adds
// Jc dc for a free camera (dc non-null) and sums no cost.  kRob: as lin_obs / chunk_backsub -- the
// Huber scale of the raw residual (before Jc dc) on r and the Jacobians, the cost sums rho.
// kWt (observation weights, DESIGN.md §Observation weights and culling): sw = sqrt(w_o) multiplies
// r and the Jacobians ahead of the Huber rule, which then sees the whitened residual; sw == 0 is a
// select, not a product, so an inactive observation with a non-finite raw residual leaves zeros.
template <bool kJc, bool kBack, bool kRob, bool kWt = false>
__device__ __forceinline__ void obs_lin_w(LinWave& S, const LinArgs& A, const double* T, int o,
                                          const double* dc, double& cost, double sw = 1.0) {
  const int q = S.img.obs_pt[o];
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
  if constexpr (kWt) {
    const bool on = sw > 0.0;
    r0 = on ? r0 * sw : 0.0; r1 = on ? r1 * sw : 0.0;
    j00 = on ? j00 * sw : 0.0; j02 = on ? j02 * sw : 0.0;
    j11 = on ? j11 * sw : 0.0; j12 = on ? j12 * sw : 0.0;
  }
  if constexpr (kRob) {
    double rho;
    const double s = huber_scale(r0, r1, A.huber, A.huber2, rho);
    if (!kBack) cost += rho;
    r0 *= s; r1 *= s;
    j00 *= s; j02 *= s; j11 *= s; j12 *= s;
  }
  if (kBack && dc) {
    r0 += j00 * dc[0] + j02 * dc[2] + (j02 * y) * dc[3] + (j00 * z - j02 * x) * dc[4] - (j00 * y) * dc[5];
    r1 += j11 * dc[1] + j12 * dc[2] + (j12 * y - j11 * z) * dc[3] - (j12 * x) * dc[4] + (j11 * x) * dc[5];
  }
  if (!kBack && !kRob) cost += r0 * r0 + r1 * r1;
  S.zb[kZbR + 2 * o] = r0;
  S.zb[kZbR + 2 * o + 1] = r1;
  if (kJc) {  // compressed rows (jc_load): row 0 without column 1, row 1 without column 0
    double2* jc = reinterpret_cast<double2*>(S.Jc[o]);
    jc[0] = make_double2(j00, j02);
    jc[1] = make_double2(j02 * y, j00 * z - j02 * x);
    jc[2] = make_double2(-j00 * y, j11);
    jc[3] = make_double2(j12, j12 * y - j11 * z);
    jc[4] = make_double2(-j12 * x, j11 * x);
  }
  double* jp = &S.zb[6 * o];
  jp[0] = j00 * T[0] + j02 * T[6];
  jp[1] = j00 * T[1] + j02 * T[7];
  jp[2] = j00 * T[2] + j02 * T[8];
  jp[3] = j11 * T[3] + j12 * T[6];
  jp[4] = j11 * T[4] + j12 * T[7];
  jp[5] = j11 * T[5] + j12 * T[8];
}

// Observation o's camera Jacobian rows from the compressed LDS row (10 doubles: row 0 without
// its structural zero at column 1, row 1 without column 0; 80-byte rows start on 16 bank
// offsets)
__device__ __forceinline__ void jc_load(const LinWave& S, int o, double (&jj)[12]) {
  const double2* jr = reinterpret_cast<const double2*>(S.Jc[o]);
  const double2 a = jr[0], b = jr[1], c = jr[2], d = jr[3], e = jr[4];
  jj[0] = a.x; jj[1] = 0.0; jj[2] = a.y; jj[3] = b.x; jj[4] = b.y; jj[5] = c.x;
  jj[6] = 0.0; jj[7] = c.y; jj[8] = d.x; jj[9] = d.y; jj[10] = e.x; jj[11] = e.y;
}

// One lane's Schur item (one-wave K1): active slot si's block, -sum over the slot's pairs of
// Z_x Z_y^T as FMA chains with both Z rows in registers (pair j+1's rows fetched while pair j
// accumulates); a diagonal slot's lane adds U over its pairs' observations (pair (x, x): track
// entry x of the slot's camera).  The block goes straight to its slab row.
template <bool kGroup, class Stamp>
__device__ __forceinline__ void schur_block(LinWave& S, const LinArgs& A, int si, bool live, Stamp& st) {
  double out[36];
#pragma unroll
  for (int e = 0; e < 36; ++e) out[e] = 0.0;
  const int e0 = S.img.slotp[si], n = live ? S.img.apcnt[si] : 0;
  const int dcam = S.img.adcam[si], s = S.img.aslot[si];
  if (n > 0) {
    auto zload = [&](int pr, double2 (&zx)[9], double2 (&zy)[9]) {
      const double2* px = reinterpret_cast<const double2*>(&S.zb[kZbStride * (pr & 255)]);
      const double2* py = reinterpret_cast<const double2*>(&S.zb[kZbStride * (pr >> 8)]);
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        zx[k] = px[k];
        zy[k] = py[k];
      }
    };
    auto accum = [&](const double2 (&zx)[9], const double2 (&zy)[9]) {
      const double* x = reinterpret_cast<const double*>(zx);
      const double* y = reinterpret_cast<const double*>(zy);
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          double v = out[6 * i + j];
          v = __builtin_fma(-x[3 * i], y[3 * j], v);
          v = __builtin_fma(-x[3 * i + 1], y[3 * j + 1], v);
          out[6 * i + j] = __builtin_fma(-x[3 * i + 2], y[3 * j + 2], v);
        }
    };
    auto pid = [&](int j) { return (int)S.img.pairs[e0 + min(j, n - 1)]; };
    double2 zxA[9], zyA[9], zxB[9], zyB[9];
    zload(pid(0), zxA, zyA);
    int pn = pid(1);
    int j = 0;
    for (; j + 2 <= n; j += 2) {
      zload(pn, zxB, zyB);
      pn = pid(j + 2);
      accum(zxA, zyA);
      zload(pn, zxA, zyA);
      pn = pid(j + 3);
      accum(zxB, zyB);
    }
    if (j < n) accum(zxA, zyA);
  }
  st.mark(kPhSchur);  // stamped builds: the pair sums
  // a diagonal item: U over its pairs' observations (camol entries [auo[si], auo[si + 1]), in
  // observation order, observation i + 1's Jc fetched while i accumulates) and its share of
  // b over its pairs (track entry x's bt row)
  double ob[6] = {0, 0, 0, 0, 0, 0};
  const int u0 = S.img.auo[si], un = live ? S.img.auo[si + 1] - u0 : 0;
  if (un > 0) {
    auto uacc = [&](const double (&jj)[12]) {
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int c = 0; c < 6; ++c)
          out[6 * i + c] = __builtin_fma(jj[6 + i], jj[6 + c], __builtin_fma(jj[i], jj[c], out[6 * i + c]));
    };
    auto oid = [&](int i) { return (int)S.img.camol[u0 + min(i, un - 1)]; };
    double jA[12], jB[12];
    jc_load(S, oid(0), jA);
    int on = oid(1);
    int i = 0;
    for (; i + 2 <= un; i += 2) {
      jc_load(S, on, jB);
      on = oid(i + 2);
      uacc(jA);
      jc_load(S, on, jA);
      on = oid(i + 3);
      uacc(jB);
    }
    if (i < un) uacc(jA);
  }
  if (n > 0 && dcam != 0xFF) {
    int xn = S.img.pairs[e0] & 255;
    for (int e = 0; e < n; ++e) {
      const double2* br = reinterpret_cast<const double2*>(S.bt[xn]);
      xn = S.img.pairs[e0 + min(e + 1, n - 1)] & 255;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double2 v = br[k];
        ob[2 * k] += v.x;
        ob[2 * k + 1] += v.y;
      }
    }
  }
  if (!live) {
    st.mark(kPhSchurU);
    return;
  }
  if (dcam != 0xFF) {  // this copy's share of the camera's b, for rhs_rows (the X | L | h region is dead)
    double2* bp = reinterpret_cast<double2*>(&S.X[0][0]) + 3 * si;
#pragma unroll
    for (int k = 0; k < 3; ++k) bp[k] = make_double2(ob[2 * k], ob[2 * k + 1]);
  }
  if (!kGroup && S.img.anp[si] <= 1) {  // a slot of one item: its slab row
    double2* w = reinterpret_cast<double2*>(&A.slab[36l * S.spos[s]]);
#pragma unroll
    for (int e = 0; e < 18; ++e) w[e] = make_double2(out[2 * e], out[2 * e + 1]);
  } else {  // a copy (or any item of a multi-chunk segment): its block to the scratch (Jc | Z | bt)
    lds_sync_wave();  // every lane's reads of that region are done (one wave, in order)
    double2* w = reinterpret_cast<double2*>(&S.Jc[0][0]) + 18 * si;
#pragma unroll
    for (int e = 0; e < 18; ++e) w[e] = make_double2(out[2 * e], out[2 * e + 1]);
  }
  st.mark(kPhSchurU);  // stamped builds: U, the b partials and the block's slab stores
}

// A slot's copies (one-wave K1): copy k of m sums entries [36 k / m, 36 (k + 1) / m) of the
// slot's m partial blocks (scratch rows of consecutive items) in copy order into the slab row
// (kGroup: into the first copy's scratch row, for the segment's combine; copy k only ever reads
// and writes entry range k of that row).
static_assert(offsetof(LinWave, zb) == offsetof(LinWave, Jc) + sizeof(LinWave::Jc) &&
                  offsetof(LinWave, bt) == offsetof(LinWave, zb) + sizeof(LinWave::zb) &&
                  sizeof(LinWave::Jc) + sizeof(LinWave::zb) + sizeof(LinWave::bt) >= 36 * sizeof(double) * kWaveItems,
              "the copies' scratch (kWaveItems items) fits the Jc | Z | bt region");
template <bool kGroup>
__device__ __forceinline__ void copy_rows(LinWave& S, const LinArgs& A, int si, bool live) {
  const int m = S.img.anp[si];
  if (!live || m <= 1) return;
  const int k = S.img.acopy[si], j0 = si - k;
  const int e0 = 36 * k / m, ne = 36 * (k + 1) / m - e0;  // <= 18 entries (m >= 2)
  double* sc = &S.Jc[0][0] + 36 * j0 + e0;
  double acc[18];
#pragma unroll
  for (int i = 0; i < 18; ++i) acc[i] = sc[min(i, ne - 1)];  // every load of a copy in flight
  int c = 1;
  for (; c + 2 <= m; c += 2) {  // two copies' loads in flight, added in copy order
    double v[18], u[18];
#pragma unroll
    for (int i = 0; i < 18; ++i) {
      v[i] = sc[36 * c + min(i, ne - 1)];
      u[i] = sc[36 * (c + 1) + min(i, ne - 1)];
    }
#pragma unroll
    for (int i = 0; i < 18; ++i) acc[i] = (acc[i] + v[i]) + u[i];
  }
  if (c < m)
#pragma unroll
    for (int i = 0; i < 18; ++i) acc[i] += sc[36 * c + min(i, ne - 1)];
  double* row = kGroup ? sc : &A.slab[36l * S.spos[S.img.aslot[si]] + e0];
#pragma unroll
  for (int i = 0; i < 18; ++i)
    if (i < ne) row[i] = acc[i];
}

// The rhs of the chunk's window cameras (one-wave K1): lane (active camera ci, row a) adds row a
// of the camera's diagonal copies' partial sums (consecutive items cdiag0 .. + cdiagn, left in
// the X | L | h region by schur_block) in item order into its slab entry (kGroup: into the dead
// pose_n region by window camera, for the segment's combine).
template <bool kGroup>
__device__ __forceinline__ void rhs_rows(LinWave& S, const LinArgs& A, int nac, int tid) {
  static_assert(sizeof(S.X) + sizeof(S.L) + sizeof(S.h) >= 6 * sizeof(double) * kWaveSlots &&
                    offsetof(LinWave, L) == offsetof(LinWave, X) + sizeof(S.X) &&
                    offsetof(LinWave, h) == offsetof(LinWave, L) + sizeof(S.L),
                "b partials of every item fit the X | L | h region");
  const double* bp = &S.X[0][0];
  for (int q = tid; q < 6 * nac; q += kLinLanesWave) {
    const int ci = q / 6, a = q - 6 * ci;
    const int j0 = S.img.cdiag0[ci], nj = S.img.cdiagn[ci];
    double acc = 0.0;
    for (int j = 0; j < nj; j += 8) {  // eight partials' loads in flight, added in item order
      double v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = bp[6 * (j0 + min(j + k, nj - 1)) + a];
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (j + k < nj) acc += v[k];
    }
    if (kGroup) (&S.pose_n[0][0])[6 * S.img.acid[ci] + a] = acc;
    else A.slab_b[6l * S.cpos[S.img.acid[ci]] + a] = acc;
  }
}

// The one-wave K1 (wave plans, seg_obs == 1): one wave per chunk, NW chunks of one first-camera
// group per segment = workgroup (the plan's seg_chunks; chunk = segment * NW + wave, padded with
// empty chunks).  NW == 1: each item's block goes straight to its slab row.  NW > 1: the waves
// run on their own LDS images without waiting on each other, leave their blocks in their scratch
// rows, and after one workgroup barrier the segment's slots are summed over its chunks in chunk
// order into one slab row each (fewer rows for K2: one per segment slot, not per chunk slot).
// NW > 4: the waves of chunks 0..3 sum their own chunks' parts before that barrier, while the
// two waves that share a SIMD still run, and add the late chunks' parts after it.
static_assert(sizeof(LinWave::pose_n) >= kSegCams * 6 * sizeof(double), "the chunk's b sums fit pose_n");

// A 16-byte piece of a slab row from the combine, stored write-through (sc1): its readers are
// K2's workgroups on other XCDs, and a line left dirty in this XCD's L2 is written back at the
// kernel's end, on the next launch's path.  No flag or fence goes with it (the kernel boundary
// orders it as before).  The s_nop covers the wait state a wide store's data registers need.
__device__ __forceinline__ void slab_store(double2* p, double2 v) {
  typedef double f64x2 __attribute__((ext_vector_type(2)));
  const f64x2 d = {v.x, v.y};
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 0" ::"v"(p), "v"(d) : "memory");
}

// The pose gate of a K1 workgroup that rides in the solve launch of the iteration before its own
// (ba_band.hip, the chained instantiation).  Its solver publishes `want` (the launch's sequence
// number, shifted up one bit: never zero) once pose_new and dc are out, or `want | 1` when the
// solve failed or an earlier one had: the state is then frozen.
typedef __attribute__((address_space(3))) int lin_lds_int;
struct LinGate {
  const unsigned* pub = nullptr;  // the publish word this workgroup polls
  unsigned want = 0;
  int* status = nullptr;          // a gate that timed out records itself here, as the solver's waits do
  int iter_tag = 0;
  int timeout_flag = 0;           // kBandStatusTimeout (ba_band.h)
  lin_lds_int* s_gate = nullptr;  // LDS: the verdict, from the polling lane to every wave
  unsigned long long* stamps = nullptr;  // diagnostic build: start, prefix done, gate passed, end
};
// Spins of the gate's poll (s_sleep(2) + one sc1 load each, so no shorter than a spin of the
// solver's own polls: s_sleep(1) + one sc1 load).  The solver's bounded waits on the path to its
// publish are the prologue's column poll and the loader's band_cols_wait, 2^22 spins each; the
// gate allows four times their sum, so it cannot give up on a solver that still publishes.
constexpr unsigned kLinGateSpins = 1u << 25;

typedef __attribute__((address_space(1))) unsigned long long lin_gu64;
typedef __attribute__((address_space(1))) unsigned lin_gu32;
// an 8-byte sc1 (agent-scope relaxed) global load: L2-served, never this CU's L1
__device__ __forceinline__ double ld_sc1_f64(const double* p) {
  return __longlong_as_double((long long)__hip_atomic_load((lin_gu64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// The kernel's body.  Sw: the workgroup's NW LDS images; s_arrive_p: its arrival word (kEarly);
// seg: its segment.  kGated: see LinGate -- level 1 and the level-2 loads that do not depend on
// the solve (landmarks, pose_old, slab rows) and their LDS stores come before the gate, pose_new
// and dc behind it by sc1 loads only, and the body from the back substitution on is the same code.
// kWeighted modes: sqw holds sqrt(w) per observation in the plan's observation order (the chunk's
// first at header int 0); every other mode neither reads nor receives it.
template <int MODE, bool kStamp, int NW, bool kGated>
__device__ __forceinline__ void lin_wave_body(LinArgs A, LinWave* Sw, int* s_arrive_p, const int seg, const LinGate G,
                                              const double* sqw = nullptr) {
  int& s_arrive = *s_arrive_p;
  constexpr bool kGroup = NW > 1;
  constexpr bool kRob = (MODE & kRobust) != 0;
  constexpr bool kWt = (MODE & kWeighted) != 0;
  static_assert(!kWt || (kRob && !kGated), "weighted K1: the Huber code, never in the chained launch");
  if constexpr ((MODE & kLm) != 0) A.lambda = *A.lm_lambda;  // step control: the damping is on the device
  // the cross-chunk combine: its waves, whether they start before the late waves are done, and
  // a thread's 16-byte pieces of the slots' blocks and of the rhs
  constexpr int kCombWaves = NW < 4 ? NW : 4;
  constexpr bool kEarly = NW > kCombWaves && (MODE & kAccum);
  constexpr int kCombS = (kSegSlots * 18 + 64 * kCombWaves - 1) / (64 * kCombWaves);
  constexpr int kCombB = (kSegCams * 3 + 64 * kCombWaves - 1) / (64 * kCombWaves);
  static_assert(kLinLanesWave == 64, "one wave");
  static_assert(!kGated || (MODE & (kBacksub | kAccum | kLm)) == (kBacksub | kAccum), "the gated K1: a GN iteration's");
  const int wv = kGroup ? __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6) : 0;
  // NW > 4: waves 4.. run on the SIMDs of waves 0.. (measured: in every workgroup), and the
  // arbiter gives the older wave of a pair nearly every issue slot, so the younger one finishes
  // ~9k cycles after it, the last of them alone on its SIMD.  The younger wave holds priority 1
  // from its first instruction until its elimination is done (about half of a chunk's own work),
  // the older one has the rest: the pair ends closer together and the workgroup earlier.  wv is
  // an SGPR, so both s_setprio sit under scalar branches.
  constexpr bool kPrio = kEarly;
  if constexpr (kPrio)
    if (wv >= kCombWaves) __builtin_amdgcn_s_setprio(1);
  auto prio_drop = [&]() __attribute__((always_inline)) {
    if constexpr (kPrio)
      if (wv >= kCombWaves) __builtin_amdgcn_s_setprio(0);
  };
  LinWave& S = Sw[wv];
  const int tid = (int)threadIdx.x & 63, chk = seg * NW + wv;
  Stamper<kStamp> st;
  st.start(tid == 0, chk);
  // level 1: status, segment header (uniform), this lane's camera ids (fixed header offsets)
  // and the chunk's image (chunk = segment)
  const int* SH = A.seg_hdr + (long)kSegHdr * seg;
  const int4* SH4 = reinterpret_cast<const int4*>(SH);
  const int16_t* SH16 = reinterpret_cast<const int16_t*>(SH);
  const int stat = !kGated && A.status ? *A.status : 0;  // (gated: the publish word carries it)
  const int4 g0 = SH4[0], g1 = SH4[1];
  // this wave's chunk header: the segment header's copy (one chunk per segment), or its own
  const int4* CH = kGroup ? A.chunk_hdr + 4l * chk : SH4 + 8;
  const int4 h0 = CH[0], h1 = CH[1], h2 = CH[2], h3 = CH[3];
  constexpr int kImgVec = (int)(sizeof(ChunkImg) / 16);
  static_assert(kImgVec > 128 && kImgVec <= 192, "three 16-byte staging granules per lane");
  const uint4* img = reinterpret_cast<const uint4*>(A.chunk_img + chk);
  const uint4 img0 = img[tid], img1 = img[64 + tid], img2 = img[min(128 + tid, kImgVec - 1)];
  int i_acam[3], i_wcam[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    i_acam[k] = SH16[16 + min((tid + 64 * k) / 12, kSegAllCams - 1)];
    i_wcam[k] = SH16[32 + min((tid + 64 * k) / 6, kSegCams - 1)];
  }
  if (kEarly) {  // the arrival word starts at zero for every wave (under the level-1 loads)
    if (threadIdx.x == 0) s_arrive = 0;
    lds_sync_wave();  // (a bare barrier: a fence would wait for the loads in flight)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
  if (stat) return;  // a previous solve failed: state frozen
  const int nslots = g0.x, slot_off = g0.y, cam0 = g0.z, ncams = g0.w, na = g1.x;
  const int nob = h0.y, nte = h0.w, p0 = h1.x, npt = h1.y;
  double* dcw = &S.zb[kZbDc];
  double* pose_o = &S.zb[kZbPoseO];
  // level 2: landmarks, poses, pending update, slab rows
  double vx[2], vpn[3], vpo[3], vdc[3];
  const long xb = npt > 0 ? 3l * p0 : 0;  // an empty (padding) chunk may start past the last landmark
#pragma unroll
  for (int k = 0; k < 2; ++k) vx[k] = A.points[xb + min(tid + 64 * k, max(3 * npt - 1, 0))];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int e = tid + 64 * k;
    if (!kGated) vpn[k] = A.pose_new[12l * i_acam[k] + e % 12];
    if (MODE & kBacksub) {
      vpo[k] = A.pose_old[12l * i_acam[k] + e % 12];
      if (!kGated) vdc[k] = A.dc[6l * i_wcam[k] + e % 6];
    }
  }
  double sw = 1.0;
  if constexpr (kWt) sw = sqw[nob > 0 ? h0.x + min(tid, nob - 1) : 0];  // (a padding chunk: any entry)
  int vsp = 0, vcp = 0;
  if ((MODE & kAccum) && nslots > 0) {
    vsp = A.slab_pos[slot_off + min(tid, nslots - 1)];
    vcp = A.cam_pos[cam0 + min(tid, max(ncams - 1, 0))];
  }
  {
    uint4* d = reinterpret_cast<uint4*>(&S.img);
    d[tid] = img0;
    d[64 + tid] = img1;
    if (128 + tid < kImgVec) d[128 + tid] = img2;
  }
#pragma unroll
  for (int k = 0; k < 2; ++k)
    if (tid + 64 * k < 3 * npt) (&S.X[0][0])[tid + 64 * k] = vx[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int e = tid + 64 * k;
    if (e < 12 * na) {
      if (!kGated) (&S.pose_n[0][0])[e] = vpn[k];
      if (MODE & kBacksub) pose_o[e] = vpo[k];
    }
    if (!kGated && (MODE & kBacksub) && e < 6 * ncams) dcw[e] = vdc[k];
  }
  if (MODE & kAccum) {
    if (tid < nslots) S.spos[tid] = vsp;
    if (tid < ncams) S.cpos[tid] = vcp;
    if (kGroup) {
      S.srow[tid] = 0xFF;
      if (tid < kSegCams) S.crow[tid] = 0;
    }
  }
  if constexpr (kGated) {
#if VO_BA_STAMPS
    if (G.stamps && threadIdx.x == 0) {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // the prefix: loads in, LDS stores out
      G.stamps[1] = __builtin_amdgcn_s_memrealtime();
    }
#endif
    // The gate: one lane polls the publish word by relaxed agent-scope (sc1) loads, bounded; the
    // other waves wait at the workgroup barrier that the polling wave joins behind its match, and
    // every load of pose_new and dc below is an sc1 load behind that barrier.
    if (threadIdx.x == 0) {
      unsigned spins = 0, v;
      while (((v = __hip_atomic_load((lin_gu32*)G.pub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) | 1u) !=
             (G.want | 1u)) {
        __builtin_amdgcn_s_sleep(2);
        if (++spins > kLinGateSpins) break;
      }
      int verdict = (int)(v & 1u);
      if ((v | 1u) != (G.want | 1u)) {  // timed out: reported as the reducers' timeout is
        verdict = 1;
        // (every workgroup of the launch that finds the word clear ORs the same tag in)
        const unsigned prior = __hip_atomic_load((lin_gu32*)G.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_or((lin_gu32*)G.status, (unsigned)G.timeout_flag | (prior ? 0u : (unsigned)G.iter_tag),
                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      *G.s_gate = verdict;
    }
    lds_sync_wave();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (__builtin_amdgcn_readfirstlane(*(volatile lin_lds_int*)G.s_gate)) return;  // failed, or never published: state frozen
#if VO_BA_STAMPS
    if (G.stamps && threadIdx.x == 0) G.stamps[2] = __builtin_amdgcn_s_memrealtime();
#endif
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int e = tid + 64 * k;
      vpn[k] = ld_sc1_f64(A.pose_new + 12l * i_acam[k] + e % 12);
      vdc[k] = ld_sc1_f64(A.dc + 6l * i_wcam[k] + e % 6);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int e = tid + 64 * k;
      if (e < 12 * na) (&S.pose_n[0][0])[e] = vpn[k];
      if (e < 6 * ncams) dcw[e] = vdc[k];
    }
  }
  st.count(kPhSlots, nslots);
  st.count(kPhCams, ncams);
  st.count(kPhObs, nob);
  st.count(kPhTe, nte);
  st.count(kPhPts, npt);
  st.count(kPhPairs, h2.y - h2.x);
  double cost = 0.0;
  lds_sync_wave();
  st.mark(kPhLoad);

  if (MODE & kBacksub) {
    // the pending step at its linearisation point: r + Jc dc and Jp per observation, then
    // dp = -V^-1 sum Jp^T (r + Jc dc) per landmark (chunk_backsub)
    if (tid < nob) {
      const int lc = S.img.obs_lcam[tid];
      obs_lin_w<false, true, kRob, kWt>(S, A, &pose_o[12 * S.img.acam[tid]], tid, lc >= 0 ? &dcw[6 * lc] : nullptr, cost,
                                        sw);
    }
    lds_sync_wave();
    if (tid < npt) {
      double l[6], h[3];
      if (point_block_w(S, A.lambda, tid, l, h)) {
        const double x2 = -h[2] * l[5];
        const double x1 = (-h[1] - l[4] * x2) * l[2];
        const double x0 = (-h[0] - l[1] * x1 - l[3] * x2) * l[0];
        S.X[tid][0] += x0;
        S.X[tid][1] += x1;
        S.X[tid][2] += x2;
        A.points[3l * (p0 + tid)] = S.X[tid][0];
        A.points[3l * (p0 + tid) + 1] = S.X[tid][1];
        A.points[3l * (p0 + tid) + 2] = S.X[tid][2];
      }
    }
    lds_sync_wave();
    st.mark(kPhBacksub);
  }

  // residuals and Jacobians at the current linearisation point (cost at the updated state)
  if (tid < nob)
    obs_lin_w<(MODE & kAccum) != 0, false, kRob, kWt>(S, A, S.pose_n[S.img.acam[tid]], tid, nullptr, cost, sw);
  if (MODE & kAccum) {
    lds_sync_wave();
    st.mark(kPhLinObs);
    // per landmark: V (+lambda), its pivot-tested Cholesky and h = L^-1 g
    if (tid < npt) {
      double l[6], h[3];
      const bool ok = point_block_w(S, A.lambda, tid, l, h);
      S.valid[tid] = ok;
#pragma unroll
      for (int e = 0; e < 6; ++e) S.L[tid][e] = l[e];
      S.h[tid][0] = ok ? h[0] : 0.0;
      S.h[tid][1] = ok ? h[1] : 0.0;
      S.h[tid][2] = ok ? h[2] : 0.0;
    }
    lds_sync_wave();
    st.mark(kPhReduce);
    // per track entry: W = Jc^T Jp, gc = Jc^T r over its observations, then Z = W L^-T and
    // bt = -gc + Z h (zero, and the observations' Jc zeroed, for a frozen landmark or a
    // fixed camera); Z | bt overwrite the Jp | r every lane has read
    {
      double W[18], g[6];
#pragma unroll
      for (int e = 0; e < 18; ++e) W[e] = 0.0;
#pragma unroll
      for (int e = 0; e < 6; ++e) g[e] = 0.0;
      const int t = min(tid, max(nte - 1, 0));
      const bool live = tid < nte;
      const int oa = S.img.te_obs[t], ob = live ? S.img.te_obs[t + 1] : oa;
      for (int o = oa; o < ob; ++o) {
        double jj[12];
        jc_load(S, o, jj);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const double rk = S.zb[kZbR + 2 * o + k];
          const double q0 = S.zb[6 * o + 3 * k], q1 = S.zb[6 * o + 3 * k + 1], q2 = S.zb[6 * o + 3 * k + 2];
#pragma unroll
          for (int a = 0; a < 6; ++a) {
            const double jc = jj[6 * k + a];
            W[3 * a] += jc * q0;
            W[3 * a + 1] += jc * q1;
            W[3 * a + 2] += jc * q2;
            g[a] += jc * rk;
          }
        }
      }
      const int p = S.img.te_pt[t];
      const bool use = live && S.valid[p] && S.img.te_lcam[t] >= 0;
      const double i00 = S.L[p][0], l10 = S.L[p][1], i11 = S.L[p][2];
      const double l20 = S.L[p][3], l21 = S.L[p][4], i22 = S.L[p][5];
      const double hh0 = S.h[p][0], hh1 = S.h[p][1], hh2 = S.h[p][2];
      double bt[6];
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        const double z0 = W[3 * a] * i00;
        const double z1 = (W[3 * a + 1] - l10 * z0) * i11;
        const double z2 = (W[3 * a + 2] - l20 * z0 - l21 * z1) * i22;
        W[3 * a] = use ? z0 : 0.0;
        W[3 * a + 1] = use ? z1 : 0.0;
        W[3 * a + 2] = use ? z2 : 0.0;
        bt[a] = use ? -g[a] + (z0 * hh0 + z1 * hh1 + z2 * hh2) : 0.0;
      }
      if (live && !use)  // frozen landmark: its observations leave U too
        for (int o = oa; o < ob; ++o)
#pragma unroll
          for (int e = 0; e < 10; ++e) S.Jc[o][e] = 0.0;
      lds_sync_wave();  // every lane has read its Jp | r
      if (live) {
        double2* zr = reinterpret_cast<double2*>(&S.zb[kZbStride * t]);
#pragma unroll
        for (int e = 0; e < 9; ++e) zr[e] = make_double2(W[2 * e], W[2 * e + 1]);
        double2* br = reinterpret_cast<double2*>(S.bt[t]);
#pragma unroll
        for (int e = 0; e < 3; ++e) br[e] = make_double2(bt[2 * e], bt[2 * e + 1]);
      }
    }
    lds_sync_wave();
    st.mark(kPhElim);
    prio_drop();

    // Schur items: lane j sums active slot j's whole block (copies of a heavy slot balance
    // the lanes, each its own slab row); then the rhs by camera-row lanes
    {
      const int nas = h3.z;
      for (int j = tid; j - tid < nas; j += kLinLanesWave)
        schur_block<kGroup>(S, A, min(j, nas - 1), j < nas, st);
      lds_sync_wave();  // the copies' blocks and the diagonal items' b partials
      for (int j = tid; j - tid < nas; j += kLinLanesWave) copy_rows<kGroup>(S, A, min(j, nas - 1), j < nas);
      rhs_rows<kGroup>(S, A, h3.w, tid);
      if (kGroup) {  // where the combine finds this chunk's blocks (nas <= kWaveItems < 64 lanes)
        if (tid < nas && S.img.acopy[tid] == 0) S.srow[S.img.aslot[tid]] = (uint8_t)tid;
        if (tid < h3.w) S.crow[S.img.acid[tid]] = 1;
      }
    }
    st.mark(kPhWrite);  // stamped builds: the rhs (with the final write below)
  }  // kAccum
  // chunk cost: a fixed xor butterfly over the wave (deterministic)
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) cost += __shfl_xor(cost, m, 64);
  if (!kGroup) {
    if (tid == 0) A.slab_cost[seg] = cost;
  } else {
    if (tid == 0) S.wcost = cost;
    // The combine: segment slot s' block and window camera c's rhs, the chunks' parts summed in
    // chunk order (only the chunks that have it), by 16-byte pieces: two neighbouring entries of
    // one slab row, each with its own scalar sum.  The waves of the first kCombWaves chunks do
    // it.  A segment of more chunks has two waves on some SIMDs, and those finish thousands of
    // cycles after the others: the combining waves meet early at the arrival word and sum their
    // pieces over their own chunks in registers while the late waves still run; after the
    // barrier only the late chunks' parts and the stores are left.
    const int t = (int)threadIdx.x;
    const int nps = nslots * 18, npb = ncams * 3;
    double2 accS[kCombS], accB[kCombB];
    bool anyS[kCombS], anyB[kCombB];
    double2 *dstS[kCombS], *dstB[kCombB];
    auto comb = [&](auto w0c, auto w1c) __attribute__((always_inline)) {
      constexpr int W0 = decltype(w0c)::value, W1 = decltype(w1c)::value;
#pragma unroll
      for (int k = 0; k < kCombS; ++k) {
        const int p = min(t + 64 * kCombWaves * k, max(nps - 1, 0));
        const int s = p / 18, i = 2 * (p - 18 * s);
        if constexpr (W0 == 0) {
          accS[k] = make_double2(0.0, 0.0);
          anyS[k] = false;
          dstS[k] = reinterpret_cast<double2*>(A.slab + 36l * S.spos[s] + i);
        }
#pragma unroll
        for (int w = W0; w < W1; ++w) {
          const int r = Sw[w].srow[s];
          const double2 v = *reinterpret_cast<const double2*>(&Sw[w].Jc[0][0] + 36 * (r == 0xFF ? 0 : r) + i);
          accS[k].x = r == 0xFF ? accS[k].x : anyS[k] ? accS[k].x + v.x : v.x;
          accS[k].y = r == 0xFF ? accS[k].y : anyS[k] ? accS[k].y + v.y : v.y;
          anyS[k] = anyS[k] || r != 0xFF;
        }
      }
#pragma unroll
      for (int k = 0; k < kCombB; ++k) {
        const int p = min(t + 64 * kCombWaves * k, max(npb - 1, 0));
        const int c = p / 3, i = 2 * (p - 3 * c);
        if constexpr (W0 == 0) {
          accB[k] = make_double2(0.0, 0.0);
          anyB[k] = false;
          dstB[k] = reinterpret_cast<double2*>(A.slab_b + 6l * S.cpos[c] + i);
        }
#pragma unroll
        for (int w = W0; w < W1; ++w) {
          const bool on = Sw[w].crow[c] != 0;
          const double2 v = *reinterpret_cast<const double2*>(&Sw[w].pose_n[0][0] + 6 * c + i);
          accB[k].x = !on ? accB[k].x : anyB[k] ? accB[k].x + v.x : v.x;
          accB[k].y = !on ? accB[k].y : anyB[k] ? accB[k].y + v.y : v.y;
          anyB[k] = anyB[k] || on;
        }
      }
    };
    using std::integral_constant;
    if constexpr (kEarly) {
      if (wv < kCombWaves) {
        lds_sync_wave();  // this wave's blocks, b sums, maps and cost are in LDS
        if (tid == 0) __hip_atomic_fetch_add(&s_arrive, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        // waves of one resident workgroup, all of which arrive (the status test above is uniform)
        while (__builtin_amdgcn_readfirstlane(
                   __hip_atomic_load(&s_arrive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) < kCombWaves)
          __builtin_amdgcn_s_sleep(4);
        asm volatile("" ::: "memory");
        comb(integral_constant<int, 0>{}, integral_constant<int, kCombWaves>{});
      }
    }
    __syncthreads();  // every wave's blocks, b sums, maps and cost
    if ((MODE & kAccum) && wv < kCombWaves) {
      comb(integral_constant<int, kEarly ? kCombWaves : 0>{}, integral_constant<int, NW>{});
#pragma unroll
      for (int k = 0; k < kCombS; ++k)
        if (t + 64 * kCombWaves * k < nps) slab_store(dstS[k], accS[k]);
#pragma unroll
      for (int k = 0; k < kCombB; ++k)
        if (t + 64 * kCombWaves * k < npb) slab_store(dstB[k], accB[k]);
    }
    if (t == 0) {
      double c = 0.0;
#pragma unroll
      for (int w = 0; w < NW; ++w) c += Sw[w].wcost;
      A.slab_cost[seg] = c;
    }
  }
  st.mark(kPhWrite);
  st.flush(A.stamps);
#if VO_BA_STAMPS
  if constexpr (kGated)
    if (G.stamps && threadIdx.x == 0) G.stamps[3] = __builtin_amdgcn_s_memrealtime();
#endif
}

}  // namespace

}  // namespace vo
