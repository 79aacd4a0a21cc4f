// Projection-gated descriptor matcher (vo_match_gated, include/vo_hip.h): search by projection.
//
// Query rows (landmarks) are matched against train rows (the frame's keypoints), each query only
// among the keypoints inside a circle around its predicted pixel position.  Build-defined: the
// reference has no such step.  Semantics (the header states the contract):
//   gate      float32 dx, dy; (double)dx*dx + (double)dy*dy <= (double)r*r; a query with a
//             non-finite prediction or !(r >= 0) and a keypoint with a non-finite coordinate
//             have no candidates;
//   distance  the float path's: the k-ordered fp32 chain acc = fmaf(a_k - b_k, a_k - b_k, acc),
//             sqrtf correctly rounded (match.hip; exact for SIFT integers with dim <= 256);
//   select    the two smallest keys (dist, j) among the candidates with dist < FLT_MAX, then
//             max_dist, then the ratio test (vacuous for a lone candidate);
//   unique    per train row the kept pair with the smallest key (dist1, i).
//
// Layout.  The keypoints are binned into a uniform cell grid (count, scan, fill: three small
// launches; integer atomics, and the order inside a cell cannot change a result because the
// keys are a total order).  Cells are kCell pixels wide (doubled until the hinted image is at
// most kMaxCells cells per side); keypoints outside the hinted extent are clamped into the
// border cells, and a query's cell range is clamped by the same monotone function, so the
// binning only prunes: every pair inside the cell range takes the exact gate above.  The cells
// of one grid row are contiguous in the item list, so a query walks one item range per row.
// Search: a 16-lane group per query (four queries per wave, 16 per workgroup); the lanes stride
// over the items, each lane running the serial chain of its own candidate against the query row
// (every lane of a group reads the same query address: one broadcast request), keeping a top-2
// of 64-bit keys (dist bits << 32 | j); the groups merge by xor shuffles below 16.  Lane 0
// applies the keep rule and, under VO_MATCH_GATE_UNIQUE, claims the train row with a 64-bit
// atomicMax of ~(dist bits << 32 | i) (non-negative float bits order as the floats; the
// complement lets one memset to zero clear the claims together with the cell counts); a second
// small launch drops the pairs that lost their row.  compact_pairs (match.hip) finishes.
// A very large radius stays correct (the range is the whole grid) and is not meant to be fast.
// Profiler ids: the clears and the grid build count under match_pack (3), search and filter under
// match_f32 (5).
//
// Segment-gated matcher (vo_match_segment): the same grid, claims, filter and compaction; the gate
// is a capsule, dist(keypoint, segment a_i b_i) <= r_i, evaluated exactly as the header states
// (float32 differences widened to double, every two-term sum rounded once, no division; a == b is
// the circular gate above to the bit).  The walk is per grid row: a candidate lies within R of some
// point p of the segment (R = r plus a margin for the float32 differences), so a keypoint of row cy
// has p.y inside the row's y band widened by R, and its x within R of that sub-segment's x extent.
// Row 0 and the last row hold every keypoint clamped into them, so their bands are unbounded on
// the outer side; the column range is clamped by cell_index like the circular gate's.  A row whose
// widened band the segment does not reach is skipped.  R not finite (r = +inf, overflowing
// differences): the whole grid.  The 16 lanes of a query take 16 rows at a time, one each, and
// then stride over the rows' item ranges laid end to end, so a long thin capsule costs a few
// trips and not one dependent load chain per row.
#include <algorithm>
#include <cfloat>
#include <vector>

#include "vo_ctx.h"

namespace vo {
namespace {

constexpr int kCell = 16;        // pixels per cell side before doubling
constexpr int kMaxCells = 256;   // cells per side at most
constexpr int kGroup = 16;       // lanes per query
constexpr int kSearchThreads = 256;
constexpr int kScanThreads = 1024;

struct Grid {
  int gw, gh;
  double inv_cell;  // 1 / cell side, a power of two
};

Grid grid_shape(int width, int height) {
  const int64_t w = width > 0 ? width : 1024, h = height > 0 ? height : 1024;
  int64_t cell = kCell;
  while ((w + cell - 1) / cell > kMaxCells || (h + cell - 1) / cell > kMaxCells) cell *= 2;
  Grid g;
  g.gw = (int)std::max<int64_t>(1, (w + cell - 1) / cell);
  g.gh = (int)std::max<int64_t>(1, (h + cell - 1) / cell);
  g.inv_cell = 1.0 / (double)cell;
  return g;
}

// Monotone in v: floor, then the clamp into [0, n - 1] (-inf and +inf land in the border cells).
__device__ __forceinline__ int cell_index(double v, double inv_cell, int n) {
  return (int)fmin(fmax(floor(v * inv_cell), 0.0), (double)(n - 1));
}

__device__ __forceinline__ bool finite2(float x, float y) { return isfinite(x) && isfinite(y); }

// Correctly rounded sqrtf, as match.hip's: the f64 sqrt is correctly rounded and 53 >= 2*24 + 2.
__device__ __forceinline__ float sqrtf_rn(float x) { return (float)sqrt((double)x); }

__device__ __forceinline__ uint64_t key64(uint32_t d, uint32_t j) { return ((uint64_t)d << 32) | j; }

// top-2 of the union of two ascending pairs (match.hip's merge2)
__device__ __forceinline__ void merge2(uint64_t& a1, uint64_t& a2, uint64_t b1, uint64_t b2) {
  const uint64_t lo = a1 < b1 ? a1 : b1;
  const uint64_t hi = a1 < b1 ? b1 : a1;
  const uint64_t m = a2 < b2 ? a2 : b2;
  a1 = lo;
  a2 = hi < m ? hi : m;
}

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int m) {
  const uint32_t lo = __shfl_xor((uint32_t)v, m, 64);
  const uint32_t hi = __shfl_xor((uint32_t)(v >> 32), m, 64);
  return ((uint64_t)hi << 32) | lo;
}

// ---- the cell grid: count, scan, fill ----------------------------------------
__global__ __launch_bounds__(256) void gate_count_kernel(const float* __restrict__ kp1, int n1, Grid g,
                                                         int32_t* __restrict__ count) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n1) return;
  const float x = kp1[2 * (long)j], y = kp1[2 * (long)j + 1];
  if (!finite2(x, y)) return;  // never a candidate: in no cell
  atomicAdd(&count[cell_index(y, g.inv_cell, g.gh) * g.gw + cell_index(x, g.inv_cell, g.gw)], 1);
}

// One workgroup: start[c] = the exclusive prefix sum of count (ncell + 1 entries), cursor = start.
__global__ __launch_bounds__(kScanThreads) void gate_scan_kernel(const int32_t* __restrict__ count, int ncell,
                                                                 int32_t* __restrict__ start,
                                                                 int32_t* __restrict__ cursor) {
  __shared__ int part[kScanThreads];
  const int t = threadIdx.x;
  const int per = (ncell + kScanThreads - 1) / kScanThreads;
  const int c0 = min(t * per, ncell), c1 = min(c0 + per, ncell);
  int s = 0;
  for (int c = c0; c < c1; ++c) s += count[c];
  part[t] = s;
  __syncthreads();
  for (int d = 1; d < kScanThreads; d <<= 1) {  // inclusive scan of the per-thread sums
    const int v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - s;
  for (int c = c0; c < c1; ++c) {
    start[c] = run;
    cursor[c] = run;
    run += count[c];
  }
  if (t == kScanThreads - 1) start[ncell] = part[t];
}

__global__ __launch_bounds__(256) void gate_fill_kernel(const float* __restrict__ kp1, int n1, Grid g,
                                                        int32_t* __restrict__ cursor, int32_t* __restrict__ items) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n1) return;
  const float x = kp1[2 * (long)j], y = kp1[2 * (long)j + 1];
  if (!finite2(x, y)) return;
  // below n1: the cursors start at the prefix sums of gate_count_kernel's counts of the same cells
  const int pos = atomicAdd(&cursor[cell_index(y, g.inv_cell, g.gh) * g.gw + cell_index(x, g.inv_cell, g.gw)], 1);
  items[pos] = j;
}

// ---- the gated search ----------------------------------------------------------
struct SearchArgs {
  const float* des0;
  const float* des1;
  const float* pred;  // (n0, 2) circular gate; (n0, 4) a, b for the segment gate
  const float* radius;
  const float* kp1;
  const int32_t* start;
  const int32_t* items;
  unsigned long long* owner;  // (n1) ~ the smallest (dist bits << 32 | i) claiming each train row, 0 = unclaimed;
                              // null = not unique
  int32_t* best;
  float* dist;
  Grid g;
  float radius0, max_dist;  // max_dist: the caller's, rounded to float
  double ratio;
  int n0, dim;
  int use_max;  // the caller's max_dist != 0
};

// The k-ordered chain of one pair.  V4: dim % 4 == 0 and both row sets 16-byte aligned.
template <bool V4>
__device__ __forceinline__ float chain_d2(const float* __restrict__ a, const float* __restrict__ b, int dim) {
  float acc = 0.0f;
  if constexpr (V4) {
    const float4* a4 = reinterpret_cast<const float4*>(a);
    const float4* b4 = reinterpret_cast<const float4*>(b);
#pragma unroll 8
    for (int k = 0; k < dim / 4; ++k) {
      const float4 p = a4[k], q = b4[k];
      const float d0 = p.x - q.x, d1 = p.y - q.y, d2 = p.z - q.z, d3 = p.w - q.w;
      acc = __builtin_fmaf(d0, d0, acc);
      acc = __builtin_fmaf(d1, d1, acc);
      acc = __builtin_fmaf(d2, d2, acc);
      acc = __builtin_fmaf(d3, d3, acc);
    }
  } else {
#pragma unroll 8
    for (int k = 0; k < dim; ++k) {
      const float d = a[k] - b[k];
      acc = __builtin_fmaf(d, d, acc);
    }
  }
  return acc;
}

// The group's top-2, the keep rule, and the claim of the train row (every lane of the wave calls it).
__device__ __forceinline__ void keep_and_claim(const SearchArgs& p, int i, int gl, uint64_t k1, uint64_t k2) {
#pragma unroll
  for (int m = 1; m < kGroup; m <<= 1) merge2(k1, k2, shfl_xor64(k1, m), shfl_xor64(k2, m));
  if (gl != 0 || i >= p.n0) return;
  int j1 = -1;
  float s1 = 0.0f;
  if (k1 != ~0ull) {
    s1 = __uint_as_float((uint32_t)(k1 >> 32));
    const bool near = !p.use_max || s1 <= p.max_dist;
    const bool distinct = k2 == ~0ull || (double)s1 < p.ratio * (double)__uint_as_float((uint32_t)(k2 >> 32));
    if (near && distinct) j1 = (int)(uint32_t)k1;
  }
  p.best[i] = j1;
  p.dist[i] = s1;
  if (p.owner && j1 >= 0) atomicMax(&p.owner[j1], (unsigned long long)~key64(__float_as_uint(s1), (uint32_t)i));
}

template <bool V4>
__global__ __launch_bounds__(kSearchThreads) void gate_search_kernel(SearchArgs p) {
  const int i = blockIdx.x * (kSearchThreads / kGroup) + (threadIdx.x / kGroup);
  const int gl = threadIdx.x & (kGroup - 1);
  float px = 0.0f, py = 0.0f, r = -1.0f;
  if (i < p.n0) {
    px = p.pred[2 * (long)i];
    py = p.pred[2 * (long)i + 1];
    r = p.radius ? p.radius[i] : p.radius0;
  }
  // every lane stays in the flow to the shuffles below; an inactive query walks no cell
  const bool active = i < p.n0 && finite2(px, py) && r >= 0.0f;
  uint64_t k1 = ~0ull, k2 = ~0ull;
  if (active) {
    // A candidate has |fl(kx - px)| <= r (1 + 2^-53), so kx >= px - r (1 + 2^-22): the margin
    // below covers the float subtraction's rounding, and cell_index is monotone, so no candidate
    // lies outside the range (r = +inf gives the whole grid).
    const double rr = (double)r * (1.0 + 1e-6);
    const int cx0 = cell_index((double)px - rr, p.g.inv_cell, p.g.gw);
    const int cx1 = cell_index((double)px + rr, p.g.inv_cell, p.g.gw);
    const int cy0 = cell_index((double)py - rr, p.g.inv_cell, p.g.gh);
    const int cy1 = cell_index((double)py + rr, p.g.inv_cell, p.g.gh);
    const double r2 = (double)r * (double)r;
    const float* a = p.des0 + (long)i * p.dim;
    for (int cy = cy0; cy <= cy1; ++cy) {
      const int t0 = p.start[cy * p.g.gw + cx0], t1 = p.start[cy * p.g.gw + cx1 + 1];
      for (int t = t0 + gl; t < t1; t += kGroup) {
        const int j = p.items[t];
        const float dx = p.kp1[2 * (long)j] - px, dy = p.kp1[2 * (long)j + 1] - py;
        if ((double)dx * (double)dx + (double)dy * (double)dy <= r2) {
          const float d = sqrtf_rn(chain_d2<V4>(a, p.des1 + (long)j * p.dim, p.dim));
          if (d < FLT_MAX) merge2(k1, k2, key64(__float_as_uint(d), (uint32_t)j), ~0ull);
        }
      }
    }
  }
  keep_and_claim(p, i, gl, k1, k2);
}

// ---- the segment-gated search ---------------------------------------------------
// The capsule gate of the header, to the letter: float32 differences widened to double, products
// of two widened floats exact, each two-term sum one rounding (the explicit fma rounds the exact
// sum once, as the plain form does), the tests in this order.
struct SegQuery {
  float ax, ay, bx, by;
  double dx, dy, dd, r2;
};

__device__ __forceinline__ bool capsule_gate(const SegQuery& q, float kx, float ky) {
  const double vx = (double)(kx - q.ax), vy = (double)(ky - q.ay);
  const double s = fma(vx, q.dx, vy * q.dy);
  if (s <= 0.0) return fma(vx, vx, vy * vy) <= q.r2;
  if (s >= q.dd) {
    const double wx = (double)(kx - q.bx), wy = (double)(ky - q.by);
    return fma(wx, wx, wy * wy) <= q.r2;
  }
  const double cr = fma(vx, q.dy, -(vy * q.dx));
  return cr * cr <= q.r2 * q.dd;
}

template <bool V4>
__global__ __launch_bounds__(kSearchThreads) void segment_search_kernel(SearchArgs p) {
  const int i = blockIdx.x * (kSearchThreads / kGroup) + (threadIdx.x / kGroup);
  const int gl = threadIdx.x & (kGroup - 1);
  SegQuery q{};
  float r = -1.0f;
  if (i < p.n0) {
    q.ax = p.pred[4 * (long)i];
    q.ay = p.pred[4 * (long)i + 1];
    q.bx = p.pred[4 * (long)i + 2];
    q.by = p.pred[4 * (long)i + 3];
    r = p.radius ? p.radius[i] : p.radius0;
  }
  const bool active = i < p.n0 && finite2(q.ax, q.ay) && finite2(q.bx, q.by) && r >= 0.0f;
  uint64_t k1 = ~0ull, k2 = ~0ull;
  if (active) {
    q.dx = (double)(q.bx - q.ax);
    q.dy = (double)(q.by - q.ay);
    q.dd = fma(q.dx, q.dx, q.dy * q.dy);
    q.r2 = (double)r * (double)r;
    // The walk works on the exact segment (the float coordinates in double).  An accepted keypoint
    // is within r (1 + 2^-21) + 2^-21 (L + r) of it, L = |b - a|_1: each float32 difference is off
    // by at most 2^-24 of itself, so the cross product by at most 2^-22 |v| |d| and a misjudged
    // end by as much along the segment, with |v| <= |d| + dist.  R takes 1e-5 of both instead.
    const double ax = q.ax, ay = q.ay, bx = q.bx, by = q.by;
    const double ex = bx - ax, ey = by - ay;  // exact or, past 2^53 apart, as good as
    const double R = (double)r + 1e-5 * ((double)r + fabs(ex) + fabs(ey));
    const bool whole = !(R < 1e30);  // +inf or NaN: no pruning
    const double cell = 1.0 / p.g.inv_cell;
    const int gw = p.g.gw, gh = p.g.gh;
    const int cy0 = whole ? 0 : cell_index(fmin(ay, by) - R, p.g.inv_cell, gh);
    const int cy1 = whole ? gh - 1 : cell_index(fmax(ay, by) + R, p.g.inv_cell, gh);
    const float* a = p.des0 + (long)i * p.dim;
    // A long segment crosses many rows with a few items in each, and a loop over the rows would
    // pay a dependent start -> items -> keypoint load chain per row.  So each lane of the group
    // takes one row (16 rows per trip), the lanes' item ranges are laid end to end by a prefix
    // sum, and the group strides over that one list.  `active`, the row bounds and `total` are
    // the same in all 16 lanes, so the width-16 shuffles only ever read lanes that run with them.
    for (int base = cy0; base <= cy1; base += kGroup) {
      const int cy = base + gl;
      int t_lo = 0, cnt = 0;  // this lane's row: items [t_lo, t_lo + cnt)
      if (cy <= cy1) {
        int cx0 = 0, cx1 = gw - 1;
        bool reach = true;
        if (!whole) {
          // the keypoints of this row have y in [lo, hi): unbounded outwards in the border rows
          const double lo = cy == 0 ? -INFINITY : (double)cy * cell;
          const double hi = cy == gh - 1 ? INFINITY : (double)(cy + 1) * cell;
          double t0 = 0.0, t1 = 1.0;  // the part of the segment with y in [lo - R, hi + R]
          if (ey != 0.0) {
            const double ta = ((lo - R) - ay) / ey, tb = ((hi + R) - ay) / ey;
            t0 = fmax(fmin(ta, tb), 0.0);
            t1 = fmin(fmax(ta, tb), 1.0);
          }
          reach = t0 <= t1;  // else the capsule does not touch this row
          const double xa = ax + t0 * ex, xb = ax + t1 * ex;
          cx0 = cell_index(fmin(xa, xb) - R, p.g.inv_cell, gw);
          cx1 = cell_index(fmax(xa, xb) + R, p.g.inv_cell, gw);
        }
        if (reach) {
          t_lo = p.start[cy * gw + cx0];
          cnt = p.start[cy * gw + cx1 + 1] - t_lo;
        }
      }
      int end = cnt;  // inclusive prefix sum over the group's lanes
#pragma unroll
      for (int d = 1; d < kGroup; d <<= 1) {
        const int v = __shfl_up(end, d, kGroup);
        if (gl >= d) end += v;
      }
      const int total = __shfl(end, kGroup - 1, kGroup);
      const int first = end - cnt;
      for (int b = 0; b < total; b += kGroup) {
        const int idx = b + gl;
        int t = -1;  // the idx-th item of the rows laid end to end
#pragma unroll
        for (int m = 0; m < kGroup; ++m) {
          const int f = __shfl(first, m, kGroup), c = __shfl(cnt, m, kGroup), tl = __shfl(t_lo, m, kGroup);
          if (idx >= f && idx < f + c) t = tl + (idx - f);
        }
        if (t >= 0) {
          const int j = p.items[t];
          if (capsule_gate(q, p.kp1[2 * (long)j], p.kp1[2 * (long)j + 1])) {
            const float d = sqrtf_rn(chain_d2<V4>(a, p.des1 + (long)j * p.dim, p.dim));
            if (d < FLT_MAX) merge2(k1, k2, key64(__float_as_uint(d), (uint32_t)j), ~0ull);
          }
        }
      }
    }
  }
  keep_and_claim(p, i, gl, k1, k2);
}

// VO_MATCH_GATE_UNIQUE: a kept pair survives iff its query holds the train row's smallest key.
__global__ __launch_bounds__(256) void gate_unique_kernel(int32_t* __restrict__ best,
                                                          const unsigned long long* __restrict__ owner, int n0) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n0) return;
  const int j = best[i];
  if (j >= 0 && (uint32_t)~owner[j] != (uint32_t)i) best[i] = -1;
}

size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

// gate_run's device arrays: descriptors, gate and keypoints in, best (n0) and dist (n0) out.
struct GateArgs {
  const float* des0;    // (n0, dim)
  const float* des1;    // (n1, dim)
  const float* pred;    // (n0, 2); with segment (n0, 4): ax, ay, bx, by
  const float* radius;  // (n0) or null: radius0
  const float* kp1;     // (n1, 2)
  float radius0;
  int n0, n1, dim, width, height;
  double ratio, max_dist;
  bool unique;
  bool segment;         // the capsule gate of vo_match_segment around pred's segments
  int32_t* best;        // (n0) kept train row or -1
  float* dist;          // (n0) dist1 of the kept pair (unspecified where best is -1)
};

}  // namespace

// scratch: start (ncell + 1) | cursor (ncell) | items (n1) | owner (n1 x u64) | count (ncell): the
// last two are cleared by one memset
static size_t gate_scratch_bytes(int n1, int width, int height) {
  const Grid g = grid_shape(width, height);
  const size_t ncell = (size_t)g.gw * g.gh;
  return align16((ncell + 1) * 4) + align16(ncell * 4) + align16((size_t)n1 * 4) + (size_t)n1 * 8 + ncell * 4 + 16;
}

static void gate_run(vo_ctx* ctx, const GateArgs& a, void* scratch) {
  if (a.n0 == 0) return;
  hipStream_t st = ctx->stream;
  const Grid g = grid_shape(a.width, a.height);
  const size_t ncell = (size_t)g.gw * g.gh;
  char* base = static_cast<char*>(scratch);
  int32_t* start = reinterpret_cast<int32_t*>(base);
  int32_t* cursor = reinterpret_cast<int32_t*>(base + align16((ncell + 1) * 4));
  int32_t* items = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(cursor) + align16(ncell * 4));
  unsigned long long* owner =
      reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(items) + align16((size_t)a.n1 * 4));
  int32_t* count = reinterpret_cast<int32_t*>(owner + a.n1);
  const bool unique = a.unique && a.n1 > 0;

  ctx->prof.begin(st, kKMatchPack);
  // the cell counts and, for the unique pass, the train rows' claims right before them
  if (unique) VO_HIP_CHECK(hipMemsetAsync(owner, 0, (size_t)a.n1 * 8 + ncell * 4, st));
  else VO_HIP_CHECK(hipMemsetAsync(count, 0, ncell * 4, st));
  if (a.n1 > 0)
    hipLaunchKernelGGL(gate_count_kernel, dim3(ceil_div(a.n1, 256)), dim3(256), 0, st, a.kp1, a.n1, g, count);
  hipLaunchKernelGGL(gate_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, count, (int)ncell, start, cursor);
  if (a.n1 > 0)
    hipLaunchKernelGGL(gate_fill_kernel, dim3(ceil_div(a.n1, 256)), dim3(256), 0, st, a.kp1, a.n1, g, cursor, items);
  VO_HIP_CHECK(hipGetLastError());
  ctx->prof.end(st);

  SearchArgs s{};
  s.des0 = a.des0;
  s.des1 = a.des1;
  s.pred = a.pred;
  s.radius = a.radius;
  s.kp1 = a.kp1;
  s.start = start;
  s.items = items;
  s.owner = unique ? owner : nullptr;
  s.best = a.best;
  s.dist = a.dist;
  s.g = g;
  s.radius0 = a.radius0;
  s.max_dist = (float)std::min(a.max_dist, (double)FLT_MAX);  // every selected distance is < FLT_MAX
  s.use_max = a.max_dist != 0.0 ? 1 : 0;
  s.ratio = a.ratio;
  s.n0 = a.n0;
  s.dim = a.dim;
  const bool v4 = a.dim % 4 == 0 && (((uintptr_t)a.des0 | (uintptr_t)a.des1) & 15) == 0;
  ctx->prof.begin(st, kKMatchF32);
  const dim3 grid(ceil_div(a.n0, kSearchThreads / kGroup));
  if (a.segment) {
    if (v4) hipLaunchKernelGGL(segment_search_kernel<true>, grid, dim3(kSearchThreads), 0, st, s);
    else hipLaunchKernelGGL(segment_search_kernel<false>, grid, dim3(kSearchThreads), 0, st, s);
  } else {
    if (v4) hipLaunchKernelGGL(gate_search_kernel<true>, grid, dim3(kSearchThreads), 0, st, s);
    else hipLaunchKernelGGL(gate_search_kernel<false>, grid, dim3(kSearchThreads), 0, st, s);
  }
  if (s.owner) hipLaunchKernelGGL(gate_unique_kernel, dim3(ceil_div(a.n0, 256)), dim3(256), 0, st, a.best, owner, a.n0);
  VO_HIP_CHECK(hipGetLastError());
  ctx->prof.end(st);
}

void match_gate_host(vo_ctx* ctx, const float* des0, int n0, const float* des1, int n1, int dim, const GateHostArgs& h,
                     int32_t* out_pairs, float* out_dist, int32_t* out_count) {
  hipStream_t st = ctx->stream;
  MatchWorkspace& ws = ctx->match;
  const size_t qrow = (size_t)h.qcols * 4;  // bytes per query of the gate's array
  // descriptors: des0 | des1 (host train rows), each 16-byte aligned for the float4 loads
  const size_t b0 = align16((size_t)n0 * dim * 4), b1 = (size_t)n1 * dim * 4;
  ws.des.reserve(b0 + (h.dev ? 0 : b1) + 16);
  float* d0 = ws.des.as<float>();
  const float* d1 = des1;
  VO_HIP_CHECK(hipMemcpyAsync(d0, des0, (size_t)n0 * dim * 4, hipMemcpyHostToDevice, st));
  if (!h.dev) {
    float* s1 = reinterpret_cast<float*>(ws.des.as<char>() + b0);
    VO_HIP_CHECK(hipMemcpyAsync(s1, des1, b1, hipMemcpyHostToDevice, st));
    d1 = s1;
  }
  // gate workspace: pred or seg | radius | kp1 (host keypoints) | dist | the grid's scratch
  const size_t bp = align16((size_t)n0 * qrow), br = align16((size_t)n0 * 4), bk = h.dev ? 0 : align16((size_t)n1 * 8);
  ws.gate.reserve(bp + br + bk + br + gate_scratch_bytes(n1, h.width, h.height));
  char* gb = ws.gate.as<char>();
  float* d_pred = reinterpret_cast<float*>(gb);
  float* d_rad = reinterpret_cast<float*>(gb + bp);
  float* d_kp = reinterpret_cast<float*>(gb + bp + br);
  float* d_dist = reinterpret_cast<float*>(gb + bp + br + bk);
  VO_HIP_CHECK(hipMemcpyAsync(d_pred, h.query, (size_t)n0 * qrow, hipMemcpyHostToDevice, st));
  if (h.radius) VO_HIP_CHECK(hipMemcpyAsync(d_rad, h.radius, (size_t)n0 * 4, hipMemcpyHostToDevice, st));
  if (!h.dev) VO_HIP_CHECK(hipMemcpyAsync(d_kp, h.kp1, (size_t)n1 * 8, hipMemcpyHostToDevice, st));
  ws.best.reserve((size_t)n0 * 4);
  GateArgs g{};
  g.des0 = d0;
  g.des1 = d1;
  g.pred = d_pred;
  g.radius = h.radius ? d_rad : nullptr;
  g.kp1 = h.dev ? h.kp1 : d_kp;
  g.radius0 = h.radius0;
  g.n0 = n0;
  g.n1 = n1;
  g.dim = dim;
  g.width = h.width;
  g.height = h.height;
  g.ratio = h.ratio;
  g.max_dist = h.max_dist;
  g.unique = h.unique;
  g.segment = h.qcols == 4;
  g.best = ws.best.as<int32_t>();
  g.dist = d_dist;
  gate_run(ctx, g, gb + bp + br + bk + br);
  ws.pairs.reserve((size_t)n0 * 8 + 16);
  int32_t* d_pairs = ws.pairs.as<int32_t>();
  int32_t* d_count = d_pairs + 2 * (size_t)n0;
  compact_pairs(ctx, g.best, n0, d_pairs, d_count);
  std::vector<float> dist_q(out_dist ? (size_t)n0 : 0);
  VO_HIP_CHECK(hipMemcpyAsync(out_count, d_count, 4, hipMemcpyDeviceToHost, st));
  VO_HIP_CHECK(hipMemcpyAsync(out_pairs, d_pairs, (size_t)n0 * 8, hipMemcpyDeviceToHost, st));
  if (out_dist) VO_HIP_CHECK(hipMemcpyAsync(dist_q.data(), d_dist, (size_t)n0 * 4, hipMemcpyDeviceToHost, st));
  VO_HIP_CHECK(hipStreamSynchronize(st));
  // dist1 per pair: the per-query distances gathered in the pairs' order
  if (out_dist)
    for (int m = 0; m < *out_count; ++m) out_dist[m] = dist_q[out_pairs[2 * (size_t)m]];
}

}  // namespace vo
