// Shi-Tomasi corner detection on gfx950 (vo_good_features, vo_corner_response, vo_corner_select).
//
// The contract is the restatement in tests/corners_ref.py; the per-pixel and
// per-candidate arithmetic is corners_math.h, compiled here without FMA contraction and shared with
// the host build (corners_host_check.cpp).  Every block sum is an int32 and every distance test an
// exact comparison, so the results do not depend on the mapping below.
//   corner_response_kernel<K>  one workgroup of 256 per 64 x 16 tile.  The tile and a halo of K + 1
//                              pixels are staged in LDS as bytes; gx*gx, gx*gy, gy*gy are formed
//                              once per pixel of the tile + K halo in LDS (the gradient field is
//                              read at reflected indices, so a halo pixel outside the image takes
//                              the gradient of its mirror pixel); the block sums are taken
//                              separably, rows then columns; a wave stores 64 consecutive floats
//                              per row; the workgroup's maximum over unmasked pixels goes into the
//                              global maximum with one atomic (on the bits of max(resp, +0)).
//   corner_candidates_kernel   one thread per pixel: interior, mask, threshold, 3 x 3 test; the
//                              64-bit keys are compacted with one counter add per wave.
//   rocprim radix sort of the keys: response descending, ties by pixel index.
//   corner_unpack_kernel       coordinates, row ids and responses of the sorted candidates.
//   The selection is the lexicographically first maximal independent set of the "closer than d"
//   graph in rank order, so it is decided in rounds without changing the result:
//   corner_bin_kernel          candidates and keep-away points into per-cell lists of a grid with
//                              cells of side ceil(d) (doubled while the grid would be too large)
//                              and a one-cell border, so the 3 x 3 cells around a candidate hold
//                              everything within d of it and need no bounds test.
//   corner_keep_kernel         a candidate within d of a keep-away point is rejected at once.
//   corner_round_kernel        one round over all candidates, launched kParallelRounds times when
//                              there are more than kFinishThreads candidates: an undecided
//                              candidate with an accepted neighbour of higher rank is rejected, one
//                              whose such neighbours are all rejected is accepted.  Decisions are
//                              final and only ever read as "undecided" when stale, so any mix of
//                              old and new states gives a correct (possibly later) decision.
//   corner_finish_kernel       one workgroup: rounds on the device until nothing is undecided (the
//                              lowest undecided rank is decided every round, so at most n rounds;
//                              states are read and written with agent-scope atomics and a fence
//                              precedes each barrier), then the accepted candidates compacted in
//                              rank order by a workgroup scan and cut at max_corners.
// Bounds: every global image read goes through reflect() (total for any extent); LDS indices of the
// Sobel taps are proven in DESIGN.md §Corners and clamped besides; candidate cells lie in
// 1..gw x 1..gh of a (gw + 2) x (gh + 2) grid; keep-away points outside the bordered grid are dropped.
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <vector>

#include "corners_math.h"
#include "vo_ctx.h"

#pragma clang fp contract(off)

namespace vo {
namespace {

using namespace cornm;

constexpr int kTileW = 64, kTileH = 16;
constexpr int kFinishThreads = 1024;
constexpr int kParallelRounds = 12;
constexpr int64_t kMaxCells = 1 << 22;
enum : int32_t { kUndecided = 0, kAccepted = 1, kRejected = 2 };
// control words, zeroed before every call
enum { kCtlMax = 0, kCtlCount = 1, kCtlOut = 2, kCtlRounds = 3, kCtlFailed = 4, kCtlEntry = 5, kCtlWords = 32 };
static_assert(kCtlEntry + kParallelRounds <= kCtlWords, "control block");

__device__ inline int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <int K>
__global__ __launch_bounds__(256) void corner_response_kernel(const uint8_t* img, const uint8_t* mask, int h, int w,
                                                              float* resp, uint32_t* ctl) {
  constexpr int H = K + 1;
  constexpr int BW = kTileW + 2 * H, BH = kTileH + 2 * H;  // the byte tile
  constexpr int PW = kTileW + 2 * K, PH = kTileH + 2 * K;  // the product tile
  __shared__ uint8_t s_img[BH * BW];
  __shared__ int32_t s_p[3][PH * PW];
  __shared__ int32_t s_h[3][PH * kTileW];
  __shared__ uint32_t s_max[4];
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  const int tid = threadIdx.x;
  for (int i = tid; i < BH * BW; i += 256) {
    const int by = i / BW, bx = i - by * BW;
    s_img[i] = img[(size_t)reflect(y0 - H + by, h) * w + reflect(x0 - H + bx, w)];
  }
  __syncthreads();
  // products at (X, Y) = tile + K halo, as far as an output pixel of the image needs them
  const int xe = min(x0 + kTileW, w) - 1 + K, ye = min(y0 + kTileH, h) - 1 + K;
  for (int i = tid; i < PH * PW; i += 256) {
    const int py = i / PW, px = i - py * PW;
    const int X = x0 - K + px, Y = y0 - K + py;
    int32_t pxx = 0, pxy = 0, pyy = 0;
    if (X <= xe && Y <= ye) {
      const int rx = reflect(X, w), ry = reflect(Y, h);  // the gradient field at reflected indices
      const int cx[3] = {reflect(rx - 1, w), rx, reflect(rx + 1, w)};
      const int cy[3] = {reflect(ry - 1, h), ry, reflect(ry + 1, h)};
      int v[3][3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int row = clampi(cy[j] - (y0 - H), BH - 1) * BW;
#pragma unroll
        for (int k = 0; k < 3; ++k) v[j][k] = s_img[row + clampi(cx[k] - (x0 - H), BW - 1)];
      }
      int gx, gy;
      sobel(v, gx, gy);
      pxx = gx * gx;
      pxy = gx * gy;
      pyy = gy * gy;
    }
    s_p[0][i] = pxx;
    s_p[1][i] = pxy;
    s_p[2][i] = pyy;
  }
  __syncthreads();
  for (int i = tid; i < PH * kTileW; i += 256) {
    const int py = i / kTileW, tx = i - py * kTileW;
    int32_t a = 0, b = 0, c = 0;
#pragma unroll
    for (int t = 0; t <= 2 * K; ++t) {
      a += s_p[0][py * PW + tx + t];
      b += s_p[1][py * PW + tx + t];
      c += s_p[2][py * PW + tx + t];
    }
    s_h[0][i] = a;
    s_h[1][i] = b;
    s_h[2][i] = c;
  }
  __syncthreads();
  const int tx = tid & 63, x = x0 + tx;
  uint32_t best = 0;
  for (int ty = tid >> 6; ty < kTileH; ty += 4) {
    const int y = y0 + ty;
    int32_t a = 0, b = 0, c = 0;
#pragma unroll
    for (int t = 0; t <= 2 * K; ++t) {
      a += s_h[0][(ty + t) * kTileW + tx];
      b += s_h[1][(ty + t) * kTileW + tx];
      c += s_h[2][(ty + t) * kTileW + tx];
    }
    if (x < w && y < h) {
      const float r = response(a, b, c);
      const size_t p = (size_t)y * w + x;
      resp[p] = r;
      if (!mask || mask[p]) best = max(best, max_domain(r));
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, m, 64));
  if (tx == 0) s_max[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    const uint32_t m = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
    if (m) atomicMax(&ctl[kCtlMax], m);
  }
}

__global__ __launch_bounds__(256) void corner_candidates_kernel(const float* resp, const uint8_t* mask, int h, int w,
                                                                float quality, uint32_t* ctl, uint64_t* keys,
                                                                uint32_t cap) {
  const int lane = threadIdx.x & 63;
  const int x = blockIdx.x * 64 + lane, y = blockIdx.y * 4 + (threadIdx.x >> 6);
  const float rmax = bits_float(ctl[kCtlMax]);
  bool cand = false;
  float r = 0.f;
  size_t p = 0;
  if (rmax > 0.f && x >= 1 && x <= w - 2 && y >= 1 && y <= h - 2) {
    p = (size_t)y * w + x;
    r = resp[p];
    if ((!mask || mask[p]) && above_threshold(r, quality, rmax)) {
      cand = true;
#pragma unroll
      for (int j = -1; j <= 1; ++j) {
#pragma unroll
        for (int i = -1; i <= 1; ++i) cand = cand && r >= resp[p + (ptrdiff_t)j * w + i];
      }
    }
  }
  const uint64_t votes = __ballot(cand);
  if (votes == 0) return;
  const int leader = __ffsll((unsigned long long)votes) - 1;
  uint32_t base = 0;
  if (lane == leader) base = atomicAdd(&ctl[kCtlCount], (uint32_t)__popcll(votes));
  base = (uint32_t)__shfl((int)base, leader, 64);
  if (cand) {
    const uint32_t pos = base + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
    if (pos < cap) keys[pos] = candidate_key(r, (uint32_t)p);
  }
}

struct SelArgs {
  const int32_t *cx, *cy;      // (n) candidates in rank order
  const uint32_t* ids;         // (n) pixel index or caller's row
  const float* rv;             // (n) responses
  int32_t* state;              // (n)
  int32_t *next, *head;        // per-cell lists of candidates
  const float* keep;           // (n_keep, 2)
  int32_t *knext, *khead;      // per-cell lists of keep-away points
  int n, n_keep;
  int ox, oy, side, gw, gh;    // cell of (x, y): ((x - ox) / side + 1, (y - oy) / side + 1) in a (gw + 2) x (gh + 2) grid
  double d2;
  int max_corners;
  uint32_t* ctl;
  float* out_xy;               // (max_out, 2)
  float* out_resp;             // (max_out)
  int32_t* out_id;             // (max_out)
};

__device__ inline int cell_of(const SelArgs& a, int x, int y) {
  return ((y - a.oy) / a.side + 1) * (a.gw + 2) + (x - a.ox) / a.side + 1;
}

__global__ __launch_bounds__(256) void corner_unpack_kernel(const uint64_t* keys, int n, const int32_t* xy, int w,
                                                            int32_t* cx, int32_t* cy, uint32_t* ids, float* rv) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = keys[i];
  const uint32_t id = (uint32_t)key;
  if (xy) {
    cx[i] = xy[2 * (size_t)id];
    cy[i] = xy[2 * (size_t)id + 1];
    rv[i] = 0.f;
  } else {
    cx[i] = (int32_t)(id % (uint32_t)w);
    cy[i] = (int32_t)(id / (uint32_t)w);
    rv[i] = key_response(key);
  }
  ids[i] = id;
}

__global__ __launch_bounds__(256) void corner_bin_kernel(SelArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.n) a.next[i] = atomicExch(&a.head[cell_of(a, a.cx[i], a.cy[i])], i);
  if (i < a.n_keep) {
    const float kx = a.keep[2 * (size_t)i], ky = a.keep[2 * (size_t)i + 1];
    if (finite32(kx) && finite32(ky)) {
      // a point outside the bordered grid is further than one cell side >= d from every candidate
      const double qx = floor(((double)kx - (double)a.ox) / (double)a.side);
      const double qy = floor(((double)ky - (double)a.oy) / (double)a.side);
      if (qx >= -1.0 && qx <= (double)a.gw && qy >= -1.0 && qy <= (double)a.gh)
        a.knext[i] = atomicExch(&a.khead[((int)qy + 1) * (a.gw + 2) + (int)qx + 1], i);
    }
  }
}

__global__ __launch_bounds__(256) void corner_keep_kernel(SelArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const int x = a.cx[i], y = a.cy[i];
  const int c0 = cell_of(a, x, y);
  bool rejected = false;
  for (int dy = -1; dy <= 1 && !rejected; ++dy)
    for (int dx = -1; dx <= 1 && !rejected; ++dx)
      for (int j = a.khead[c0 + dy * (a.gw + 2) + dx]; j >= 0 && !rejected; j = a.knext[j])
        rejected = keep_rejects(x, y, a.keep[2 * (size_t)j], a.keep[2 * (size_t)j + 1], a.d2);
  a.state[i] = rejected ? kRejected : kUndecided;
}

// The verdict on undecided candidate i from the states of its closer-than-d neighbours of higher rank.
template <bool kCoherent>
__device__ inline int32_t decide(const SelArgs& a, int i) {
  const int x = a.cx[i], y = a.cy[i];
  const int c0 = cell_of(a, x, y);
  bool waits = false;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx)
      for (int j = a.head[c0 + dy * (a.gw + 2) + dx]; j >= 0; j = a.next[j]) {
        if (j >= i || !pair_rejects((int64_t)x - a.cx[j], (int64_t)y - a.cy[j], a.d2)) continue;
        const int32_t s = kCoherent ? __hip_atomic_load(&a.state[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                    : a.state[j];
        if (s == kAccepted) return kRejected;
        waits = waits || s == kUndecided;
      }
  return waits ? kUndecided : kAccepted;
}

__global__ __launch_bounds__(256) void corner_round_kernel(SelArgs a, int round) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n || a.state[i] != kUndecided) return;
  atomicAdd(&a.ctl[kCtlEntry + round], 1u);
  const int32_t s = decide<false>(a, i);
  if (s != kUndecided) a.state[i] = s;
}

__global__ __launch_bounds__(kFinishThreads) void corner_finish_kernel(SelArgs a) {
  __shared__ int s_left, s_seen;
  __shared__ int s_wave[kFinishThreads / 64];
  const int tid = threadIdx.x;
  int rounds = 0;
  bool failed = false;
  for (int guard = 0;; ++guard) {
    if (tid == 0) s_left = s_seen = 0;
    __syncthreads();
    int left = 0, seen = 0;
    for (int i = tid; i < a.n; i += kFinishThreads) {
      if (__hip_atomic_load(&a.state[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != kUndecided) continue;
      ++seen;
      const int32_t s = decide<true>(a, i);
      if (s != kUndecided)
        __hip_atomic_store(&a.state[i], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else
        ++left;
    }
    if (seen) atomicAdd(&s_seen, seen);
    if (left) atomicAdd(&s_left, left);
    __threadfence();
    __syncthreads();
    const int total_left = s_left, total_seen = s_seen;
    __syncthreads();
    if (total_seen) ++rounds;
    if (total_left == 0) break;
    if (guard > a.n) {  // cannot happen: every round decides the lowest undecided rank
      failed = true;
      break;
    }
  }
  // the accepted candidates in rank order, cut at max_corners
  const int lane = tid & 63, wave = tid >> 6;
  int base = 0;
  for (int start = 0; start < a.n && base < a.max_corners; start += kFinishThreads) {
    const int i = start + tid;
    const bool acc = i < a.n && __hip_atomic_load(&a.state[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kAccepted;
    const uint64_t votes = __ballot(acc);
    if (lane == 0) s_wave[wave] = __popcll(votes);
    __syncthreads();
    int before = 0, total = 0;
    for (int k = 0; k < kFinishThreads / 64; ++k) {
      const int c = s_wave[k];
      before += k < wave ? c : 0;
      total += c;
    }
    const int pos = base + before + __popcll(votes & ((1ull << lane) - 1ull));
    if (acc && pos < a.max_corners) {
      a.out_xy[2 * (size_t)pos] = (float)a.cx[i];
      a.out_xy[2 * (size_t)pos + 1] = (float)a.cy[i];
      a.out_resp[pos] = a.rv[i];
      a.out_id[pos] = (int32_t)a.ids[i];
    }
    base += total;
    __syncthreads();
  }
  if (tid == 0) {
    a.ctl[kCtlOut] = (uint32_t)min(base, a.max_corners);
    a.ctl[kCtlRounds] = (uint32_t)rounds;
    a.ctl[kCtlFailed] = failed ? 1u : 0u;
  }
}

uint32_t* control(vo_ctx* ctx) {
  CornerWorkspace& ws = ctx->corners;
  ws.ctl.reserve(kCtlWords * 4);
  VO_HIP_CHECK(hipMemsetAsync(ws.ctl.ptr, 0, kCtlWords * 4, ctx->stream));
  return ws.ctl.as<uint32_t>();
}

void launch_response(vo_ctx* ctx, const uint8_t* d_img, const uint8_t* d_mask, int h, int w, int k, float* d_resp,
                     uint32_t* d_ctl) {
  const dim3 grid(ceil_div(w, kTileW), ceil_div(h, kTileH)), block(256);
  if (k == 1)
    hipLaunchKernelGGL(corner_response_kernel<1>, grid, block, 0, ctx->stream, d_img, d_mask, h, w, d_resp, d_ctl);
  else if (k == 2)
    hipLaunchKernelGGL(corner_response_kernel<2>, grid, block, 0, ctx->stream, d_img, d_mask, h, w, d_resp, d_ctl);
  else
    hipLaunchKernelGGL(corner_response_kernel<3>, grid, block, 0, ctx->stream, d_img, d_mask, h, w, d_resp, d_ctl);
  VO_HIP_CHECK(hipGetLastError());
}

// Level 0 of a cached KLT pyramid with this tag and shape, or the image uploaded into scratch.
const uint8_t* device_image(vo_ctx* ctx, const uint8_t* img, uint64_t tag, int h, int w, const char* who) {
  if (tag != 0)
    for (const KltPyramid& c : ctx->klt.cache)
      if (c.valid && c.tag == tag && c.h == h && c.w == w) return c.buf.as<uint8_t>();
  VO_REQUIRE(img, VO_ERR_ARG, "%s: the image is NULL and its tag is not in the pyramid cache", who);
  CornerWorkspace& ws = ctx->corners;
  ws.img.reserve((size_t)h * w);
  VO_HIP_CHECK(hipMemcpyAsync(ws.img.ptr, img, (size_t)h * w, hipMemcpyHostToDevice, ctx->stream));
  return ws.img.as<uint8_t>();
}

// Sorts the n keys in ws.keys (first half) into its second half.
const uint64_t* sort_keys(vo_ctx* ctx, int n, size_t cap) {
  CornerWorkspace& ws = ctx->corners;
  uint64_t* in = ws.keys.as<uint64_t>();
  uint64_t* out = in + cap;
  size_t tmp = 0;
  VO_HIP_CHECK(rocprim::radix_sort_keys(nullptr, tmp, in, out, (size_t)n, 0u, 64u, ctx->stream));
  ws.sort_tmp.reserve(tmp);
  VO_HIP_CHECK(rocprim::radix_sort_keys(ws.sort_tmp.ptr, tmp, in, out, (size_t)n, 0u, 64u, ctx->stream));
  return out;
}

// The selection over n sorted keys (device) -> the number accepted; outputs stay in ws.out.
// Coordinates come from xy rows (d_xy) or from pixel indices of a w-wide image, and lie in
// [lo_x, hi_x] x [lo_y, hi_y].
int select_sorted(vo_ctx* ctx, const uint64_t* d_keys, int n, const int32_t* d_xy, int w, int lo_x, int lo_y, int hi_x,
                  int hi_y, const float* keep, int n_keep, float dist, int max_corners, uint32_t* d_ctl, SelArgs& a) {
  CornerWorkspace& ws = ctx->corners;
  hipStream_t s = ctx->stream;
  const size_t n4 = (size_t)n * 4;
  ws.cand.reserve(6 * n4);
  char* c = ws.cand.as<char>();
  int32_t* cx = reinterpret_cast<int32_t*>(c);
  int32_t* cy = reinterpret_cast<int32_t*>(c + n4);
  uint32_t* ids = reinterpret_cast<uint32_t*>(c + 2 * n4);
  float* rv = reinterpret_cast<float*>(c + 3 * n4);
  a.cx = cx;
  a.cy = cy;
  a.ids = ids;
  a.rv = rv;
  a.state = reinterpret_cast<int32_t*>(c + 4 * n4);
  a.next = reinterpret_cast<int32_t*>(c + 5 * n4);
  a.n = n;
  a.n_keep = dist > 0.f ? n_keep : 0;
  a.d2 = distance2(dist);
  a.max_corners = max_corners;
  a.ctl = d_ctl;
  a.ox = lo_x;
  a.oy = lo_y;
  a.side = cell_side(dist);
  const int64_t ex = (int64_t)hi_x - lo_x, ey = (int64_t)hi_y - lo_y;
  for (;; a.side *= 2) {
    a.gw = (int)(ex / a.side) + 1;
    a.gh = (int)(ey / a.side) + 1;
    if ((int64_t)(a.gw + 2) * (a.gh + 2) <= kMaxCells) break;
  }
  const int max_out = std::min(max_corners, n);
  ws.out.reserve((size_t)max_out * 16);
  a.out_xy = ws.out.as<float>();
  a.out_resp = a.out_xy + 2 * (size_t)max_out;
  a.out_id = reinterpret_cast<int32_t*>(a.out_resp + max_out);

  const int blocks = ceil_div(n, 256);
  hipLaunchKernelGGL(corner_unpack_kernel, dim3(blocks), dim3(256), 0, s, d_keys, n, d_xy, w, cx, cy, ids, rv);
  VO_HIP_CHECK(hipGetLastError());
  if (!(dist > 0.f)) {  // nothing is rejected
    VO_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(a.state), kAccepted, (size_t)n, s));
  } else {
    const size_t cells = (size_t)(a.gw + 2) * (a.gh + 2);
    ws.grid.reserve(2 * cells * 4);
    a.head = ws.grid.as<int32_t>();
    a.khead = a.head + cells;
    VO_HIP_CHECK(hipMemsetAsync(a.head, 0xff, (a.n_keep ? 2 : 1) * cells * 4, s));
    if (a.n_keep) {
      ws.keep.reserve((size_t)a.n_keep * 12);
      float* d_keep = ws.keep.as<float>();
      VO_HIP_CHECK(hipMemcpyAsync(d_keep, keep, (size_t)a.n_keep * 8, hipMemcpyHostToDevice, s));
      a.keep = d_keep;
      a.knext = reinterpret_cast<int32_t*>(d_keep + 2 * (size_t)a.n_keep);
    } else {
      a.keep = nullptr;
      a.knext = nullptr;
    }
    hipLaunchKernelGGL(corner_bin_kernel, dim3(ceil_div(std::max(n, a.n_keep), 256)), dim3(256), 0, s, a);
    VO_HIP_CHECK(hipGetLastError());
    if (a.n_keep) {
      hipLaunchKernelGGL(corner_keep_kernel, dim3(blocks), dim3(256), 0, s, a);
      VO_HIP_CHECK(hipGetLastError());
    } else {
      VO_HIP_CHECK(hipMemsetAsync(a.state, 0, n4, s));
    }
    if (n > kFinishThreads)
      for (int r = 0; r < kParallelRounds; ++r) {
        hipLaunchKernelGGL(corner_round_kernel, dim3(blocks), dim3(256), 0, s, a, r);
        VO_HIP_CHECK(hipGetLastError());
      }
  }
  hipLaunchKernelGGL(corner_finish_kernel, dim3(1), dim3(kFinishThreads), 0, s, a);
  VO_HIP_CHECK(hipGetLastError());
  uint32_t ctl[kCtlWords];
  VO_HIP_CHECK(hipMemcpyAsync(ctl, d_ctl, sizeof ctl, hipMemcpyDeviceToHost, s));
  VO_HIP_CHECK(hipStreamSynchronize(s));
  VO_REQUIRE(ctl[kCtlFailed] == 0, VO_ERR_HIP, "corner selection did not converge");
  int rounds = (int)ctl[kCtlRounds];
  for (int r = 0; r < kParallelRounds; ++r) rounds += ctl[kCtlEntry + r] ? 1 : 0;
  ws.stats[0] = n;
  ws.stats[1] = rounds;
  ws.stats[2] = (int32_t)ctl[kCtlOut];
  ws.stats[3] = a.side;
  return (int)ctl[kCtlOut];
}

}  // namespace

void corner_response_host(vo_ctx* ctx, const uint8_t* img, int h, int w, int block_radius, float* out) {
  CornerWorkspace& ws = ctx->corners;
  const size_t npix = (size_t)h * w;
  const uint8_t* d_img = device_image(ctx, img, 0, h, w, "vo_corner_response");
  uint32_t* d_ctl = control(ctx);
  ws.resp.reserve(npix * 4);
  launch_response(ctx, d_img, nullptr, h, w, block_radius, ws.resp.as<float>(), d_ctl);
  VO_HIP_CHECK(hipMemcpyAsync(out, ws.resp.ptr, npix * 4, hipMemcpyDeviceToHost, ctx->stream));
  VO_HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

void good_features_host(vo_ctx* ctx, const uint8_t* img, uint64_t tag, int h, int w, const uint8_t* mask,
                        const float* keep, int n_keep, const vo_corner_options* opt, float* corners, float* resp,
                        int32_t* n_out) {
  CornerWorkspace& ws = ctx->corners;
  hipStream_t s = ctx->stream;
  const size_t npix = (size_t)h * w;
  for (int32_t& v : ws.stats) v = 0;
  const uint8_t* d_img = device_image(ctx, img, tag, h, w, "vo_good_features");
  const uint8_t* d_mask = nullptr;
  if (mask) {
    ws.mask.reserve(npix);
    VO_HIP_CHECK(hipMemcpyAsync(ws.mask.ptr, mask, npix, hipMemcpyHostToDevice, s));
    d_mask = ws.mask.as<uint8_t>();
  }
  uint32_t* d_ctl = control(ctx);
  ws.resp.reserve(npix * 4);
  const size_t cap = (size_t)(h - 2) * (w - 2);  // every interior pixel can be a candidate
  ws.keys.reserve(2 * cap * 8);
  launch_response(ctx, d_img, d_mask, h, w, opt->block_radius, ws.resp.as<float>(), d_ctl);
  hipLaunchKernelGGL(corner_candidates_kernel, dim3(ceil_div(w, 64), ceil_div(h, 4)), dim3(256), 0, s,
                     ws.resp.as<float>(), d_mask, h, w, opt->quality, d_ctl, ws.keys.as<uint64_t>(), (uint32_t)cap);
  VO_HIP_CHECK(hipGetLastError());
  uint32_t count = 0;
  VO_HIP_CHECK(hipMemcpyAsync(&count, d_ctl + kCtlCount, 4, hipMemcpyDeviceToHost, s));
  VO_HIP_CHECK(hipStreamSynchronize(s));
  const int n = (int)std::min<size_t>(count, cap);
  if (n == 0) return;
  const uint64_t* d_sorted = sort_keys(ctx, n, cap);
  SelArgs a{};
  const int got = select_sorted(ctx, d_sorted, n, nullptr, w, 0, 0, w - 1, h - 1, keep, n_keep, opt->min_distance,
                                opt->max_corners, d_ctl, a);
  if (got > 0) {
    VO_HIP_CHECK(hipMemcpyAsync(corners, a.out_xy, (size_t)got * 8, hipMemcpyDeviceToHost, s));
    if (resp) VO_HIP_CHECK(hipMemcpyAsync(resp, a.out_resp, (size_t)got * 4, hipMemcpyDeviceToHost, s));
    VO_HIP_CHECK(hipStreamSynchronize(s));
  }
  *n_out = got;
}

void corner_select_host(vo_ctx* ctx, const int32_t* xy, const float* resp, int n, const float* keep, int n_keep,
                        float min_distance, int max_corners, int32_t* out_idx, int32_t* n_out) {
  CornerWorkspace& ws = ctx->corners;
  hipStream_t s = ctx->stream;
  for (int32_t& v : ws.stats) v = 0;
  std::vector<uint64_t> keys((size_t)n);
  int lo_x = xy[0], hi_x = xy[0], lo_y = xy[1], hi_y = xy[1];
  for (int i = 0; i < n; ++i) {
    keys[i] = select_key(resp[i], (uint32_t)i);
    lo_x = std::min(lo_x, xy[2 * (size_t)i]);
    hi_x = std::max(hi_x, xy[2 * (size_t)i]);
    lo_y = std::min(lo_y, xy[2 * (size_t)i + 1]);
    hi_y = std::max(hi_y, xy[2 * (size_t)i + 1]);
  }
  const size_t cap = (size_t)n;
  ws.keys.reserve(2 * cap * 8);
  ws.xy.reserve(cap * 8);
  VO_HIP_CHECK(hipMemcpyAsync(ws.keys.ptr, keys.data(), cap * 8, hipMemcpyHostToDevice, s));
  VO_HIP_CHECK(hipMemcpyAsync(ws.xy.ptr, xy, cap * 8, hipMemcpyHostToDevice, s));
  uint32_t* d_ctl = control(ctx);
  const uint64_t* d_sorted = sort_keys(ctx, n, cap);
  SelArgs a{};
  const int got = select_sorted(ctx, d_sorted, n, ws.xy.as<int32_t>(), 0, lo_x, lo_y, hi_x, hi_y, keep, n_keep,
                                min_distance, max_corners, d_ctl, a);
  if (got > 0) {
    VO_HIP_CHECK(hipMemcpyAsync(out_idx, a.out_id, (size_t)got * 4, hipMemcpyDeviceToHost, s));
    VO_HIP_CHECK(hipStreamSynchronize(s));
  }
  *n_out = got;
}

void corner_stats(vo_ctx* ctx, int32_t out[4]) {
  for (int k = 0; k < 4; ++k) out[k] = ctx->corners.stats[k];
}

}  // namespace vo
