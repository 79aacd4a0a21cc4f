// Sparse pyramidal Lucas-Kanade tracking on gfx950 (vo_klt_track, vo_klt_pyramid).
//
// The contract is the restatement in tests/klt_ref.py; the per-track sequence is
// klt_math.h, compiled here without FMA contraction and shared with the host build
// (klt_host_check.cpp).  Every window sum is an integer, so the results do not depend on the
// mapping below.
//   klt_pyr_down_kernel  one thread per pixel of the next level (5 x 5 binomial, reflected);
//                        levels stay uint8 in HBM, concatenated and unpitched: a KITTI-size
//                        pyramid is under 1 MB and sits in L2 for the track kernel.
//   klt_track_kernel     one 64-lane wave per point, four waves per workgroup, all levels in one
//                        launch.  A lane holds ceil((2r+1)^2 / 64) pixels of the template
//                        (I, dIx, dIy and the pixel's window offset packed into two registers
//                        each), sums its int32 partials, and the wave reduces them to int64 with
//                        xor shuffles; every lane then runs the same double solve, so the
//                        control flow of a wave is uniform.  The derivatives are taken from the
//                        uint8 level when the template is formed: no derivative image is stored.
//                        The forward-backward check is the same kernel launched again with the
//                        pyramids swapped: it re-tracks the accepted points and writes status 4.
// Every tap is bounds-proven before it is read: the inside test of klt_math.h covers the window
// and its +1 taps, and the template's 4 x 4 patches go through the reflection.
//
// Pyramids of tagged images are cached on the context (kCacheEntries, LRU), keyed by
// (tag, h, w, levels built): a hit neither uploads nor rebuilds.
#include <cstring>
#include <utility>

#include "klt_math.h"
#include "vo_ctx.h"

#pragma clang fp contract(off)

namespace vo {
namespace {

using namespace kltm;

constexpr int kWavesPerBlock = 4;

struct WavePolicy {
  static constexpr int kSlots = (kMaxPixels + 63) / 64;
  __device__ static int first() { return threadIdx.x & 63; }
  __device__ static int stride() { return 64; }
  __device__ static int64_t sum(int v) {
    long long s = v;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    return s;
  }
};

__global__ __launch_bounds__(256) void klt_pyr_down_kernel(const uint8_t* src, int sw, int sh, uint8_t* dst, int dw,
                                                           int dh) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= dw || y >= dh) return;
  dst[(size_t)y * dw + x] = pyr_down_pixel(src, sw, sh, x, y);
}

struct TrackArgs {
  Pyr A, B;          // track from A into B
  Options o;
  const float* p0;   // (n, 2) start points; the back pass compares its result with these
  float* p1;         // (n, 2) in: the guess (has_guess); out: the tracked points
  uint8_t* status;   // (n)
  float* err;        // (n)
  int n;
  int has_guess;
  int back;          // the forward-backward pass over the forward pass's outputs
  float fb_thresh;
};

__global__ __launch_bounds__(64 * kWavesPerBlock) void klt_track_kernel(TrackArgs a) {
  const int i = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);  // wave-uniform
  if (i >= a.n) return;
  const float px = a.p0[2 * (size_t)i], py = a.p0[2 * (size_t)i + 1];
  float x, y, e;
  uint8_t st;
  if (!a.back) {
    float gx = 0.f, gy = 0.f;
    if (a.has_guess) {
      gx = a.p1[2 * (size_t)i];
      gy = a.p1[2 * (size_t)i + 1];
    }
    track_point<WavePolicy>(a.A, a.B, a.o, px, py, a.has_guess != 0, gx, gy, x, y, st, e);
  } else {
    if (a.status[i] != kTracked) return;
    const float fx = a.p1[2 * (size_t)i], fy = a.p1[2 * (size_t)i + 1];
    track_point<WavePolicy>(a.A, a.B, a.o, fx, fy, true, px, py, x, y, st, e);
    if (!fb_fails(st, x, y, px, py, a.fb_thresh)) return;  // the forward result stands
    st = kFbFailed;
    x = px;
    y = py;
    e = 0.f;
  }
  if ((threadIdx.x & 63) == 0) {
    a.p1[2 * (size_t)i] = x;
    a.p1[2 * (size_t)i + 1] = y;
    a.status[i] = st;
    a.err[i] = e;
  }
}

// Levels 1 .. L - 1 of the pyramid whose level 0 is already in d_pyr.
void build_levels(vo_ctx* ctx, uint8_t* d_pyr, const Level* lv, int L) {
  for (int l = 1; l < L; ++l) {
    hipLaunchKernelGGL(klt_pyr_down_kernel, dim3(ceil_div(lv[l].w, 64), ceil_div(lv[l].h, 4)), dim3(256), 0,
                       ctx->stream, d_pyr + lv[l - 1].off, lv[l - 1].w, lv[l - 1].h, d_pyr + lv[l].off, lv[l].w,
                       lv[l].h);
    VO_HIP_CHECK(hipGetLastError());
  }
}

// The device pyramid of an image: the cache entry of a nonzero tag (built on a miss, the least
// recently used entry evicted), or scratch entry `slot` rebuilt for an untagged one.
const uint8_t* acquire(vo_ctx* ctx, const uint8_t* img, uint64_t tag, int h, int w, const Level* lv, int L,
                       int64_t bytes, int slot) {
  KltWorkspace& ws = ctx->klt;
  KltPyramid* e = nullptr;
  if (tag != 0) {
    for (KltPyramid& c : ws.cache)
      if (c.valid && c.tag == tag && c.h == h && c.w == w && c.levels == L) e = &c;
    if (e) {
      e->used = ++ws.clock;
      return e->buf.as<uint8_t>();
    }
    e = &ws.cache[0];
    for (KltPyramid& c : ws.cache)
      if (e->valid && (!c.valid || c.used < e->used)) e = &c;
  } else {
    e = &ws.scratch[slot];
  }
  VO_REQUIRE(img, VO_ERR_ARG, "vo_klt_track: image %d is NULL and its tag is not in the pyramid cache", slot);
  e->valid = false;
  e->buf.reserve((size_t)bytes);
  VO_HIP_CHECK(hipMemcpyAsync(e->buf.ptr, img, (size_t)h * w, hipMemcpyHostToDevice, ctx->stream));
  build_levels(ctx, e->buf.as<uint8_t>(), lv, L);
  e->tag = tag;
  e->h = h;
  e->w = w;
  e->levels = L;
  e->used = ++ws.clock;
  e->valid = tag != 0;
  return e->buf.as<uint8_t>();
}

}  // namespace

int klt_layout(int h, int w, int levels, int win_radius, int64_t* out, int n) {
  Level lv[kMaxLevels];
  int L = 1;
  const int64_t bytes = layout(h, w, levels, win_radius, lv, &L);
  int64_t vals[2 + 3 * kMaxLevels] = {L, bytes};
  for (int l = 0; l < L; ++l) {
    vals[2 + 3 * l] = lv[l].h;
    vals[3 + 3 * l] = lv[l].w;
    vals[4 + 3 * l] = lv[l].off;
  }
  const int count = 2 + 3 * L;
  for (int k = 0; k < count && k < n; ++k) out[k] = vals[k];
  return count;
}

void klt_pyramid_host(vo_ctx* ctx, const uint8_t* img, int h, int w, int levels, uint8_t* out, int64_t cap,
                      int32_t* levels_out) {
  Level lv[kMaxLevels];
  int L = 1;
  const int64_t bytes = layout(h, w, levels, 0, lv, &L);
  VO_REQUIRE(cap >= bytes, VO_ERR_ARG, "vo_klt_pyramid: output too small (%lld bytes needed)", (long long)bytes);
  KltPyramid& e = ctx->klt.scratch[0];
  e.buf.reserve((size_t)bytes);
  VO_HIP_CHECK(hipMemcpyAsync(e.buf.ptr, img, (size_t)h * w, hipMemcpyHostToDevice, ctx->stream));
  build_levels(ctx, e.buf.as<uint8_t>(), lv, L);
  VO_HIP_CHECK(hipMemcpyAsync(out, e.buf.ptr, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream));
  VO_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (levels_out) *levels_out = L;
}

void klt_track_host(vo_ctx* ctx, const uint8_t* img0, uint64_t tag0, const uint8_t* img1, uint64_t tag1, int h, int w,
                    const float* pts0, float* pts1, int n, const vo_klt_options* opt, uint8_t* status, float* err,
                    int32_t* n_tracked) {
  hipStream_t s = ctx->stream;
  TrackArgs a;
  int L = 1;
  const int64_t bytes = layout(h, w, opt->levels, opt->win_radius, a.A.lv, &L);
  for (int l = 0; l < kMaxLevels; ++l) {
    if (l >= L) a.A.lv[l] = Level{0, 0, 0};
    a.B.lv[l] = a.A.lv[l];
  }
  a.A.base = acquire(ctx, img0, tag0, h, w, a.A.lv, L, bytes, 0);
  a.B.base = acquire(ctx, img1, tag1, h, w, a.A.lv, L, bytes, 1);
  a.o = Options{opt->win_radius, L, opt->max_iters, opt->eps, opt->min_eig, opt->max_err};
  // staging: pts0 | pts1 (the guess in, the result out) | err | status
  const size_t np = (size_t)n * 8;
  ctx->klt.pts.reserve(2 * np + (size_t)n * 4 + (size_t)n + 16);
  char* d = ctx->klt.pts.as<char>();
  a.p0 = reinterpret_cast<const float*>(d);
  a.p1 = reinterpret_cast<float*>(d + np);
  a.err = reinterpret_cast<float*>(d + 2 * np);
  a.status = reinterpret_cast<uint8_t*>(d + 2 * np + (size_t)n * 4);
  a.n = n;
  a.has_guess = (opt->flags & VO_KLT_GUESS) ? 1 : 0;
  a.back = 0;
  a.fb_thresh = opt->fb_thresh;
  VO_HIP_CHECK(hipMemcpyAsync(d, pts0, np, hipMemcpyHostToDevice, s));
  if (a.has_guess) VO_HIP_CHECK(hipMemcpyAsync(d + np, pts1, np, hipMemcpyHostToDevice, s));
  const dim3 grid(ceil_div(n, kWavesPerBlock)), block(64 * kWavesPerBlock);
  hipLaunchKernelGGL(klt_track_kernel, grid, block, 0, s, a);
  VO_HIP_CHECK(hipGetLastError());
  if (opt->flags & VO_KLT_FB) {
    std::swap(a.A.base, a.B.base);
    a.back = 1;
    hipLaunchKernelGGL(klt_track_kernel, grid, block, 0, s, a);
    VO_HIP_CHECK(hipGetLastError());
  }
  VO_HIP_CHECK(hipMemcpyAsync(pts1, d + np, np, hipMemcpyDeviceToHost, s));
  if (err) VO_HIP_CHECK(hipMemcpyAsync(err, a.err, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  VO_HIP_CHECK(hipMemcpyAsync(status, a.status, (size_t)n, hipMemcpyDeviceToHost, s));
  VO_HIP_CHECK(hipStreamSynchronize(s));
  int good = 0;
  for (int i = 0; i < n; ++i) good += status[i] == kTracked ? 1 : 0;
  if (n_tracked) *n_tracked = good;
}

}  // namespace vo
