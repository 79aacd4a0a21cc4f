// Steered BRIEF descriptors on gfx950 (vo_brief_describe, vo_brief_pattern).
//
// The contract (include/vo_hip.h) is the restatement in tests/brief_ref.py; the
// per-point arithmetic is brief_math.h, shared with the host build (brief_host_check.cpp).  Every
// quantity is an integer, so the bits do not depend on the mapping below.
//   brief_describe_kernel  one 64-lane wave per point, four waves per workgroup, each wave in its
//                          own LDS slice:
//     1. the 31 x 31 patch as bytes (rows 32 apart), read through reflect(); the lane that loads a
//        pixel of the disc adds dx I and dy I to its partial moments, which xor shuffles sum;
//     2. the 5 x 5 box sums separably: 31 x 27 row sums, then the 27 x 27 plane, both uint16
//        (at most 25 * 255 = 6375);
//     3. every lane evaluates the 32 dot products on the same moments, so all agree on the bin;
//     4. lane l evaluates tests 64 j + l, j = 0..3: one 32-bit load of the packed test, two plane
//        reads, a strict compare; four ballots are the eight words, stored by lane 0.
//   A point of status 1 skips the work and stores zeros.  Waves past n do nothing but take part in
//   the barriers, which stand outside every branch.
// Bounds.  Global reads: row reflect(cy + dy, h) in [0, h), column reflect(cx + dx, w) in [0, w).
// Patch slice: (dy + 15) * 32 + dx + 15 <= 30 * 32 + 30 < 31 * 32.  Row sums: r * 27 + c with r < 31,
// c < 27 reads patch columns c .. c + 4 <= 30.  Plane: r, c < 27 reads row-sum rows r .. r + 4 <= 30.
// Tests: plane_index(u, v) with |u|, |v| <= 13 by brief_math.h's static_assert over the committed
// table, so the index is in [0, 27 * 27).  Outputs: point i < n only.
#include <cstring>

#include "brief_math.h"
#include "vo_ctx.h"

namespace vo {
namespace {

using namespace briefm;

constexpr int kWaves = 4;
constexpr int kPatchPitch = 32;

struct Slice {
  uint8_t patch[kPatch * kPatchPitch];
  uint16_t rows[kPatch * kPlane];
  uint16_t plane[kPlane * kPlane];
};

__global__ __launch_bounds__(64 * kWaves) void brief_describe_kernel(const uint8_t* __restrict__ img, int h, int w,
                                                                     const float* __restrict__ pts, int n,
                                                                     uint32_t* __restrict__ des,
                                                                     int32_t* __restrict__ bins,
                                                                     uint8_t* __restrict__ status) {
  __shared__ Slice s_slice[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * kWaves + wave;
  Slice& S = s_slice[wave];
  int cx = 0, cy = 0;
  bool live = false;
  if (i < n) live = centre(pts[2 * (size_t)i], pts[2 * (size_t)i + 1], w, h, cx, cy);  // wave-uniform

  int32_t m10 = 0, m01 = 0;
  if (live) {
    for (int p = lane; p < kPatch * kPatch; p += 64) {
      const int py = p / kPatch, px = p - py * kPatch;
      const int dx = px - kPatchR, dy = py - kPatchR;
      const int v = img[(size_t)reflect(cy + dy, h) * w + reflect(cx + dx, w)];
      S.patch[py * kPatchPitch + px] = (uint8_t)v;
      if (in_disc(dx, dy)) {
        m10 += dx * v;
        m01 += dy * v;
      }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      m10 += __shfl_xor(m10, m, 64);
      m01 += __shfl_xor(m01, m, 64);
    }
  }
  __syncthreads();
  if (live) {
    for (int p = lane; p < kPatch * kPlane; p += 64) {
      const int r = p / kPlane, c = p - r * kPlane;
      const uint8_t* q = &S.patch[r * kPatchPitch + c];
      S.rows[p] = (uint16_t)(q[0] + q[1] + q[2] + q[3] + q[4]);
    }
  }
  __syncthreads();
  if (live) {
    for (int p = lane; p < kPlane * kPlane; p += 64) {
      const uint16_t* q = &S.rows[p];  // row r, column c: rows r .. r + 4
      S.plane[p] = (uint16_t)(q[0] + q[kPlane] + q[2 * kPlane] + q[3 * kPlane] + q[4 * kPlane]);
    }
  }
  __syncthreads();
  if (i >= n) return;
  const int bin = live ? best_bin(m10, m01) : 0;
  uint64_t votes[kTests / 64];
#pragma unroll
  for (int j = 0; j < kTests / 64; ++j) {
    bool bit = false;
    if (live) {
      const Test t = test_of(bin, 64 * j + lane);
      bit = S.plane[plane_index(t.px, t.py)] < S.plane[plane_index(t.qx, t.qy)];
    }
    votes[j] = __ballot(bit);
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < kTests / 64; ++j) {
      des[(size_t)i * kWords + 2 * j] = (uint32_t)votes[j];
      des[(size_t)i * kWords + 2 * j + 1] = (uint32_t)(votes[j] >> 32);
    }
    bins[i] = bin;
    status[i] = live ? 0 : 1;
  }
}

// Level 0 of a cached KLT pyramid with this tag and shape, or the image uploaded into scratch.
const uint8_t* device_image(vo_ctx* ctx, const uint8_t* img, uint64_t tag, int h, int w) {
  if (tag != 0)
    for (const KltPyramid& c : ctx->klt.cache)
      if (c.valid && c.tag == tag && c.h == h && c.w == w) return c.buf.as<uint8_t>();
  VO_REQUIRE(img, VO_ERR_ARG, "vo_brief_describe: the image is NULL and its tag is not in the pyramid cache");
  BriefWorkspace& ws = ctx->brief;
  ws.img.reserve((size_t)h * w);
  VO_HIP_CHECK(hipMemcpyAsync(ws.img.ptr, img, (size_t)h * w, hipMemcpyHostToDevice, ctx->stream));
  return ws.img.as<uint8_t>();
}

}  // namespace

void brief_describe_host(vo_ctx* ctx, const uint8_t* img, uint64_t tag, int h, int w, const float* pts, int n,
                         uint32_t* des_out, int32_t* bin_out, uint8_t* status_out) {
  BriefWorkspace& ws = ctx->brief;
  hipStream_t s = ctx->stream;
  const uint8_t* d_img = device_image(ctx, img, tag, h, w);
  const size_t np = (size_t)n;
  ws.pts.reserve(np * 8);
  ws.out.reserve(np * (kWords * 4 + 4 + 1));
  float* d_pts = ws.pts.as<float>();
  uint32_t* d_des = ws.out.as<uint32_t>();
  int32_t* d_bin = reinterpret_cast<int32_t*>(d_des + np * kWords);
  uint8_t* d_status = reinterpret_cast<uint8_t*>(d_bin + np);
  VO_HIP_CHECK(hipMemcpyAsync(d_pts, pts, np * 8, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(brief_describe_kernel, dim3(ceil_div(n, kWaves)), dim3(64 * kWaves), 0, s, d_img, h, w, d_pts, n,
                     d_des, d_bin, d_status);
  VO_HIP_CHECK(hipGetLastError());
  VO_HIP_CHECK(hipMemcpyAsync(des_out, d_des, np * kWords * 4, hipMemcpyDeviceToHost, s));
  if (bin_out) VO_HIP_CHECK(hipMemcpyAsync(bin_out, d_bin, np * 4, hipMemcpyDeviceToHost, s));
  if (status_out) VO_HIP_CHECK(hipMemcpyAsync(status_out, d_status, np, hipMemcpyDeviceToHost, s));
  VO_HIP_CHECK(hipStreamSynchronize(s));
}

void brief_pattern(int8_t* out, int32_t* dir_out) {
  for (int i = 0; i < kBins * kTests; ++i) {
    const Test t = unpack_test(kBriefPattern[i]);
    out[4 * i] = (int8_t)t.px;
    out[4 * i + 1] = (int8_t)t.py;
    out[4 * i + 2] = (int8_t)t.qx;
    out[4 * i + 3] = (int8_t)t.qy;
  }
  for (int k = 0; k < kBins; ++k) {
    dir_out[k] = kBriefDirC[k];
    dir_out[kBins + k] = kBriefDirS[k];
  }
}

}  // namespace vo
