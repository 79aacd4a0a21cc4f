// Steered BRIEF: the per-point arithmetic, shared by the gfx950 kernel (brief.hip) and the host
// build (brief_host_check.cpp).
//
// The contract is include/vo_hip.h (vo_brief_describe) and DESIGN.md §BRIEF, restated in numpy by
// tests/brief_ref.py.  Every quantity is an integer: the patch is bytes, the moments are int32, the
// bin is an argmax over int64 dot products, the box sums fit 16 bits, a bit is a strict integer
// comparison.  So the result does not depend on which lane takes which pixel or test, nor on the
// order of a reduction.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "brief_pattern.h"
#include "klt_math.h"

namespace vo {
namespace briefm {

using kltm::reflect;

constexpr int kBins = 32, kTests = 256, kWords = kTests / 32;
constexpr int kPatchR = 15, kPatch = 2 * kPatchR + 1;  // the patch: 31 x 31 bytes around the centre
constexpr int kDisc2 = kPatchR * kPatchR;              // moments over dx^2 + dy^2 <= 225
constexpr int kBoxR = 2;                               // box sums over 5 x 5
constexpr int kPlaneR = kPatchR - kBoxR, kPlane = 2 * kPlaneR + 1;  // box centres: |u|, |v| <= 13

// Test t of bin k: int8 coordinates packed px | py << 8 | qx << 16 | qy << 24.
struct Test {
  int px, py, qx, qy;
};

constexpr Test unpack_test(uint32_t v) {
  return Test{(int)(int8_t)(v & 0xffu), (int)(int8_t)((v >> 8) & 0xffu), (int)(int8_t)((v >> 16) & 0xffu),
              (int)(int8_t)(v >> 24)};
}

// The bound every plane index below rests on, checked where the table is compiled: a box centre of
// the committed table lies in [-kPlaneR, kPlaneR]^2, so its 5 x 5 box lies in the patch.
constexpr bool pattern_in_plane() {
  for (int i = 0; i < kBins * kTests; ++i) {
    const Test t = unpack_test(kBriefPattern[i]);
    if (t.px < -kPlaneR || t.px > kPlaneR || t.py < -kPlaneR || t.py > kPlaneR || t.qx < -kPlaneR || t.qx > kPlaneR ||
        t.qy < -kPlaneR || t.qy > kPlaneR)
      return false;
  }
  return true;
}
static_assert(pattern_in_plane(), "brief_pattern.h: a test point lies outside the box-sum plane");

// Plane index of the box centred (u, v) of the patch's centre; in [0, kPlane^2) by the assert above.
VO_HD int plane_index(int u, int v) { return (v + kPlaneR) * kPlane + (u + kPlaneR); }

// Status 0 and the centre pixel, or status 1: a coordinate is not finite, is 2^24 or more in
// magnitude, or rounds (half to even) to a pixel outside the w x h image.
VO_HD bool centre(float x, float y, int w, int h, int& cx, int& cy) {
  cx = cy = 0;
  if (!(fabsf(x) < 16777216.f) || !(fabsf(y) < 16777216.f)) return false;  // NaN and inf fail too
  const int ix = (int)rintf(x), iy = (int)rintf(y);
  if (ix < 0 || ix > w - 1 || iy < 0 || iy > h - 1) return false;
  cx = ix;
  cy = iy;
  return true;
}

VO_HD bool in_disc(int dx, int dy) { return dx * dx + dy * dy <= kDisc2; }

// The bin: the k maximising m10 C[k] + m01 S[k] in int64, ties to the lowest k.
VO_HD int best_bin(int32_t m10, int32_t m01) {
  int best = 0;
  int64_t bv = (int64_t)m10 * kBriefDirC[0] + (int64_t)m01 * kBriefDirS[0];
  for (int k = 1; k < kBins; ++k) {
    const int64_t v = (int64_t)m10 * kBriefDirC[k] + (int64_t)m01 * kBriefDirS[k];
    if (v > bv) {
      bv = v;
      best = k;
    }
  }
  return best;
}

VO_HD Test test_of(int bin, int t) { return unpack_test(kBriefPattern[bin * kTests + t]); }

// One point on one caller: the host's whole sequence (the kernel deals the same steps over a wave).
// des: 8 words; returns the status.
inline uint8_t describe_point(const uint8_t* img, int h, int w, float x, float y, uint32_t des[kWords], int32_t& bin) {
  for (int k = 0; k < kWords; ++k) des[k] = 0;
  bin = 0;
  int cx, cy;
  if (!centre(x, y, w, h, cx, cy)) return 1;
  uint8_t patch[kPatch * kPatch];
  int32_t m10 = 0, m01 = 0;
  for (int dy = -kPatchR; dy <= kPatchR; ++dy)
    for (int dx = -kPatchR; dx <= kPatchR; ++dx) {
      const uint8_t v = img[(size_t)reflect(cy + dy, h) * w + reflect(cx + dx, w)];
      patch[(dy + kPatchR) * kPatch + dx + kPatchR] = v;
      if (in_disc(dx, dy)) {
        m10 += dx * (int)v;
        m01 += dy * (int)v;
      }
    }
  bin = best_bin(m10, m01);
  uint16_t plane[kPlane * kPlane];
  for (int v = -kPlaneR; v <= kPlaneR; ++v)
    for (int u = -kPlaneR; u <= kPlaneR; ++u) {
      int s = 0;
      for (int j = -kBoxR; j <= kBoxR; ++j)
        for (int i = -kBoxR; i <= kBoxR; ++i) s += patch[(v + j + kPatchR) * kPatch + u + i + kPatchR];
      plane[plane_index(u, v)] = (uint16_t)s;
    }
  for (int t = 0; t < kTests; ++t) {
    const Test q = test_of(bin, t);
    if (plane[plane_index(q.px, q.py)] < plane[plane_index(q.qx, q.qy)]) des[t >> 5] |= 1u << (t & 31);
  }
  return 0;
}

}  // namespace briefm
}  // namespace vo
