// Shi-Tomasi corner detection: the per-pixel and per-candidate arithmetic, shared by the gfx950
// kernels (corners.hip) and the host build (corners_host_check.cpp).
//
// The contract is DESIGN.md §Corners, restated in numpy by tests/corners_ref.py.  Everything summed
// over a block is an int32, so the sums do not depend on tiling or order; the response is three
// double operations and one rounding to float32, compiled without contraction; the distance tests
// are double comparisons of exactly representable integers (pairs) or of once-rounded operations
// (keep-away points).
#pragma once

#include "klt_math.h"

#pragma clang fp contract(off)

namespace vo {
namespace cornm {

using kltm::finite32;
using kltm::reflect;

constexpr int kMaxBlockRadius = 3;
constexpr float kMaxDistance = 1024.f;
constexpr int kMaxSelectCoord = 1 << 24;  // vo_corner_select: |x|, |y| at most this (exact squares in int64)

// The 3 x 3 Sobel derivatives from the patch v[row][column] around a pixel.
VO_HD void sobel(const int v[3][3], int& gx, int& gy) {
  gx = (v[0][2] + 2 * v[1][2] + v[2][2]) - (v[0][0] + 2 * v[1][0] + v[2][0]);
  gy = (v[2][0] + 2 * v[2][1] + v[2][2]) - (v[0][0] + 2 * v[0][1] + v[0][2]);
}

// The derivatives at pixel (x, y) of the w x h image I, 0 <= x < w, 0 <= y < h: its neighbours reflected.
VO_HD void sobel_at(const uint8_t* I, int w, int h, int x, int y, int& gx, int& gy) {
  const int xs[3] = {reflect(x - 1, w), x, reflect(x + 1, w)};
  const int ys[3] = {reflect(y - 1, h), y, reflect(y + 1, h)};
  int v[3][3];
  KLT_UNROLL
  for (int j = 0; j < 3; ++j) {
    KLT_UNROLL
    for (int i = 0; i < 3; ++i) v[j][i] = I[(size_t)ys[j] * w + xs[i]];
  }
  sobel(v, gx, gy);
}

// The smaller eigenvalue of [[a, b], [b, c]] from the block's integer sums.
VO_HD float response(int32_t a, int32_t b, int32_t c) {
  const int64_t d = (int64_t)a - (int64_t)c;
  const int64_t q = d * d + 4 * ((int64_t)b * (int64_t)b);
  const double tr = (double)(a + c);
  const double root = kltm::klt_sqrt((double)q);
  const double diff = tr - root;
  return (float)(0.5 * diff);
}

VO_HD uint32_t float_bits(float v) {
  union {
    float f;
    uint32_t u;
  } c;
  c.f = v;
  return c.u;
}

VO_HD float bits_float(uint32_t u) {
  union {
    float f;
    uint32_t u;
  } c;
  c.u = u;
  return c.f;
}

// The comparison domain of the global maximum: the bits of max(resp, +0), which order as unsigned.
// A maximum that is not > 0 means "no corners", so nothing is lost below zero.
VO_HD uint32_t max_domain(float resp) { return resp > 0.f ? float_bits(resp) : 0u; }

VO_HD bool above_threshold(float resp, float quality, float rmax) {
  return (double)resp > (double)quality * (double)rmax;  // the product of two float32 is exact in double
}

// Sort key of a candidate (resp > 0): ascending keys are resp descending, then index ascending.
VO_HD uint64_t candidate_key(float resp, uint32_t index) { return (uint64_t)(~float_bits(resp)) << 32 | index; }
VO_HD float key_response(uint64_t key) { return bits_float(~(uint32_t)(key >> 32)); }

// The same for any finite response (vo_corner_select): the usual order-preserving map of a float
// to unsigned, -0 taken as +0.
VO_HD uint64_t select_key(float resp, uint32_t row) {
  uint32_t u = float_bits(resp == 0.f ? 0.f : resp);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return (uint64_t)(~u) << 32 | row;
}

VO_HD double distance2(float d) { return (double)d * (double)d; }

// A keep-away point (finite in both coordinates) rejects the candidate at (x, y).
VO_HD bool keep_rejects(int x, int y, float kx, float ky, double d2) {
  const double dx = (double)x - (double)kx, dy = (double)y - (double)ky;
  const double xx = dx * dx, yy = dy * dy;
  return xx + yy < d2;
}

// An accepted corner rejects the candidate dx, dy away.
VO_HD bool pair_rejects(int64_t dx, int64_t dy, double d2) { return (double)(dx * dx + dy * dy) < d2; }

// Side of the grid cells the selection bins by: ceil(d), at least 1 (any side >= d is correct).
VO_HD int cell_side(float d) {
  const int s = (int)ceilf(d);
  return s < 1 ? 1 : s;
}

}  // namespace cornm
}  // namespace vo
