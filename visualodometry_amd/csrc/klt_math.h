// Pyramidal Lucas-Kanade tracking of one point: the whole per-track sequence, shared by the
// gfx950 kernel (klt.hip) and the host build (klt_host_check.cpp).
//
// The contract is DESIGN.md §KLT, restated in numpy by tests/klt_ref.py.  Everything summed over
// the window is an integer (fixed-point patches as in OpenCV's calcOpticalFlowPyrLK), so the sums
// do not depend on which lane takes which pixel nor on the order of the reduction; the 2 x 2
// solve, the update and the stop rules are double / float32 operations rounded once each, compiled
// without contraction.  A policy P says how the window's pixels are dealt out and summed:
//   P::kSlots          pixels one caller holds at most (its share of the template)
//   P::first(), P::stride()   the caller's pixels are first(), first() + stride(), ...
//   P::sum(int)        the sum over all callers of a track, as int64, known to every caller
// The kernel's policy is one 64-lane wave per track, the host's one caller holding every pixel.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

#ifndef VO_HD
#define VO_HD __host__ __device__ inline __attribute__((always_inline))
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define KLT_UNROLL _Pragma("unroll")
#else
#define KLT_UNROLL
#endif

namespace vo {
namespace kltm {

constexpr int kMaxLevels = 8;
constexpr int kMaxRadius = 15;
constexpr int kMaxPixels = (2 * kMaxRadius + 1) * (2 * kMaxRadius + 1);

enum Status : uint8_t {
  kTracked = 0, kStartOutside = 1, kDegenerate = 2, kLeftImage = 3, kFbFailed = 4, kErrAbove = 5, kBadInput = 6
};

struct Level {
  int64_t off;  // bytes from the pyramid's base
  int32_t w, h;
};

struct Pyr {
  const uint8_t* base;
  Level lv[kMaxLevels];
};

struct Options {
  int32_t r, levels /* L_eff */, max_iters;
  float eps, min_eig, max_err;
};

// Level sizes of an h x w image and L_eff: the largest L <= levels whose level L - 1 is at least
// (2r + 3) x (2r + 3), at least 1.  Returns the pyramid's bytes (levels concatenated, unpitched).
inline int64_t layout(int h, int w, int levels, int r, Level* lv, int* l_eff) {
  const int m = 2 * r + 3;
  int L = 1;
  lv[0] = Level{0, w, h};
  int64_t bytes = (int64_t)h * w;
  while (L < levels && L < kMaxLevels) {
    const int nw = (lv[L - 1].w + 1) / 2, nh = (lv[L - 1].h + 1) / 2;
    if (nw < m || nh < m) break;
    lv[L] = Level{bytes, nw, nh};
    bytes += (int64_t)nw * nh;
    ++L;
  }
  *l_eff = L;
  return bytes;
}

// Reflection without repeating the edge (-1 -> 1, n -> n - 2), total for any n >= 1.
VO_HD int reflect(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}

// pyrDown: one pixel of the next level.
VO_HD uint8_t pyr_down_pixel(const uint8_t* I, int w, int h, int x, int y) {
  const int k[5] = {1, 4, 6, 4, 1};
  int acc = 0;
  KLT_UNROLL
  for (int j = 0; j < 5; ++j) {
    const uint8_t* row = I + (size_t)reflect(2 * y + j - 2, h) * w;
    int s = 0;
    KLT_UNROLL
    for (int i = 0; i < 5; ++i) s += k[i] * row[reflect(2 * x + i - 2, w)];
    acc += k[j] * s;
  }
  return (uint8_t)((acc + 128) >> 8);
}

// The window with corner c - r: its integer corner, the bilinear weights (x 16384) and whether it
// and its +1 taps lie inside the w x h level.  A non-finite centre is outside.
struct Win {
  int ix, iy, w00, w01, w10, w11;
  bool inside;
};

VO_HD Win window(float cx, float cy, int r, int w, int h) {
  Win o{0, 0, 0, 0, 0, 0, false};
  const float qx = cx - (float)r, qy = cy - (float)r;
  const float fx = floorf(qx), fy = floorf(qy);
  o.inside = fx >= 0.f && fy >= 0.f && fx <= (float)(w - 2 * r - 2) && fy <= (float)(h - 2 * r - 2);
  if (!o.inside) return o;
  o.ix = (int)fx;
  o.iy = (int)fy;
  const float a = qx - fx, b = qy - fy;
  const float u = 1.f - a, v = 1.f - b;
  o.w00 = (int)rintf((u * v) * 16384.f);
  o.w01 = (int)rintf((a * v) * 16384.f);
  o.w10 = (int)rintf((u * b) * 16384.f);
  o.w11 = 16384 - o.w00 - o.w01 - o.w10;
  return o;
}

// The normal matrix of a template from its integer sums, and whether it can be solved.
struct Gram {
  double a11, a12, a22, D;
  bool ok;
};

VO_HD double klt_sqrt(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dsqrt_rn(x);
#else
  return std::sqrt(x);
#endif
}

VO_HD Gram gram(int64_t A11, int64_t A12, int64_t A22, int r, float min_eig) {
  const double s = 1.0 / 1048576.0;  // 2^-20
  Gram g;
  g.a11 = (double)A11 * s;
  g.a12 = (double)A12 * s;
  g.a22 = (double)A22 * s;
  const double p1 = g.a11 * g.a22, p2 = g.a12 * g.a12;
  g.D = p1 - p2;
  const double t1 = g.a11 - g.a22;
  const double t2 = t1 * t1, t4 = 4.0 * p2;
  const double root = klt_sqrt(t2 + t4);
  const double u = g.a22 + g.a11;
  const double W = (double)(2 * r + 1);
  const double min_e = (u - root) / (2.0 * (W * W));
  g.ok = !(min_e < (double)min_eig) && !(g.D < (double)FLT_EPSILON);
  return g;
}

struct Step {
  double dx, dy;
};

VO_HD Step step(const Gram& g, int64_t B1, int64_t B2) {
  const double s = 1.0 / 1048576.0;
  const double b1 = (double)B1 * s, b2 = (double)B2 * s;
  Step d;
  const double x1 = g.a12 * b2, x2 = g.a22 * b1;
  const double y1 = g.a12 * b1, y2 = g.a11 * b2;
  d.dx = (x1 - x2) / g.D;
  d.dy = (y1 - y2) / g.D;
  return d;
}

// n += delta and the two stop rules; true when the level's iteration ends.  prev is the previous
// iteration's step (j > 0).
VO_HD bool update(float& nx, float& ny, const Step& d, Step& prev, int j, float eps) {
  const float fx = (float)d.dx, fy = (float)d.dy;
  nx = nx + fx;
  ny = ny + fy;
  const double xx = d.dx * d.dx, yy = d.dy * d.dy;
  const double e2 = (double)eps * (double)eps;
  if (xx + yy <= e2) return true;
  if (j > 0 && fabs(d.dx + prev.dx) < 0.01 && fabs(d.dy + prev.dy) < 0.01) {
    nx = nx - 0.5f * fx;
    ny = ny - 0.5f * fy;
    return true;
  }
  prev = d;
  return false;
}

// The forward-backward verdict: (bx, by) is where the back track of a point that started at
// (px, py) ended, bstatus how it ended.
VO_HD bool fb_fails(uint8_t bstatus, float bx, float by, float px, float py, float fb_thresh) {
  if (bstatus != kTracked) return true;
  const float dx = bx - px, dy = by - py;
  const double d2 = (double)dx * (double)dx + (double)dy * (double)dy;
  return d2 > (double)fb_thresh * (double)fb_thresh;
}

VO_HD bool finite32(float v) { return v - v == 0.f; }

// One track from pyramid A to pyramid B (the same layout).  The start window at (X, Y) .. +2r+1 is
// inside the level, so the 4 x 4 patch around a pixel of it reaches one past the level at most:
// that is what the reflection is for.
template <class P>
VO_HD void track_point(const Pyr& A, const Pyr& B, const Options& o, float p0x, float p0y, bool has_guess, float gx,
                       float gy, float& outx, float& outy, uint8_t& status, float& err) {
  const int r = o.r, W = 2 * r + 1, npix = W * W;
  status = kTracked;
  err = 0.f;
  outx = p0x;
  outy = p0y;
  if (!finite32(p0x) || !finite32(p0y) || (has_guess && (!finite32(gx) || !finite32(gy)))) {
    status = kBadInput;
    return;
  }
  if (A.lv[0].w < 2 * r + 3 || A.lv[0].h < 2 * r + 3) {
    status = kStartOutside;
    return;
  }
  const int L = o.levels;
  const float top = 1.f / (float)(1 << (L - 1));
  float nx = (has_guess ? gx : p0x) * top, ny = (has_guess ? gy : p0y) * top;
  uint32_t tI[P::kSlots], tD[P::kSlots];  // I | x << 16 | y << 24; dIx (low int16) | dIy (high int16)
  for (int l = L - 1; l >= 0; --l) {
    if (l != L - 1) {
      nx = nx * 2.f;
      ny = ny * 2.f;
    }
    const float s = 1.f / (float)(1 << l);
    const int w = A.lv[l].w, h = A.lv[l].h;
    const uint8_t* Ia = A.base + A.lv[l].off;
    const uint8_t* Ib = B.base + B.lv[l].off;
    const Win wp = window(p0x * s, p0y * s, r, w, h);
    if (!wp.inside) {
      if (l == 0) {
        status = kStartOutside;
        return;
      }
      continue;
    }
    int s11 = 0, s12 = 0, s22 = 0;
    KLT_UNROLL
    for (int k = 0; k < P::kSlots; ++k) {
      const int p = P::first() + P::stride() * k;
      if (p < npix) {
        const int y = p / W, x = p - y * W;
        const int X = wp.ix + x, Y = wp.iy + y;
        int cx[4], v[4][4];
        KLT_UNROLL
        for (int i = 0; i < 4; ++i) cx[i] = reflect(X - 1 + i, w);
        KLT_UNROLL
        for (int j = 0; j < 4; ++j) {
          const uint8_t* row = Ia + (size_t)reflect(Y - 1 + j, h) * w;
          KLT_UNROLL
          for (int i = 0; i < 4; ++i) v[j][i] = row[cx[i]];
        }
        int gxv[2][2], gyv[2][2];  // [j][i]: the Scharr derivatives at tap (X + i, Y + j)
        KLT_UNROLL
        for (int j = 0; j < 2; ++j) {
          KLT_UNROLL
          for (int i = 0; i < 2; ++i) {
            gxv[j][i] = 3 * (v[j][i + 2] - v[j][i]) + 10 * (v[j + 1][i + 2] - v[j + 1][i]) +
                        3 * (v[j + 2][i + 2] - v[j + 2][i]);
            gyv[j][i] = 3 * (v[j + 2][i] - v[j][i]) + 10 * (v[j + 2][i + 1] - v[j][i + 1]) +
                        3 * (v[j + 2][i + 2] - v[j][i + 2]);
          }
        }
        const int iv = (wp.w00 * v[1][1] + wp.w01 * v[1][2] + wp.w10 * v[2][1] + wp.w11 * v[2][2] + 256) >> 9;
        const int dx = (wp.w00 * gxv[0][0] + wp.w01 * gxv[0][1] + wp.w10 * gxv[1][0] + wp.w11 * gxv[1][1] + 8192) >> 14;
        const int dy = (wp.w00 * gyv[0][0] + wp.w01 * gyv[0][1] + wp.w10 * gyv[1][0] + wp.w11 * gyv[1][1] + 8192) >> 14;
        tI[k] = (uint32_t)iv | (uint32_t)x << 16 | (uint32_t)y << 24;
        tD[k] = ((uint32_t)dx & 0xffffu) | (uint32_t)dy << 16;
        s11 += dx * dx;
        s12 += dx * dy;
        s22 += dy * dy;
      }
    }
    const Gram g = gram(P::sum(s11), P::sum(s12), P::sum(s22), r, o.min_eig);
    if (!g.ok) {
      if (l == 0) {
        status = kDegenerate;
        return;
      }
      continue;
    }
    Step prev{0.0, 0.0};
    for (int j = 0; j < o.max_iters; ++j) {
      const Win wn = window(nx, ny, r, w, h);
      if (!wn.inside) {
        if (l == 0) {
          status = kLeftImage;
          return;
        }
        break;
      }
      int b1 = 0, b2 = 0;
      KLT_UNROLL
      for (int k = 0; k < P::kSlots; ++k) {
        const int p = P::first() + P::stride() * k;
        if (p < npix) {
          const uint32_t ti = tI[k], td = tD[k];
          const uint8_t* q = Ib + (size_t)(wn.iy + (int)(ti >> 24)) * w + (wn.ix + (int)((ti >> 16) & 0xff));
          const int jv = (wn.w00 * q[0] + wn.w01 * q[1] + wn.w10 * q[w] + wn.w11 * q[w + 1] + 256) >> 9;
          const int diff = jv - (int)(ti & 0xffffu);
          b1 += diff * (int)(int16_t)(td & 0xffffu);
          b2 += diff * ((int32_t)td >> 16);
        }
      }
      const Step d = step(g, P::sum(b1), P::sum(b2));
      if (update(nx, ny, d, prev, j, o.eps)) break;
    }
    if (l == 0) {
      const Win wf = window(nx, ny, r, w, h);
      if (!wf.inside) {
        status = kLeftImage;
        return;
      }
      int e = 0;
      KLT_UNROLL
      for (int k = 0; k < P::kSlots; ++k) {
        const int p = P::first() + P::stride() * k;
        if (p < npix) {
          const uint32_t ti = tI[k];
          const uint8_t* q = Ib + (size_t)(wf.iy + (int)(ti >> 24)) * w + (wf.ix + (int)((ti >> 16) & 0xff));
          const int jv = (wf.w00 * q[0] + wf.w01 * q[1] + wf.w10 * q[w] + wf.w11 * q[w + 1] + 256) >> 9;
          const int diff = jv - (int)(ti & 0xffffu);
          e += diff < 0 ? -diff : diff;
        }
      }
      const float ev = (float)((double)P::sum(e) / (double)(32 * npix));
      if (o.max_err > 0.f && ev > o.max_err) {
        status = kErrAbove;
        return;
      }
      err = ev;
      outx = nx;
      outy = ny;
    }
  }
}

}  // namespace kltm
}  // namespace vo
