// Runs the corner detector (corners_math.h: gradients, block sums, response, candidate test, keys,
// the sequential selection) on the host, for tests/test_corners_host_math.py to compare with
// tests/corners_ref.py without a GPU.  Diagnostic build only: never part of libvo_hip.so.
//   corners_host_check in.bin out.bin
// in:  int32 h, w, block_radius, max_corners, n_keep, has_mask; float quality, min_distance;
//      uint8 img[h][w]; uint8 mask[h][w] (has_mask); float keep[n_keep][2]
// out: float resp[h][w]; int32 n_candidates, n; float corners[n][2]; float corner_resp[n]
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "corners_math.h"

using namespace vo::cornm;

namespace {

template <class T>
bool rd(FILE* f, T* p, size_t n) {
  return n == 0 || std::fread(p, sizeof(T), n, f) == n;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* fi = std::fopen(argv[1], "rb");
  if (!fi) return 2;
  int32_t hd[6];
  float fo[2];
  if (!rd(fi, hd, 6) || !rd(fi, fo, 2)) return 2;
  const int h = hd[0], w = hd[1], k = hd[2], max_corners = hd[3], n_keep = hd[4], has_mask = hd[5];
  const float quality = fo[0], dist = fo[1];
  if (h < 1 || w < 1 || k < 1 || k > kMaxBlockRadius || n_keep < 0 || max_corners < 1) return 2;
  const size_t npix = (size_t)h * w;
  std::vector<uint8_t> img(npix), mask(has_mask ? npix : 0);
  std::vector<float> keep((size_t)n_keep * 2);
  if (!rd(fi, img.data(), npix) || !rd(fi, mask.data(), mask.size()) || !rd(fi, keep.data(), keep.size())) return 2;
  std::fclose(fi);

  // the gradient field, then per pixel the block sums over it at reflected indices
  std::vector<int32_t> gx(npix), gy(npix);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      int a, b;
      sobel_at(img.data(), w, h, x, y, a, b);
      gx[(size_t)y * w + x] = a;
      gy[(size_t)y * w + x] = b;
    }
  std::vector<float> resp(npix);
  uint32_t rmax_bits = 0;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      int32_t a = 0, b = 0, c = 0;
      for (int j = -k; j <= k; ++j)
        for (int i = -k; i <= k; ++i) {
          const size_t p = (size_t)reflect(y + j, h) * w + reflect(x + i, w);
          a += gx[p] * gx[p];
          b += gx[p] * gy[p];
          c += gy[p] * gy[p];
        }
      const float r = response(a, b, c);
      resp[(size_t)y * w + x] = r;
      if (!has_mask || mask[(size_t)y * w + x]) rmax_bits = std::max(rmax_bits, max_domain(r));
    }
  const float rmax = bits_float(rmax_bits);

  std::vector<uint64_t> keys;
  if (rmax > 0.f && h >= 3 && w >= 3)
    for (int y = 1; y <= h - 2; ++y)
      for (int x = 1; x <= w - 2; ++x) {
        const size_t p = (size_t)y * w + x;
        const float r = resp[p];
        if ((has_mask && !mask[p]) || !above_threshold(r, quality, rmax)) continue;
        bool peak = true;
        for (int j = -1; j <= 1; ++j)
          for (int i = -1; i <= 1; ++i) peak = peak && r >= resp[p + (ptrdiff_t)j * w + i];
        if (peak) keys.push_back(candidate_key(r, (uint32_t)p));
      }
  std::sort(keys.begin(), keys.end());

  const double d2 = distance2(dist);
  std::vector<float> out_xy, out_r;
  std::vector<int> ax, ay;
  for (uint64_t key : keys) {
    if ((int)ax.size() >= max_corners) break;
    const uint32_t p = (uint32_t)key;
    const int x = (int)(p % (uint32_t)w), y = (int)(p / (uint32_t)w);
    bool rejected = false;
    for (int j = 0; j < n_keep && !rejected; ++j) {
      const float kx = keep[2 * (size_t)j], ky = keep[2 * (size_t)j + 1];
      rejected = finite32(kx) && finite32(ky) && keep_rejects(x, y, kx, ky, d2);
    }
    for (size_t j = 0; j < ax.size() && !rejected; ++j) rejected = pair_rejects(x - ax[j], y - ay[j], d2);
    if (rejected) continue;
    ax.push_back(x);
    ay.push_back(y);
    out_xy.push_back((float)x);
    out_xy.push_back((float)y);
    out_r.push_back(key_response(key));
  }

  FILE* fw = std::fopen(argv[2], "wb");
  if (!fw) return 2;
  const int32_t counts[2] = {(int32_t)keys.size(), (int32_t)ax.size()};
  std::fwrite(resp.data(), 4, resp.size(), fw);
  std::fwrite(counts, 4, 2, fw);
  std::fwrite(out_xy.data(), 4, out_xy.size(), fw);
  std::fwrite(out_r.data(), 4, out_r.size(), fw);
  std::fclose(fw);
  return 0;
}
