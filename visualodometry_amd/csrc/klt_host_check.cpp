// Runs whole KLT tracks (klt_math.h: the pyramid, the track kernel's per-point sequence, the
// forward-backward verdict) on the host, for tests/test_klt_host_math.py to compare with
// tests/klt_ref.py without a GPU.  Diagnostic build only: never part of libvo_hip.so.
//   klt_host_check in.bin out.bin
// in:  int32 h, w, n, win_radius, levels, max_iters, flags; float eps, min_eig, fb_thresh, max_err;
//      uint8 img0[h][w], img1[h][w]; float pts0[n][2]; float guess[n][2] (read with VO_KLT_GUESS)
// out: float pts1[n][2]; float err[n]; uint8 status[n]; int32 L_eff; int64 bytes;
//      uint8 pyramid of img0 [bytes] (levels concatenated, unpitched)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "klt_math.h"

using namespace vo::kltm;

namespace {

// One caller per track: it holds every pixel of the template and its sums are the totals.
struct HostPolicy {
  static constexpr int kSlots = kMaxPixels;
  static int first() { return 0; }
  static int stride() { return 1; }
  static int64_t sum(int v) { return v; }
};

std::vector<uint8_t> build_pyramid(const std::vector<uint8_t>& img, const Level* lv, int L, int64_t bytes) {
  std::vector<uint8_t> p((size_t)bytes);
  std::copy(img.begin(), img.end(), p.begin());
  for (int l = 1; l < L; ++l)
    for (int y = 0; y < lv[l].h; ++y)
      for (int x = 0; x < lv[l].w; ++x)
        p[(size_t)lv[l].off + (size_t)y * lv[l].w + x] =
            pyr_down_pixel(p.data() + lv[l - 1].off, lv[l - 1].w, lv[l - 1].h, x, y);
  return p;
}

template <class T>
bool rd(FILE* f, T* p, size_t n) {
  return std::fread(p, sizeof(T), n, f) == n;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* fi = std::fopen(argv[1], "rb");
  if (!fi) return 2;
  int32_t hd[7];
  float fo[4];
  if (!rd(fi, hd, 7) || !rd(fi, fo, 4)) return 2;
  const int h = hd[0], w = hd[1], n = hd[2], r = hd[3], levels = hd[4], max_iters = hd[5], flags = hd[6];
  if (h < 1 || w < 1 || n < 0 || r < 1 || r > kMaxRadius || levels < 1 || levels > kMaxLevels) return 2;
  std::vector<uint8_t> img0((size_t)h * w), img1((size_t)h * w);
  std::vector<float> pts0((size_t)n * 2), guess((size_t)n * 2);
  if (!rd(fi, img0.data(), img0.size()) || !rd(fi, img1.data(), img1.size()) || !rd(fi, pts0.data(), pts0.size()) ||
      !rd(fi, guess.data(), guess.size()))
    return 2;
  std::fclose(fi);

  Pyr A, B;
  int L = 1;
  const int64_t bytes = layout(h, w, levels, r, A.lv, &L);
  for (int l = 0; l < kMaxLevels; ++l) B.lv[l] = A.lv[l];
  const std::vector<uint8_t> pa = build_pyramid(img0, A.lv, L, bytes), pb = build_pyramid(img1, A.lv, L, bytes);
  A.base = pa.data();
  B.base = pb.data();
  const Options o{r, L, max_iters, fo[0], fo[1], fo[3]};

  std::vector<float> pts1((size_t)n * 2), err(n);
  std::vector<uint8_t> status(n);
  for (int i = 0; i < n; ++i) {
    const float px = pts0[2 * (size_t)i], py = pts0[2 * (size_t)i + 1];
    float x, y, e;
    uint8_t st;
    track_point<HostPolicy>(A, B, o, px, py, (flags & 1) != 0, guess[2 * (size_t)i], guess[2 * (size_t)i + 1], x, y,
                            st, e);
    if (st == kTracked && (flags & 2)) {  // the back track: roles swapped, the start as the guess
      float bx, by, be;
      uint8_t bs;
      track_point<HostPolicy>(B, A, o, x, y, true, px, py, bx, by, bs, be);
      if (fb_fails(bs, bx, by, px, py, fo[2])) {
        st = kFbFailed;
        x = px;
        y = py;
        e = 0.f;
      }
    }
    pts1[2 * (size_t)i] = x;
    pts1[2 * (size_t)i + 1] = y;
    err[i] = e;
    status[i] = st;
  }

  FILE* fw = std::fopen(argv[2], "wb");
  if (!fw) return 2;
  const int32_t l_eff = L;
  std::fwrite(pts1.data(), 4, pts1.size(), fw);
  std::fwrite(err.data(), 4, err.size(), fw);
  std::fwrite(status.data(), 1, status.size(), fw);
  std::fwrite(&l_eff, 4, 1, fw);
  std::fwrite(&bytes, 8, 1, fw);
  std::fwrite(pa.data(), 1, pa.size(), fw);
  std::fclose(fw);
  return 0;
}
