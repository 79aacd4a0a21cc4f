// Runs the steered BRIEF descriptor (brief_math.h: status, patch, moments, bin, box sums, bits) on
// the host, for tests/test_brief_host_math.py to compare with tests/brief_ref.py without a GPU.
// Diagnostic build only: never part of libvo_hip.so.
//   brief_host_check in.bin out.bin
// in:  int32 h, w, n; uint8 img[h][w]; float pts[n][2]
// out: uint32 des[n][8]; int32 bin[n]; uint8 status[n]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "brief_math.h"

using namespace vo::briefm;

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
  int32_t hd[3];
  if (!rd(fi, hd, 3)) return 2;
  const int h = hd[0], w = hd[1], n = hd[2];
  if (h < 1 || w < 1 || n < 0 || (int64_t)h * w > (int64_t)1 << 30) return 2;
  std::vector<uint8_t> img((size_t)h * w);
  std::vector<float> pts((size_t)n * 2);
  if (!rd(fi, img.data(), img.size()) || !rd(fi, pts.data(), pts.size())) return 2;
  std::fclose(fi);

  std::vector<uint32_t> des((size_t)n * kWords);
  std::vector<int32_t> bins((size_t)n);
  std::vector<uint8_t> status((size_t)n);
  for (int i = 0; i < n; ++i)
    status[i] = describe_point(img.data(), h, w, pts[2 * (size_t)i], pts[2 * (size_t)i + 1], &des[(size_t)i * kWords],
                               bins[i]);

  FILE* fw = std::fopen(argv[2], "wb");
  if (!fw) return 2;
  std::fwrite(des.data(), 4, des.size(), fw);
  std::fwrite(bins.data(), 4, bins.size(), fw);
  std::fwrite(status.data(), 1, status.size(), fw);
  std::fclose(fw);
  return 0;
}
