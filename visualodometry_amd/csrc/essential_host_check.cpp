// Runs the essential-matrix kernels' scalar math (essential_math.h) on the host, for
// tests/test_essential_host_math.py to compare with tests/essential_ref.py without a GPU.
// Diagnostic build only: never part of libvo_hip.so.
//   essential_host_check models in.bin out.bin   per subset (what ess_hyp_kernel computes)
// in:  int32 count, double K[4] (fu, fv, uc, vc), then count x (p1[5][2], p2[5][2]) float32 pixels
// out: count x (number of models, 10 x E[9]) doubles, unused models zero
//   essential_host_check full in.bin out.bin     one call through the kernels' logic:
//                                                findEssentialMat, then recoverPose on its E
// in:  int32 n, int32 H, double K[4], double threshold, double prob, double distance_thresh,
//      float p1[n][2], float p2[n][2], int32 subsets[H][5]
// out: double E[9], R[9], t[3], int32 success, inliers, good, 0, uint8 mask[n], uint8 pose_mask[n]
//   essential_host_check pose in.bin out.bin     recoverPose on a given E
// in:  int32 n, double K[4], double distance_thresh, double E[9], float p1[n][2], float p2[n][2]
// out: double R[9], t[3], int32 good, 0, uint8 pose_mask[n]
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "essential_math.h"

using namespace vo::essm;
using vo::pnpm::Cam;

namespace {

struct Pose {
  double R[9], t[3];
  int good;
  std::vector<uint8_t> mask;
};

// ess_pose_kernel: the four candidates in the order [R1|t] [R2|t] [R1|-t] [R2|-t], the first
// with the most points passing.
Pose recover_pose(const double* E, const std::vector<double>& q, int n, double dist) {
  double R1[9], R2[9], t[3], tn[3];
  decompose_essential(E, R1, R2, t);
  for (int k = 0; k < 3; ++k) tn[k] = -t[k];
  const double* Rc[4] = {R1, R2, R1, R2};
  const double* tc[4] = {t, t, tn, tn};
  std::vector<uint8_t> flags((size_t)4 * n, 0);
  int cnt[4] = {0, 0, 0, 0};
  for (int i = 0; i < n; ++i)
    for (int c = 0; c < 4; ++c) {
      flags[4 * (size_t)i + c] = cheirality(Rc[c], tc[c], q[4 * (size_t)i], q[4 * (size_t)i + 1],
                                            q[4 * (size_t)i + 2], q[4 * (size_t)i + 3], dist);
      cnt[c] += flags[4 * (size_t)i + c];
    }
  int w = 0;
  for (int c = 1; c < 4; ++c)
    if (cnt[c] > cnt[w]) w = c;
  Pose p;
  for (int k = 0; k < 9; ++k) p.R[k] = Rc[w][k];
  for (int k = 0; k < 3; ++k) p.t[k] = tc[w][k];
  p.good = cnt[w];
  p.mask.resize(n);
  for (int i = 0; i < n; ++i) p.mask[i] = flags[4 * (size_t)i + w];
  return p;
}

std::vector<double> normalised(const std::vector<float>& p1, const std::vector<float>& p2, int n, const Cam& K) {
  std::vector<double> q((size_t)4 * n);
  for (int i = 0; i < n; ++i) {
    normalise(p1[2 * (size_t)i], p1[2 * (size_t)i + 1], K, q[4 * (size_t)i], q[4 * (size_t)i + 1]);
    normalise(p2[2 * (size_t)i], p2[2 * (size_t)i + 1], K, q[4 * (size_t)i + 2], q[4 * (size_t)i + 3]);
  }
  return q;
}

int solve_subset(const std::vector<double>& q, const int32_t* idx, double* models) {
  double q1[kPts][2], q2[kPts][2], work[kElimDoubles];
  for (int p = 0; p < kPts; ++p) {
    const double* s = &q[4 * (size_t)idx[p]];
    q1[p][0] = s[0];
    q1[p][1] = s[1];
    q2[p][0] = s[2];
    q2[p][1] = s[3];
  }
  return five_point(q1, q2, Col{work, 1}, models);
}

int run_models(const char* in_path, const char* out_path) {
  FILE* fi = std::fopen(in_path, "rb");
  if (!fi) return 2;
  int count = 0;
  double k[4];
  if (std::fread(&count, 4, 1, fi) != 1 || std::fread(k, 8, 4, fi) != 4) return 2;
  std::vector<float> in((size_t)count * 20);
  if (std::fread(in.data(), 4, in.size(), fi) != in.size()) return 2;
  std::fclose(fi);
  const Cam K{k[0], k[1], k[2], k[3]};
  std::vector<double> out((size_t)count * 91, 0.0);
  const int32_t idx[kPts] = {0, 1, 2, 3, 4};
  for (int h = 0; h < count; ++h) {
    std::vector<float> p1(in.begin() + 20 * (size_t)h, in.begin() + 20 * (size_t)h + 10);
    std::vector<float> p2(in.begin() + 20 * (size_t)h + 10, in.begin() + 20 * (size_t)h + 20);
    const std::vector<double> q = normalised(p1, p2, kPts, K);
    out[91 * (size_t)h] = solve_subset(q, idx, &out[91 * (size_t)h + 1]);
  }
  FILE* fo = std::fopen(out_path, "wb");
  if (!fo) return 2;
  std::fwrite(out.data(), 8, out.size(), fo);
  std::fclose(fo);
  return 0;
}

int run_pose(const char* in_path, const char* out_path) {
  FILE* fi = std::fopen(in_path, "rb");
  if (!fi) return 2;
  int n = 0;
  double k[4], dist = 0, E[9];
  if (std::fread(&n, 4, 1, fi) != 1 || std::fread(k, 8, 4, fi) != 4 || std::fread(&dist, 8, 1, fi) != 1 ||
      std::fread(E, 8, 9, fi) != 9)
    return 2;
  std::vector<float> p1((size_t)2 * n), p2((size_t)2 * n);
  if (std::fread(p1.data(), 4, p1.size(), fi) != p1.size() || std::fread(p2.data(), 4, p2.size(), fi) != p2.size())
    return 2;
  std::fclose(fi);
  const Cam K{k[0], k[1], k[2], k[3]};
  const Pose p = recover_pose(E, normalised(p1, p2, n, K), n, dist);
  const int32_t st[2] = {p.good, 0};
  FILE* fo = std::fopen(out_path, "wb");
  if (!fo) return 2;
  std::fwrite(p.R, 8, 9, fo);
  std::fwrite(p.t, 8, 3, fo);
  std::fwrite(st, 4, 2, fo);
  std::fwrite(p.mask.data(), 1, p.mask.size(), fo);
  std::fclose(fo);
  return 0;
}

int run_full(const char* in_path, const char* out_path) {
  FILE* fi = std::fopen(in_path, "rb");
  if (!fi) return 2;
  int n = 0, H = 0;
  double k[4], threshold = 0, prob = 0, dist = 0;
  if (std::fread(&n, 4, 1, fi) != 1 || std::fread(&H, 4, 1, fi) != 1 || std::fread(k, 8, 4, fi) != 4 ||
      std::fread(&threshold, 8, 1, fi) != 1 || std::fread(&prob, 8, 1, fi) != 1 || std::fread(&dist, 8, 1, fi) != 1)
    return 2;
  std::vector<float> p1((size_t)2 * n), p2((size_t)2 * n);
  std::vector<int32_t> sub((size_t)kPts * H);
  if (std::fread(p1.data(), 4, p1.size(), fi) != p1.size() || std::fread(p2.data(), 4, p2.size(), fi) != p2.size() ||
      std::fread(sub.data(), 4, sub.size(), fi) != sub.size())
    return 2;
  std::fclose(fi);
  const Cam K{k[0], k[1], k[2], k[3]};
  const float thr = sampson_threshold(threshold, K);
  const std::vector<double> q = normalised(p1, p2, n, K);
  // ess_hyp_kernel + ess_score_kernel
  const int nh = n == kPts ? 1 : (n > kPts ? H : 0);
  std::vector<double> models((size_t)90 * (nh ? nh : 1), 0.0);
  std::vector<int> nmodels(nh ? nh : 1, 0), counts((size_t)kMaxModels * (nh ? nh : 1), 0);
  const int32_t all[kPts] = {0, 1, 2, 3, 4};
  for (int h = 0; h < nh; ++h) {
    nmodels[h] = solve_subset(q, n == kPts ? all : &sub[kPts * (size_t)h], &models[90 * (size_t)h]);
    if (n > kPts)
      for (int m = 0; m < nmodels[h]; ++m)
        for (int i = 0; i < n; ++i)
          counts[kMaxModels * (size_t)h + m] +=
              sampson_f32(&models[90 * (size_t)h + 9 * m], q[4 * (size_t)i], q[4 * (size_t)i + 1],
                          q[4 * (size_t)i + 2], q[4 * (size_t)i + 3]) <= thr;
  }
  // ess_final_kernel
  const double* best = nullptr;
  if (n == kPts) {
    if (nmodels[0] > 0) best = &models[0];
  } else if (n > kPts) {
    Replay r = replay_start(H);
    replay_range(r, nmodels.data(), counts.data(), 0, H, n, prob);
    if (r.best_it >= 0) best = &models[90 * (size_t)r.best_it + 9 * r.best_m];
  }
  double E[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  int32_t st[4] = {0, 0, 0, 0};
  std::vector<uint8_t> mask(n, 0);
  Pose pose;
  pose.good = 0;
  pose.mask.assign(n, 0);
  for (int e = 0; e < 9; ++e) pose.R[e] = 0.0;
  for (int e = 0; e < 3; ++e) pose.t[e] = 0.0;
  if (best) {
    for (int e = 0; e < 9; ++e) E[e] = best[e];
    for (int i = 0; i < n; ++i) {
      mask[i] = n == kPts ? 1
                          : sampson_f32(best, q[4 * (size_t)i], q[4 * (size_t)i + 1], q[4 * (size_t)i + 2],
                                        q[4 * (size_t)i + 3]) <= thr;
      st[1] += mask[i];
    }
    st[0] = 1;
    pose = recover_pose(E, q, n, dist);
    st[2] = pose.good;
  }
  FILE* fo = std::fopen(out_path, "wb");
  if (!fo) return 2;
  std::fwrite(E, 8, 9, fo);
  std::fwrite(pose.R, 8, 9, fo);
  std::fwrite(pose.t, 8, 3, fo);
  std::fwrite(st, 4, 4, fo);
  std::fwrite(mask.data(), 1, mask.size(), fo);
  std::fwrite(pose.mask.data(), 1, pose.mask.size(), fo);
  std::fclose(fo);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && std::string(argv[1]) == "models") return run_models(argv[2], argv[3]);
  if (argc == 4 && std::string(argv[1]) == "full") return run_full(argv[2], argv[3]);
  if (argc == 4 && std::string(argv[1]) == "pose") return run_pose(argv[2], argv[3]);
  std::fprintf(stderr, "usage: %s models|full|pose in.bin out.bin\n", argv[0]);
  return 2;
}
