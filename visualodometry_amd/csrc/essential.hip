// Essential-matrix RANSAC and recoverPose, the reference's initialisation step, on gfx950.
//
// Replaces cv2.findEssentialMat(uv_ref, uv_curr, K, method=RANSAC, prob, threshold) and
// cv2.recoverPose(E, uv_ref, uv_curr, K) at reference src/modules/vo.py:87-101.  The contract
//  is the restatement in tests/essential_ref.py; the scalar math is
// essential_math.h, compiled here without FMA contraction so the two agree to rounding.
//
// As in pnp.hip the RANSAC hypotheses are independent (the subsets come from cv::RNG((uint64)-1)
// alone), so they are solved and scored at once and the serial bookkeeping is replayed over the
// inlier counts afterwards:
//   ess_norm_kernel    pixels -> normalised coordinates, double, once per call;
//   ess_hyp_kernel     one lane per hypothesis: the five-point solver (0..10 models), its
//                      10 x 20 elimination matrix in LDS, one column of doubles per lane;
//   ess_score_kernel   one workgroup per hypothesis: Sampson error of every point under each of
//                      its models, inlier counts;
//   ess_decide_kernel  the replay over the first slice of hypotheses: does the loop go on?
//   ess_final_kernel   the whole replay, the best model's mask, E;
//   ess_pose_kernel    recoverPose: E's SVD and the four candidates once, one thread per
//                      (point, candidate) triangulation, counts, the first best candidate.
// The hypotheses past the first slice are solved and scored by a second pair of launches that
// return at once when the loop stopped inside the slice; the replay never reads a count past
// the iteration where the loop stops, so the result equals the full serial loop's.
#include <cstring>
#include <vector>

#include "essential_math.h"
#include "vo_ctx.h"

#pragma clang fp contract(off)

namespace vo {
namespace {

using namespace essm;
using pnpm::Cam;

struct EssArgs {
  const double* q;         // n x (x1, y1, x2, y2) normalised
  const int32_t* subsets;  // H x 5
  double* models;          // H x 10 x 9
  int32_t* nmodels;        // H
  int32_t* counts;         // H x 10
  double* E;               // 9
  uint8_t* mask;           // n
  int32_t* status;         // success, inliers
  int n, H;
  float thr;
  double prob;
};

// Hypotheses per ess_hyp workgroup: 200 doubles of LDS each, 50 KB per workgroup (160 KB per CU).
// A hypothesis is one long dependent chain, so the launch is latency bound: half-filled waves on
// more CUs cost nothing.
constexpr int kHypLanes = 32;
constexpr int kSlice = 64;         // hypotheses solved before the replay decides on the rest
constexpr int kScoreThreads = 256;
constexpr int kReplayChunk = 128;  // iterations whose counts the replay stages in LDS at a time
constexpr int kFinalThreads = 256;
constexpr int kPoseThreads = 512;

__global__ __launch_bounds__(256) void ess_norm_kernel(const float2* p1, const float2* p2, int n, Cam K, double* q) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float2 a = p1[i], b = p2[i];
  double x1, y1, x2, y2;
  normalise(a.x, a.y, K, x1, y1);
  normalise(b.x, b.y, K, x2, y2);
  q[4l * i] = x1;
  q[4l * i + 1] = y1;
  q[4l * i + 2] = x2;
  q[4l * i + 3] = y2;
}

// Hypotheses [h_lo, h_hi) (none when need is given and zero).
__global__ __launch_bounds__(kHypLanes) void ess_hyp_kernel(EssArgs a, int h_lo, int h_hi, const int32_t* need) {
  if (need && !*need) return;
  const int h = h_lo + blockIdx.x * kHypLanes + threadIdx.x;
  if (h >= h_hi) return;
  __shared__ double s_m[kElimDoubles * kHypLanes];
  double q1[kPts][2], q2[kPts][2];
#pragma unroll
  for (int p = 0; p < kPts; ++p) {
    const int i = a.subsets[(size_t)h * kPts + p];
    q1[p][0] = a.q[4l * i];
    q1[p][1] = a.q[4l * i + 1];
    q2[p][0] = a.q[4l * i + 2];
    q2[p][1] = a.q[4l * i + 3];
  }
  a.nmodels[h] = five_point(q1, q2, Col{s_m + threadIdx.x, kHypLanes}, a.models + (size_t)h * kMaxModels * 9);
}

// One workgroup per hypothesis of [h_lo, h_lo + gridDim.x): every thread takes its points
// through all the hypothesis' models (in LDS); any n.
__global__ __launch_bounds__(kScoreThreads) void ess_score_kernel(EssArgs a, int h_lo, const int32_t* need) {
  if (need && !*need) return;
  const int h = h_lo + blockIdx.x;
  const int nm = a.nmodels[h];  // uniform
  __shared__ int s_cnt[kMaxModels];
  __shared__ double s_E[kMaxModels * 9];
  if (threadIdx.x < kMaxModels) s_cnt[threadIdx.x] = 0;
  if ((int)threadIdx.x < 9 * nm) s_E[threadIdx.x] = a.models[(size_t)h * kMaxModels * 9 + threadIdx.x];
  __syncthreads();
  int cnt[kMaxModels];
#pragma unroll
  for (int m = 0; m < kMaxModels; ++m) cnt[m] = 0;
  for (int i = threadIdx.x; i < a.n; i += kScoreThreads) {
    const double x1 = a.q[4l * i], y1 = a.q[4l * i + 1], x2 = a.q[4l * i + 2], y2 = a.q[4l * i + 3];
#pragma unroll
    for (int m = 0; m < kMaxModels; ++m)
      if (m < nm) cnt[m] += sampson_f32(&s_E[9 * m], x1, y1, x2, y2) <= a.thr ? 1 : 0;
  }
#pragma unroll
  for (int m = 0; m < kMaxModels; ++m) {
    if (m < nm) {
      int v = cnt[m];
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
      if ((threadIdx.x & 63) == 0 && v) atomicAdd(&s_cnt[m], v);
    }
  }
  __syncthreads();
  if (threadIdx.x < kMaxModels) a.counts[(size_t)h * kMaxModels + threadIdx.x] = s_cnt[threadIdx.x];
}

// The replay over iterations [0, h_end), their counts staged in LDS a chunk at a time.  Every
// thread of the workgroup calls; on return every thread may read *s_rep.
__device__ void ess_replay(const EssArgs& a, int h_end, int* s_nm, int* s_cnt, Replay* s_rep) {
  const int T = blockDim.x, t = threadIdx.x;
  if (t == 0) *s_rep = replay_start(a.H);
  for (int base = 0; base < h_end; base += kReplayChunk) {
    __syncthreads();  // *s_rep written, the previous chunk consumed
    const int stop = min(min(s_rep->niters, h_end), base + kReplayChunk);  // niters only shrinks
    if (base >= stop) break;  // uniform
    for (int k = t; k < stop - base; k += T) s_nm[k] = a.nmodels[base + k];
    for (int k = t; k < (stop - base) * kMaxModels; k += T) s_cnt[k] = a.counts[(size_t)base * kMaxModels + k];
    __syncthreads();
    if (t == 0) {
      Replay r = *s_rep;
      replay_range(r, s_nm, s_cnt, base, stop, a.n, a.prob);
      *s_rep = r;
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(kReplayChunk) void ess_decide_kernel(EssArgs a, int h_end, int32_t* need) {
  __shared__ int s_nm[kReplayChunk], s_cnt[kReplayChunk * kMaxModels];
  __shared__ Replay s_rep;
  ess_replay(a, h_end, s_nm, s_cnt, &s_rep);
  if (threadIdx.x == 0) *need = s_rep.niters > h_end ? 1 : 0;
}

// exact: n == 5, the single hypothesis on all points; its first model, every point an inlier.
__global__ __launch_bounds__(kFinalThreads) void ess_final_kernel(EssArgs a, int exact) {
  __shared__ int s_nm[kReplayChunk], s_cnt[kReplayChunk * kMaxModels];
  __shared__ Replay s_rep;
  __shared__ double s_E[9];
  __shared__ int s_inl;
  const double* best = nullptr;  // uniform
  if (exact) {
    if (a.nmodels[0] > 0) best = a.models;
  } else {
    ess_replay(a, a.H, s_nm, s_cnt, &s_rep);
    if (s_rep.best_it >= 0) best = a.models + ((size_t)s_rep.best_it * kMaxModels + s_rep.best_m) * 9;
  }
  if (threadIdx.x < 9) s_E[threadIdx.x] = best ? best[threadIdx.x] : 0.0;
  if (threadIdx.x == 0) s_inl = 0;
  __syncthreads();
  int cnt = 0;
  for (int i = threadIdx.x; i < a.n; i += kFinalThreads) {
    bool in = false;
    if (best)
      in = exact || sampson_f32(s_E, a.q[4l * i], a.q[4l * i + 1], a.q[4l * i + 2], a.q[4l * i + 3]) <= a.thr;
    a.mask[i] = in ? 1 : 0;
    cnt += in ? 1 : 0;
  }
  if (cnt) atomicAdd(&s_inl, cnt);
  __syncthreads();
  if (threadIdx.x < 9) a.E[threadIdx.x] = s_E[threadIdx.x];
  if (threadIdx.x == 0) {
    a.status[0] = best ? 1 : 0;
    a.status[1] = s_inl;
  }
}

struct PoseArgs {
  const double* E;   // 9
  const double* q;   // n x 4
  uint8_t* flags;    // n x 4: point i passes under candidate c
  double* Rt;        // R (9), t (3)
  uint8_t* mask;     // n
  int32_t* good;
  int n;
  double dist;
};

// One workgroup: thread 0 decomposes E, then the (point, candidate) items go round the threads.
__global__ __launch_bounds__(kPoseThreads) void ess_pose_kernel(PoseArgs a) {
  __shared__ double s_R[2][9], s_t[2][3];
  __shared__ int s_cnt[4];
  if (threadIdx.x == 0) {
    double R1[9], R2[9], t[3];
    decompose_essential(a.E, R1, R2, t);
    for (int k = 0; k < 9; ++k) {
      s_R[0][k] = R1[k];
      s_R[1][k] = R2[k];
    }
    for (int k = 0; k < 3; ++k) {
      s_t[0][k] = t[k];
      s_t[1][k] = -t[k];
    }
  }
  if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  // candidate c: rotation c & 1, translation sign c >> 1 (a thread's c is fixed: 512 % 4 == 0)
  const int c = threadIdx.x & 3;
  double R[9], t[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = s_R[c & 1][k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = s_t[c >> 1][k];
  int cnt = 0;
  for (int i = threadIdx.x >> 2; i < a.n; i += kPoseThreads / 4) {
    const bool ok = cheirality(R, t, a.q[4l * i], a.q[4l * i + 1], a.q[4l * i + 2], a.q[4l * i + 3], a.dist);
    a.flags[4l * i + c] = ok ? 1 : 0;
    cnt += ok ? 1 : 0;
  }
  if (cnt) atomicAdd(&s_cnt[c], cnt);
  __syncthreads();  // the workgroup's flags (global) and counts are written
  int w = 0;
#pragma unroll
  for (int k = 1; k < 4; ++k) w = s_cnt[k] > s_cnt[w] ? k : w;
  for (int i = threadIdx.x; i < a.n; i += kPoseThreads) a.mask[i] = a.flags[4l * i + w];
  if (threadIdx.x < 9) a.Rt[threadIdx.x] = s_R[w & 1][threadIdx.x];
  if (threadIdx.x < 3) a.Rt[9 + threadIdx.x] = s_t[w >> 1][threadIdx.x];
  if (threadIdx.x == 0) *a.good = s_cnt[w];
}

Cam cam_of(const double* K) { return Cam{K[0], K[4], K[2], K[5]}; }

void normalise_points(vo_ctx* ctx, const float* d_p1, const float* d_p2, int n, const double* K) {
  EssWorkspace& ws = ctx->ess;
  ws.q.reserve((size_t)n * 4 * sizeof(double));
  hipLaunchKernelGGL(ess_norm_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, ctx->stream,
                     reinterpret_cast<const float2*>(d_p1), reinterpret_cast<const float2*>(d_p2), n, cam_of(K),
                     ws.q.as<double>());
  VO_HIP_CHECK(hipGetLastError());
}

// findEssentialMat on the normalised points in ws.q (n >= 5): d_E (9), d_mask (n), d_status (2).
void ess_ransac(vo_ctx* ctx, int n, const double* K, int max_iters, double threshold, double prob, double* d_E,
                uint8_t* d_mask, int32_t* d_status) {
  EssWorkspace& ws = ctx->ess;
  const bool exact = n == kPts;
  const int H = exact ? 1 : (max_iters > 1 ? max_iters : 1);
  VO_REQUIRE(H <= 65536, VO_ERR_ARG, "essential: max_iters %d > 65536", H);
  if (ws.sub_n != n || ws.sub_H != H) {  // the subsets depend on (n, H) alone
    std::vector<int32_t> sub((size_t)H * kPts);
    if (exact)
      for (int p = 0; p < kPts; ++p) sub[p] = p;
    else
      pnp_subsets(n, H, sub.data());
    ws.sub.reserve(sub.size() * sizeof(int32_t));
    VO_HIP_CHECK(hipMemcpyAsync(ws.sub.ptr, sub.data(), sub.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                                ctx->stream));
    VO_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // the host vector goes out of scope
    ws.sub_n = n;
    ws.sub_H = H;
  }
  ws.models.reserve((size_t)H * kMaxModels * 9 * sizeof(double));
  ws.counts.reserve(((size_t)H * (kMaxModels + 1) + 1) * sizeof(int32_t));
  EssArgs a;
  a.q = ws.q.as<double>();
  a.subsets = ws.sub.as<int32_t>();
  a.models = ws.models.as<double>();
  a.counts = ws.counts.as<int32_t>();
  a.nmodels = a.counts + (size_t)H * kMaxModels;
  int32_t* need = a.nmodels + H;
  a.E = d_E;
  a.mask = d_mask;
  a.status = d_status;
  a.n = n;
  a.H = H;
  a.thr = sampson_threshold(threshold, cam_of(K));
  a.prob = prob;
  hipStream_t s = ctx->stream;
  auto solve_and_score = [&](int h_lo, int h_hi, const int32_t* need_in) {
    ctx->prof.begin(s, kKEssHyp);
    hipLaunchKernelGGL(ess_hyp_kernel, dim3(ceil_div(h_hi - h_lo, kHypLanes)), dim3(kHypLanes), 0, s, a, h_lo, h_hi,
                       need_in);
    ctx->prof.end(s);
    VO_HIP_CHECK(hipGetLastError());
    if (exact) return;
    ctx->prof.begin(s, kKEssScore);
    hipLaunchKernelGGL(ess_score_kernel, dim3(h_hi - h_lo), dim3(kScoreThreads), 0, s, a, h_lo, need_in);
    ctx->prof.end(s);
    VO_HIP_CHECK(hipGetLastError());
  };
  const int h1 = H < kSlice ? H : kSlice;
  solve_and_score(0, h1, nullptr);
  if (h1 < H) {
    ctx->prof.begin(s, kKEssDecide);
    hipLaunchKernelGGL(ess_decide_kernel, dim3(1), dim3(kReplayChunk), 0, s, a, h1, need);
    ctx->prof.end(s);
    VO_HIP_CHECK(hipGetLastError());
    solve_and_score(h1, H, need);
  }
  ctx->prof.begin(s, kKEssFinal);
  hipLaunchKernelGGL(ess_final_kernel, dim3(1), dim3(kFinalThreads), 0, s, a, exact ? 1 : 0);
  ctx->prof.end(s);
  VO_HIP_CHECK(hipGetLastError());
}

// recoverPose on the normalised points in ws.q: d_Rt (R row-major, then t), d_mask (n), d_good.
void ess_pose(vo_ctx* ctx, const double* d_E, int n, double dist, double* d_Rt, uint8_t* d_mask, int32_t* d_good) {
  EssWorkspace& ws = ctx->ess;
  ws.flags.reserve((size_t)n * 4 + 16);
  PoseArgs p;
  p.E = d_E;
  p.q = ws.q.as<double>();
  p.flags = ws.flags.as<uint8_t>();
  p.Rt = d_Rt;
  p.mask = d_mask;
  p.good = d_good;
  p.n = n;
  p.dist = dist;
  ctx->prof.begin(ctx->stream, kKEssPose);
  hipLaunchKernelGGL(ess_pose_kernel, dim3(1), dim3(kPoseThreads), 0, ctx->stream, p);
  ctx->prof.end(ctx->stream);
  VO_HIP_CHECK(hipGetLastError());
}

// Staging layout of the host calls (device and page-locked mirror alike):
// p1 | p2 | E (9) Rt (12) status (4 x int32: success, inliers, good, 0) | mask (n) | pose mask (n)
struct Stage {
  size_t pts, out, total;
  char *dev, *host;
  float *d_p1, *d_p2;
  double *d_E, *d_Rt;
  int32_t* d_status;
  uint8_t *d_mask, *d_pmask;
  const double* h_out;
  const int32_t* h_status;
  const uint8_t *h_mask, *h_pmask;
};

Stage stage_for(vo_ctx* ctx, int n) {
  Stage st;
  st.pts = (size_t)n * 16;
  st.out = 21 * sizeof(double) + 16;
  st.total = st.pts + st.out + 2 * (size_t)n;
  ctx->ess.stage.reserve(st.total + 64);
  ctx->ess.hstage.reserve(st.total + 64);
  st.dev = ctx->ess.stage.as<char>();
  st.host = ctx->ess.hstage.as<char>();
  st.d_p1 = reinterpret_cast<float*>(st.dev);
  st.d_p2 = reinterpret_cast<float*>(st.dev + (size_t)n * 8);
  st.d_E = reinterpret_cast<double*>(st.dev + st.pts);
  st.d_Rt = st.d_E + 9;
  st.d_status = reinterpret_cast<int32_t*>(st.d_E + 21);
  st.d_mask = reinterpret_cast<uint8_t*>(st.dev + st.pts + st.out);
  st.d_pmask = st.d_mask + n;
  st.h_out = reinterpret_cast<const double*>(st.host + st.pts);
  st.h_status = reinterpret_cast<const int32_t*>(st.h_out + 21);
  st.h_mask = reinterpret_cast<const uint8_t*>(st.host + st.pts + st.out);
  st.h_pmask = st.h_mask + n;
  return st;
}

}  // namespace

void essential_ransac_host(vo_ctx* ctx, const float* pts1, const float* pts2, int n, const double* K, int max_iters,
                           double threshold, double prob, double* E_out, uint8_t* mask_out, int32_t* success_out,
                           int32_t* inliers_out) {
  VO_REQUIRE(prob > 0 && prob < 1, VO_ERR_ARG, "essential: prob %g not in (0, 1)", prob);
  VO_REQUIRE(threshold > 0, VO_ERR_ARG, "essential: threshold %g <= 0", threshold);
  *success_out = 0;
  *inliers_out = 0;
  for (int k = 0; k < 9; ++k) E_out[k] = 0.0;
  if (n > 0) std::memset(mask_out, 0, (size_t)n);
  if (n < kPts) return;  // no model from fewer than five correspondences
  const Stage st = stage_for(ctx, n);
  hipStream_t s = ctx->stream;
  std::memcpy(st.host, pts1, (size_t)n * 8);
  std::memcpy(st.host + (size_t)n * 8, pts2, (size_t)n * 8);
  VO_HIP_CHECK(hipMemcpyAsync(st.dev, st.host, st.pts, hipMemcpyHostToDevice, s));
  normalise_points(ctx, st.d_p1, st.d_p2, n, K);
  ess_ransac(ctx, n, K, max_iters, threshold, prob, st.d_E, st.d_mask, st.d_status);
  VO_HIP_CHECK(hipMemcpyAsync(st.host + st.pts, st.dev + st.pts, st.out + (size_t)n, hipMemcpyDeviceToHost, s));
  VO_HIP_CHECK(hipStreamSynchronize(s));
  for (int k = 0; k < 9; ++k) E_out[k] = st.h_out[k];
  std::memcpy(mask_out, st.h_mask, (size_t)n);
  *success_out = st.h_status[0];
  *inliers_out = st.h_status[1];
}

void recover_pose_host(vo_ctx* ctx, const double* E, const float* pts1, const float* pts2, int n, const double* K,
                       double distance_thresh, double* R_out, double* t_out, uint8_t* mask_out, int32_t* good_out) {
  const Stage st = stage_for(ctx, n);
  hipStream_t s = ctx->stream;
  if (n > 0) {
    std::memcpy(st.host, pts1, (size_t)n * 8);
    std::memcpy(st.host + (size_t)n * 8, pts2, (size_t)n * 8);
  }
  std::memcpy(st.host + st.pts, E, 9 * sizeof(double));
  VO_HIP_CHECK(hipMemcpyAsync(st.dev, st.host, st.pts + 9 * sizeof(double), hipMemcpyHostToDevice, s));
  if (n > 0) normalise_points(ctx, st.d_p1, st.d_p2, n, K);
  ess_pose(ctx, st.d_E, n, distance_thresh, st.d_Rt, st.d_pmask, st.d_status + 2);
  VO_HIP_CHECK(hipMemcpyAsync(st.host + st.pts, st.dev + st.pts, st.total - st.pts, hipMemcpyDeviceToHost, s));
  VO_HIP_CHECK(hipStreamSynchronize(s));
  for (int k = 0; k < 9; ++k) R_out[k] = st.h_out[9 + k];
  for (int k = 0; k < 3; ++k) t_out[k] = st.h_out[18 + k];
  if (n > 0) std::memcpy(mask_out, st.h_pmask, (size_t)n);
  *good_out = st.h_status[2];
}

}  // namespace vo
