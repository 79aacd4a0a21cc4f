// Brute-force Hamming matching of binary descriptor rows on gfx950 (vo_match_hamming).
//
// The contract is include/vo_hip.h; the restatement is in tests/test_gpu_match_hamming.py.  Every
// distance is an integer and every choice is the minimum of a totally ordered key, so the results do
// not depend on the split or the tile below.
//   hamming_slice_kernel<W>  one thread per query row, its words in W registers (W the power of two
//                            at or above `words`, the rest zero).  gridDim.y splits the train rows
//                            into slices so that a few thousand queries fill the machine.  The
//                            workgroup stages a tile of kTile train rows in LDS (zero padded to W
//                            words); every lane then reads the same row (a broadcast, no bank
//                            conflict), takes xor + popcount and keeps its two smallest keys
//                            d << 32 | j, which are distinct because the j are.  Per (slice, query)
//                            the two keys go to `partial`, ~0 where the slice had fewer rows.
//                            The cross check runs the same kernel with the roles swapped: the
//                            smallest key of train row j is then d(i', j) << 32 | i'.
//   hamming_finish_kernel    one thread per query: merges the slices' keys into the top-2, writes
//                            them, applies the keep rule and (mutual) compares the reverse pass's
//                            smallest key of j1 with d1 << 32 | i.
//   compact_pairs (match.hip) the kept rows into ascending (query, train) pairs and their count.
// Bounds: a thread past nq loads zeros and stores nothing; a tile row r < rows <= kTile reads train
// row tj + r < j1 <= nt; LDS index r * W + w < kTile * W; partial index (slice * nq + i) * 2 + {0, 1}
// with slice < gridDim.y and i < nq; the reverse lookup's j1 < n1 comes from a key this call wrote.
#include <algorithm>
#include <climits>
#include <vector>

#include "vo_ctx.h"

namespace vo {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = 256;
constexpr int kMinSliceRows = 64;
constexpr int kMaxSlices = 64;
constexpr uint64_t kNoKey = ~0ull;

template <int W>
__global__ __launch_bounds__(kThreads) void hamming_slice_kernel(const uint32_t* __restrict__ q, int nq,
                                                                 const uint32_t* __restrict__ t, int nt, int words,
                                                                 int slice_rows, uint64_t* __restrict__ partial) {
  __shared__ uint32_t s_t[kTile * W];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * kThreads + tid;
  const int slice = blockIdx.y;
  const int j0 = min((int)((int64_t)slice * slice_rows), nt), j1 = min(j0 + slice_rows, nt);
  uint32_t a[W];
#pragma unroll
  for (int w = 0; w < W; ++w) a[w] = (i < nq && w < words) ? q[(size_t)i * words + w] : 0u;
  uint64_t k1 = kNoKey, k2 = kNoKey;
  for (int tj = j0; tj < j1; tj += kTile) {
    const int rows = min(kTile, j1 - tj);
    for (int e = tid; e < rows * W; e += kThreads) {
      const int r = e / W, w = e - r * W;
      s_t[e] = w < words ? t[(size_t)(tj + r) * words + w] : 0u;
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      int d = 0;
#pragma unroll
      for (int w = 0; w < W; ++w) d += __popc(a[w] ^ s_t[r * W + w]);
      const uint64_t key = (uint64_t)(uint32_t)d << 32 | (uint32_t)(tj + r);
      if (key < k1) {
        k2 = k1;
        k1 = key;
      } else if (key < k2) {
        k2 = key;
      }
    }
    __syncthreads();
  }
  if (i < nq) {
    partial[((size_t)slice * nq + i) * 2] = k1;
    partial[((size_t)slice * nq + i) * 2 + 1] = k2;
  }
}

__global__ __launch_bounds__(256) void hamming_finish_kernel(const uint64_t* __restrict__ fwd, int slices, int n0,
                                                             const uint64_t* __restrict__ rev, int rslices, int n1,
                                                             double ratio, int max_dist, int32_t* __restrict__ idx2,
                                                             int32_t* __restrict__ dist2, int32_t* __restrict__ best) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n0) return;
  uint64_t k1 = kNoKey, k2 = kNoKey;
  for (int s = 0; s < slices; ++s) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const uint64_t key = fwd[((size_t)s * n0 + i) * 2 + c];
      if (key < k1) {
        k2 = k1;
        k1 = key;
      } else if (key < k2) {
        k2 = key;
      }
    }
  }
  const int32_t d1 = (int32_t)(k1 >> 32), d2 = (int32_t)(k2 >> 32);
  const int32_t j1 = (int32_t)(uint32_t)k1, j2 = (int32_t)(uint32_t)k2;
  idx2[2 * (size_t)i] = k1 == kNoKey ? -1 : j1;
  idx2[2 * (size_t)i + 1] = k2 == kNoKey ? -1 : j2;
  dist2[2 * (size_t)i] = k1 == kNoKey ? INT_MAX : d1;
  dist2[2 * (size_t)i + 1] = k2 == kNoKey ? INT_MAX : d2;
  bool keep = k2 != kNoKey && (max_dist == 0 || d1 <= max_dist) && (double)d1 < ratio * (double)d2;
  if (keep && rev) {
    uint64_t r1 = kNoKey;
    for (int s = 0; s < rslices; ++s) {
      const uint64_t key = rev[((size_t)s * n1 + j1) * 2];
      r1 = key < r1 ? key : r1;
    }
    keep = r1 == ((uint64_t)(uint32_t)d1 << 32 | (uint32_t)i);
  }
  best[i] = keep ? j1 : -1;
}

// The number of train slices for `blocks` workgroups of queries: about two workgroups per CU,
// slices of at least kMinSliceRows rows.
int slice_count(const vo_ctx* ctx, int blocks, int nt) {
  const int want = ceil_div(2 * std::max(ctx->num_cus, 1), blocks);
  return std::max(1, std::min({want, ceil_div(nt, kMinSliceRows), kMaxSlices}));
}

void launch_slices(vo_ctx* ctx, const uint32_t* q, int nq, const uint32_t* t, int nt, int words, int slices,
                   uint64_t* partial) {
  const dim3 grid(ceil_div(nq, kThreads), slices), block(kThreads);
  const int slice_rows = ceil_div(nt, slices);
  hipStream_t s = ctx->stream;
  if (words <= 1)
    hipLaunchKernelGGL(hamming_slice_kernel<1>, grid, block, 0, s, q, nq, t, nt, words, slice_rows, partial);
  else if (words <= 2)
    hipLaunchKernelGGL(hamming_slice_kernel<2>, grid, block, 0, s, q, nq, t, nt, words, slice_rows, partial);
  else if (words <= 4)
    hipLaunchKernelGGL(hamming_slice_kernel<4>, grid, block, 0, s, q, nq, t, nt, words, slice_rows, partial);
  else if (words <= 8)
    hipLaunchKernelGGL(hamming_slice_kernel<8>, grid, block, 0, s, q, nq, t, nt, words, slice_rows, partial);
  else
    hipLaunchKernelGGL(hamming_slice_kernel<16>, grid, block, 0, s, q, nq, t, nt, words, slice_rows, partial);
  VO_HIP_CHECK(hipGetLastError());
}

}  // namespace

void match_hamming_host(vo_ctx* ctx, const uint32_t* des0, int n0, const uint32_t* des1, int n1, int words, double ratio,
                        int max_dist, bool mutual, bool dev, int32_t* out_pairs, int32_t* out_dist, int32_t* out_count,
                        int32_t* knn_idx, int32_t* knn_dist) {
  HammingWorkspace& ws = ctx->hamming;
  hipStream_t s = ctx->stream;
  const size_t b0 = (size_t)n0 * words * 4, b1 = (size_t)n1 * words * 4;
  const uint32_t *d0 = des0, *d1 = des1;
  if (!dev) {
    ws.des.reserve(b0 + b1);
    uint32_t* stage = ws.des.as<uint32_t>();
    VO_HIP_CHECK(hipMemcpyAsync(stage, des0, b0, hipMemcpyHostToDevice, s));
    VO_HIP_CHECK(hipMemcpyAsync(stage + (size_t)n0 * words, des1, b1, hipMemcpyHostToDevice, s));
    d0 = stage;
    d1 = stage + (size_t)n0 * words;
  }
  const int slices = slice_count(ctx, ceil_div(n0, kThreads), n1);
  const int rslices = mutual ? slice_count(ctx, ceil_div(n1, kThreads), n0) : 0;
  const size_t fkeys = (size_t)slices * n0 * 2, rkeys = (size_t)rslices * n1 * 2;
  ws.partial.reserve((fkeys + rkeys) * 8);
  uint64_t* d_fwd = ws.partial.as<uint64_t>();
  uint64_t* d_rev = mutual ? d_fwd + fkeys : nullptr;
  ws.top2.reserve((size_t)n0 * 16);
  ws.best.reserve((size_t)n0 * 4);
  ws.pairs.reserve((size_t)n0 * 8 + 16);
  int32_t* d_idx2 = ws.top2.as<int32_t>();
  int32_t* d_dist2 = d_idx2 + 2 * (size_t)n0;
  int32_t* d_pairs = ws.pairs.as<int32_t>();
  int32_t* d_count = d_pairs + 2 * (size_t)n0;

  launch_slices(ctx, d0, n0, d1, n1, words, slices, d_fwd);
  if (mutual) launch_slices(ctx, d1, n1, d0, n0, words, rslices, d_rev);
  hipLaunchKernelGGL(hamming_finish_kernel, dim3(ceil_div(n0, 256)), dim3(256), 0, s, d_fwd, slices, n0, d_rev,
                     rslices, n1, ratio, max_dist, d_idx2, d_dist2, ws.best.as<int32_t>());
  VO_HIP_CHECK(hipGetLastError());
  compact_pairs(ctx, ws.best.as<int32_t>(), n0, d_pairs, d_count);
  VO_HIP_CHECK(hipMemcpyAsync(out_count, d_count, 4, hipMemcpyDeviceToHost, s));
  VO_HIP_CHECK(hipMemcpyAsync(out_pairs, d_pairs, (size_t)n0 * 8, hipMemcpyDeviceToHost, s));
  std::vector<int32_t> top;  // out_dist is looked up in the top-2 distances
  int32_t* h_dist = knn_dist;
  if (knn_idx) VO_HIP_CHECK(hipMemcpyAsync(knn_idx, d_idx2, (size_t)n0 * 8, hipMemcpyDeviceToHost, s));
  if (out_dist && !knn_dist) {
    top.resize(2 * (size_t)n0);
    h_dist = top.data();
  }
  if (h_dist) VO_HIP_CHECK(hipMemcpyAsync(h_dist, d_dist2, (size_t)n0 * 8, hipMemcpyDeviceToHost, s));
  VO_HIP_CHECK(hipStreamSynchronize(s));
  if (out_dist)
    for (int k = 0; k < *out_count; ++k) out_dist[k] = h_dist[2 * (size_t)out_pairs[2 * k]];
}

}  // namespace vo
