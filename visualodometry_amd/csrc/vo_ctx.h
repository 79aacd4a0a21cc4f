// vo_ctx: one HIP device + stream, the matcher workspace and the BA engine.
#pragma once

#include <memory>
#include <vector>

#include "vo_common.h"

namespace vo {

struct MatchWorkspace {
  DevBuf des;       // staging for host descriptors (des0 then des1)
  DevBuf q8;        // packed int8 (a - 128) descriptors, query then train
  DevBuf norms;     // int32 squared norms of the packed rows
  DevBuf colconst;  // uint32 per train column (see match.hip)
  DevBuf partial;   // per (split, row) top-2 partials
  DevBuf best;      // int32 (batch, n0) best train index or -1
  DevBuf rev;       // cross check: int32 (batch, n1) nearest query row of each train row
  DevBuf top2;      // int32 (n0, 2) + float (n0, 2)
  DevBuf pairs;     // int32 (n0, 2) compacted pairs + count
  DevBuf flag;      // uint32: == gen when this call's descriptors are not 0..255 integers
  DevBuf hbf;       // float path: bf16 images of both sides (match_bf16.hip)
  DevBuf fnorm;     // float path: |b'|^2 per train row, |a| per query row
  DevBuf fpart;     // float path: top-2 of A per (split, row), the sweeps' own split
  DevBuf bmax;      // float path: max |b| per batch entry (zero between calls)
  DevBuf cand;      // float path: candidate lists + counts
  DevBuf gate;      // gated matcher (match_gate.hip): pred, radius, kp1 staging, cell grid, owner keys, dist
  uint32_t gen = 0;        // generation tag of the current call
  int kind_hint = 0;        // VO_DESC_* (vo_match_hint)
  bool flag_fresh = true;   // flag not yet zeroed
};

// The matcher's cached query side (vo_match_knn2_ratio_dev / _q with a nonzero tag): the
// reference matches every frame against the same keyframe (vo.py:64-65), so the keyframe's
// packed int8 rows, norms and integer verdict are kept across calls.  Keyed on (tag, source
// pointer, n0, dim, device or host source); host sources also keep their float copy (the
// exact sweep and the float path read it).
struct MatchQueryCache {
  DevBuf des;    // host sources: the query's float32 rows on the device
  DevBuf q8;     // packed int8 (a - 128) rows (n0_pad x Dp)
  DevBuf norms;  // int32 squared norms
  DevBuf colconst;  // uint32 column constants (the cross check's reverse pass takes these rows as columns)
  DevBuf flag;   // [0] 1 = a value is not a 0..255 integer, [1] 1 = a value is not finite
  uint64_t tag = 0;
  const void* src = nullptr;
  int n0 = -1, dim = -1;
  bool device_src = false;
  bool valid = false;
};

// Triangulation workspace (tri.hip).
struct TriWorkspace {
  DevBuf stage;  // host-call staging: pts1, pts2, pts3d, mask
};

// PnP-RANSAC workspace (pnp.hip): RANSAC subsets cached per frame layout.
struct PnpWorkspace {
  DevBuf sub;     // int32 (batch, H, 5) subsets
  DevBuf off;     // int32 (batch + 1) frame offsets
  DevBuf models;  // double (batch, H, 16)
  DevBuf counts;  // int32 (batch, H)
  DevBuf need;    // int32 (batch): frames whose hypotheses past the first h1 are solved
  DevBuf stage;   // host-call staging: points, outputs
  HostBuf hstage; // its page-locked mirror: one upload and one download per host call
  std::vector<int32_t> offsets;  // layout the cached subsets were made for
  int H = 0;
  int last_h1 = 0;  // hypotheses solved for every frame by the last call (pnp_run)
};

// Essential-matrix workspace (essential.hip): RANSAC subsets cached per (n, max_iters).
struct EssWorkspace {
  DevBuf q;       // double (n, 4) normalised correspondences
  DevBuf sub;     // int32 (H, 5) subsets
  DevBuf models;  // double (H, 10, 9)
  DevBuf counts;  // int32 (H, 10) inlier counts, (H) model counts, the go-on flag
  DevBuf flags;   // uint8 (n, 4) recoverPose: point passes under candidate
  DevBuf stage;   // host-call staging: points, outputs
  HostBuf hstage; // its page-locked mirror
  int sub_n = -1, sub_H = -1;  // what the cached subsets were made for
};

// SIFT detection workspace (sift.hip): Gaussian and DoG pyramids of a batch.
struct SiftWorkspace {
  DevBuf g, d;     // float pyramids (pitched, all octaves)
  DevBuf img;      // host-call staging: the uint8 image
  DevBuf kp;       // host-call staging: keypoints + count
  DevBuf cand_ext; // packed 26-neighbour extrema awaiting refinement + their count
  DevBuf cand;     // detectAndCompute: refined extrema (float + int records, count)
  DevBuf okp;      // oriented keypoints (batch, capacity, 8 floats)
  DevBuf keys;     // uint64 sort keys in / out
  DevBuf vals;     // uint32 record indices in / out, then the selection
  DevBuf segs;     // int32 per-image counts, segment bounds, kept counts
  DevBuf sort_tmp; // rocprim temporary storage
  DevBuf out;      // host-call staging: keypoints, descriptors, count
  // The overlapped pyramid (sift_run): octave o + 1's down-sample and first levels on the
  // context stream while octave o's last two levels and its extrema test run on this one.
  hipStream_t side = nullptr;
  hipEvent_t side_ev[17] = {};  // per octave (its level n_layers done), then the join
  SiftWorkspace() = default;
  SiftWorkspace(const SiftWorkspace&) = delete;
  SiftWorkspace& operator=(const SiftWorkspace&) = delete;
  ~SiftWorkspace() {
    if (side) (void)hipStreamSynchronize(side);
    for (hipEvent_t e : side_ev)
      if (e) (void)hipEventDestroy(e);
    if (side) (void)hipStreamDestroy(side);
  }
};

// KLT tracker workspace (klt.hip): device pyramids (uint8 levels, concatenated and unpitched).
struct KltPyramid {
  DevBuf buf;
  uint64_t tag = 0;
  int h = -1, w = -1, levels = -1;  // levels: how many were built (L_eff)
  uint64_t used = 0;                // the workspace clock at the last use (LRU)
  bool valid = false;
};
constexpr int kKltCacheEntries = 4;
struct KltWorkspace {
  KltPyramid cache[kKltCacheEntries];  // pyramids of tagged images, keyed by (tag, h, w, levels)
  KltPyramid scratch[2];               // pyramids of this call's untagged images
  DevBuf pts;                          // host-call staging: pts0, pts1, err, status
  uint64_t clock = 0;
};

// Corner detector workspace (corners.hip).
struct CornerWorkspace {
  DevBuf img, mask;  // host-call staging: an untagged (or uncached) image, the mask
  DevBuf resp;       // float (h, w) response map
  DevBuf keys;       // uint64 candidate keys, unsorted then sorted
  DevBuf sort_tmp;   // rocprim temporary storage
  DevBuf xy;         // vo_corner_select: the caller's int32 (n, 2) coordinates
  DevBuf cand;       // per sorted candidate: x, y, id, response, state, next in its cell
  DevBuf grid;       // int32 list heads per cell: candidates, keep-away points
  DevBuf keep;       // keep-away points (n_keep, 2) and their next links
  DevBuf out;        // accepted corners: xy, response, id
  DevBuf ctl;        // control words (maximum, counts, rounds)
  int32_t stats[4] = {0, 0, 0, 0};  // the last call's candidates, rounds, accepted, cell side
};

// Steered BRIEF workspace (brief.hip).
struct BriefWorkspace {
  DevBuf img;  // host-call staging: an untagged (or uncached) image
  DevBuf pts;  // host-call staging: the points (n, 2)
  DevBuf out;  // descriptors (n, 8), bins (n), status (n)
};

// Hamming matcher workspace (match_hamming.hip).
struct HammingWorkspace {
  DevBuf des;      // host-call staging: des0 then des1
  DevBuf partial;  // uint64 keys: (slices, n0, 2) forward, then (slices, n1) reverse
  DevBuf top2;     // int32 (n0, 2) indices, (n0, 2) distances
  DevBuf best;     // int32 (n0): the kept train row or -1
  DevBuf pairs;    // int32 (n0, 2) compacted pairs + count
};

class BAEngine;   // ba_engine.hip
struct Comm;      // ba_comm.h (RCCL communicator or loopback group)

// Kernel ids of the event profiler (vo_profile_* in include/vo_hip.h).
enum KernelId {
  kKBaLin = 0, kKBaReduce, kKBaSolve, kKMatchPack, kKMatchI8, kKMatchF32, kKMatchMerge,
  kKTriangulate, kKPnpHyp, kKPnpScore, kKPnpFinal, kKSiftPyramid, kKSiftExtrema, kKSiftOrient, kKSiftSelect,
  kKSiftDesc, kKMatchRerank, kKPnpDecide, kKPnpHypTail, kKPnpScoreTail, kKEssHyp, kKEssScore, kKEssDecide, kKEssFinal,
  kKEssPose, kKCount
};

// HIP-event timing of individual kernels on the context stream (off by default).
struct Profiler {
  bool on = false;
  struct Rec { int id; hipEvent_t start, stop; };
  std::vector<Rec> recs;
  std::vector<hipEvent_t> pool;
  size_t used = 0;
  hipEvent_t get();
  void begin(hipStream_t st, int id);  // records a start event if on
  void end(hipStream_t st);            // records the matching stop event
  void read(double* ms, int64_t* counts);  // after a stream sync; clears the records
  ~Profiler();
};

}  // namespace vo

struct vo_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int num_cus = 0;
  vo::MatchWorkspace match;
  vo::MatchQueryCache match_q;
  vo::TriWorkspace tri;
  vo::PnpWorkspace pnp;
  vo::EssWorkspace ess;
  vo::SiftWorkspace sift;
  vo::KltWorkspace klt;
  vo::CornerWorkspace corners;
  vo::BriefWorkspace brief;
  vo::HammingWorkspace hamming;
  vo::Profiler prof;
  std::unique_ptr<vo::BAEngine> ba;
  std::unique_ptr<vo::Comm> comm;
  bool ba_split_reduce = false;  // test/tool switch (vo_ba_split_reduce): K2 never fused into K3
  int ba_drop_reducers = 0;      // test switch (vo_ba_testing_drop_reducers): fused launches short of reducers
  bool ba_no_split = false;      // test switch (vo_ba_testing_no_split): no split band layout at setup
  int pnp_group = 0;      // test switch (vo_pnp_testing_group): 0 auto, 1 lane groups, -1 one lane per hypothesis
  int pnp_split = 0;      // test/tool switch (vo_pnp_testing_split): 0 auto, -1 never, n > 0 first n hypotheses
  bool ba_no_chain = false;      // test switch (vo_ba_testing_no_chain): no K1 chained into the solve launch
  int ba_chain_poll = 0;         // tool switch (vo_ba_testing_chain_poll): publish word replicas, 0 the default
  bool ba_chain_stamps = false;  // tool switch (vo_ba_testing_chain_stamps): stamped builds chain and stamp the gate
  int ba_k1_variant = 0;  // test switch (vo_ba_testing_k1): -1 four-wave K1, n >= 1 one-wave K1 of n chunks per segment
  vo_ctx();
  ~vo_ctx();
};

namespace vo {
// Matcher entry points (match.hip).  match_run, match_mutual_batch: device arrays, asynchronous.
// match_host: host arrays (device descriptors with device_src), synchronous.
void match_run(vo_ctx* ctx, const float* d_des0, const float* d_des1, int batch, int n0,
               int n1, int dim, double ratio, int32_t* d_best, int32_t* d_idx2,
               float* d_dist2, const MatchQueryCache* qc = nullptr, int32_t* d_rev = nullptr);
void match_mutual_batch(vo_ctx* ctx, const float* d_des0, const float* d_des1, int batch, int n0, int n1, int dim,
                        double ratio, int32_t* d_best);
void match_host(vo_ctx* ctx, const float* des0, int n0, const float* des1, int n1, int dim,
                double ratio, int32_t* pairs, int32_t* count, int32_t* idx2, float* dist2, uint64_t q_tag = 0,
                bool device_src = false, bool mutual = false);
void compact_pairs(vo_ctx* ctx, const int32_t* d_best, int n0, int32_t* d_pairs,
                   int32_t* d_count);
// Projection-gated and segment-gated matcher (match_gate.hip): host arrays (device train rows and
// keypoints with dev), synchronous; the arguments are checked by the caller.
struct GateHostArgs {
  const float* query;   // (n0, qcols) the gate's per-query array
  int qcols;            // 2: predicted position (circular gate); 4: segment a, b (capsule gate)
  const float* radius;  // (n0) or null: radius0
  const float* kp1;     // (n1, 2)
  float radius0;
  int width, height;
  double ratio, max_dist;
  bool unique;
  bool dev;             // des1 and kp1 are device arrays
};
void match_gate_host(vo_ctx* ctx, const float* des0, int n0, const float* des1, int n1, int dim, const GateHostArgs& h,
                     int32_t* out_pairs, float* out_dist, int32_t* out_count);
// Triangulation (tri.hip).  tri_run: host matrices, device points, asynchronous.  triangulate_host:
// host arrays, synchronous; the arguments are checked by the caller.
void tri_run(vo_ctx* ctx, const double* P1, const double* P2, const double* T_cw2, const double* K,
             const float* d_pts1, const float* d_pts2, int n, double min_depth, double max_reproj_err,
             float* d_pts3d, uint8_t* d_mask);
void triangulate_host(vo_ctx* ctx, const double* P1, const double* P2, const double* T_cw2, const double* K,
                      const float* pts1, const float* pts2, int n, double min_depth, double max_reproj_err,
                      float* pts3d_out, uint8_t* mask_out);
// PnP-RANSAC (pnp.hip).  pnp_run: device points, host offsets and K, asynchronous.  pnp_ransac_host:
// host arrays, synchronous; the arguments are checked by the caller.
void pnp_run(vo_ctx* ctx, const float* d_X, const float* d_uv, const int32_t* offsets, int batch,
             const double* K, int iterations, double reproj_err, double confidence, double* d_pose,
             uint8_t* d_mask, int32_t* d_status);
void pnp_ransac_host(vo_ctx* ctx, const float* objpts, const float* imgpts, int n, const double* K, int iterations,
                     double reproj_err, double confidence, double* rvec_out, double* tvec_out, uint8_t* mask_out,
                     int32_t* success_out);
// The last pnp_run's split (test entry vo_pnp_testing_last_split): reads the frames' need flags back.
void pnp_last_split(vo_ctx* ctx, int* h1, int* tail_frames);
void pnp_subsets(int count, int iters, int32_t* out);
// Essential-matrix RANSAC and recoverPose (essential.hip): host arrays, synchronous.
void essential_ransac_host(vo_ctx* ctx, const float* pts1, const float* pts2, int n, const double* K, int max_iters,
                           double threshold, double prob, double* E_out, uint8_t* mask_out, int32_t* success_out,
                           int32_t* inliers_out);
void recover_pose_host(vo_ctx* ctx, const double* E, const float* pts1, const float* pts2, int n, const double* K,
                       double distance_thresh, double* R_out, double* t_out, uint8_t* mask_out, int32_t* good_out);
// KLT tracker (klt.hip): host arrays, synchronous; the arguments are checked by the caller.
void klt_track_host(vo_ctx* ctx, const uint8_t* img0, uint64_t tag0, const uint8_t* img1, uint64_t tag1, int h, int w,
                    const float* pts0, float* pts1, int n, const vo_klt_options* opt, uint8_t* status, float* err,
                    int32_t* n_tracked);
void klt_pyramid_host(vo_ctx* ctx, const uint8_t* img, int h, int w, int levels, uint8_t* out, int64_t cap,
                      int32_t* levels_out);
int klt_layout(int h, int w, int levels, int win_radius, int64_t* out, int n);
// Corner detector (corners.hip): host arrays, synchronous; the arguments are checked by the caller.
void good_features_host(vo_ctx* ctx, const uint8_t* img, uint64_t tag, int h, int w, const uint8_t* mask,
                        const float* keep, int n_keep, const vo_corner_options* opt, float* corners, float* resp,
                        int32_t* n_out);
void corner_response_host(vo_ctx* ctx, const uint8_t* img, int h, int w, int block_radius, float* out);
void corner_select_host(vo_ctx* ctx, const int32_t* xy, const float* resp, int n, const float* keep, int n_keep,
                        float min_distance, int max_corners, int32_t* out_idx, int32_t* n_out);
void corner_stats(vo_ctx* ctx, int32_t out[4]);
// Steered BRIEF (brief.hip): host arrays, synchronous; the arguments are checked by the caller.
void brief_describe_host(vo_ctx* ctx, const uint8_t* img, uint64_t tag, int h, int w, const float* pts, int n,
                         uint32_t* des_out, int32_t* bin_out, uint8_t* status_out);
void brief_pattern(int8_t* out, int32_t* dir_out);
// Hamming matcher (match_hamming.hip): host outputs, host or (dev) device rows, synchronous; the
// arguments are checked by the caller, n0 >= 1.
void match_hamming_host(vo_ctx* ctx, const uint32_t* des0, int n0, const uint32_t* des1, int n1, int words, double ratio,
                        int max_dist, bool mutual, bool dev, int32_t* out_pairs, int32_t* out_dist, int32_t* out_count,
                        int32_t* knn_idx, int32_t* knn_dist);
// SIFT detection (sift.hip).  sift_run: device images, device keypoint outputs (unsorted),
// asynchronous.  sift_detect_host (keypoints in OpenCV's order) and sift_pyramid_host: host
// arrays, synchronous; the arguments are checked by the caller.
void sift_run(vo_ctx* ctx, const uint8_t* d_img, int batch, int h, int w, double contrast, double edge,
              double sigma, int n_layers, int capacity, float* d_kpf, int32_t* d_kpi, int32_t* d_count,
              float** g_out, float** d_out, int64_t* layout);
void sift_detect_host(vo_ctx* ctx, const uint8_t* img, int h, int w, double contrast, double edge, double sigma,
                      int n_layers, int capacity, float* kp_f, int32_t* kp_i, int32_t* count);
void sift_pyramid_host(vo_ctx* ctx, const uint8_t* img, int h, int w, double sigma, int n_layers, float* g_out,
                       int64_t g_floats, float* d_out, int64_t d_floats);
int sift_layout(int h, int w, int n_layers, int64_t* out, int n);
// SIFT detectAndCompute (sift_desc.hip): sift_run's candidates, then orientation, filtering and
// descriptors.  _run: a device batch into the caller's device buffers, asynchronous.  _host: a
// host image, synchronous, the results copied to host arrays or (device_out) to the caller's
// device buffers; fn names the entry in the messages; the arguments are checked by the caller.
void sift_detect_and_compute_run(vo_ctx* ctx, const uint8_t* d_imgs, int batch, int h, int w, int nfeatures,
                                 double contrast, double edge, double sigma, int n_layers, int capacity,
                                 vo_sift_keypoint* d_kps, float* d_desc, int32_t* d_counts);
void sift_detect_and_compute_host(vo_ctx* ctx, const uint8_t* img, int h, int w, int nfeatures, double contrast,
                                  double edge, double sigma, int n_layers, int capacity, vo_sift_keypoint* kps,
                                  float* desc, int32_t* count, bool device_out, const char* fn);
// sift_describe's selection stage alone on host records (test entry vo_sift_testing_select).
void sift_testing_select(vo_ctx* ctx, const float* okp, const int32_t* counts, int batch, int cap_img, int nfeatures,
                         uint32_t* sel, int32_t* sel_count);
}  // namespace vo
