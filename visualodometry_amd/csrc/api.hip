// extern "C" entry points of libvo_hip.so (declared in include/vo_hip.h).
#include <cstdarg>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "ba_band.h"
#include "ba_comm.h"
#include "ba_engine.h"
#include "ba_plan.h"
#include "ba_tables.h"
#include "vo_ctx.h"
#include "../../include/vo_hip_testing.h"
#include "../../include/vo_hip_testing_chain.h"

namespace vo {

namespace {
thread_local std::string g_err;
}

void set_error(const char* f, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, f);
  std::vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  g_err = buf;
}
const char* last_error() { return g_err.c_str(); }

hipEvent_t Profiler::get() {
  if (used == pool.size()) {
    hipEvent_t e;
    VO_HIP_CHECK(hipEventCreate(&e));
    pool.push_back(e);
  }
  return pool[used++];
}

void Profiler::begin(hipStream_t st, int id) {
  if (!on) return;
  Rec r{id, get(), get()};
  VO_HIP_CHECK(hipEventRecord(r.start, st));
  recs.push_back(r);
}

void Profiler::end(hipStream_t st) {
  if (!on || recs.empty()) return;
  VO_HIP_CHECK(hipEventRecord(recs.back().stop, st));
}

static_assert(kKCount == VO_PROFILE_KERNELS, "profiler ids match include/vo_hip.h");

void Profiler::read(double* ms, int64_t* counts) {
  for (int k = 0; k < kKCount; ++k) {
    ms[k] = 0.0;
    counts[k] = 0;
  }
  for (const Rec& r : recs) {
    float t = 0.0f;
    VO_HIP_CHECK(hipEventElapsedTime(&t, r.start, r.stop));
    ms[r.id] += t;
    counts[r.id] += 1;
  }
  recs.clear();
  used = 0;
}

Profiler::~Profiler() {
  for (hipEvent_t e : pool) (void)hipEventDestroy(e);
}

namespace {

void bind(vo_ctx* ctx) {
  VO_REQUIRE(ctx, VO_ERR_ARG, "null vo_ctx");
  VO_HIP_CHECK(hipSetDevice(ctx->device));
}

// A caller's device pointer must be device memory of the context's GPU, known to this HIP runtime,
// whose allocation covers [p, p + bytes).
void check_device_range(vo_ctx* ctx, const void* p, size_t bytes, const char* what) {
  if (bytes == 0) return;
  VO_REQUIRE(p != nullptr, VO_ERR_ARG, "%s: null device pointer", what);
  hipPointerAttribute_t at{};
  const hipError_t e = hipPointerGetAttributes(&at, p);
  if (e != hipSuccess) (void)hipGetLastError();
  VO_REQUIRE(e == hipSuccess && at.type == hipMemoryTypeDevice && at.device == ctx->device, VO_ERR_ARG,
             "%s: not device memory of device %d in this process's HIP runtime", what, ctx->device);
  void* base = nullptr;
  size_t size = 0;
  const hipError_t e2 = hipMemGetAddressRange(&base, &size, const_cast<void*>(p));
  if (e2 != hipSuccess) (void)hipGetLastError();
  VO_REQUIRE(e2 == hipSuccess && (const char*)p + bytes <= (const char*)base + size, VO_ERR_ARG,
             "%s: %zu bytes past its allocation", what, bytes);
}

}  // namespace
}  // namespace vo

using vo::guarded;

// A vo_ba_* call on a session: bind, the caller's argument check (arg_error: its message, null if
// the arguments are fine), the session check, then f, whose return code (if it has one) is the
// call's unless something threw.
template <class F>
static int ba_call(vo_ctx* ctx, uint64_t session, F&& f, const char* arg_error = nullptr) {
  int rc = VO_OK;
  const int g = guarded([&] {
    vo::bind(ctx);
    VO_REQUIRE(!arg_error, VO_ERR_ARG, "%s", arg_error);
    vo::ba_check_session(ctx, session);
    if constexpr (std::is_void_v<decltype(f())>) f();
    else rc = f();
  });
  return g != VO_OK ? g : rc;
}

// vo_match_gated and vo_match_segment: one contract but for the gate.  The checks of either
// entry's options struct (they need no device, nor a context) and the fields the two share; the
// entry adds its per-query array (pred: 2 floats a query, seg: 4).
template <class Options>
static vo::GateHostArgs gate_options(const char* fn, int n0, int n1, int dim, const Options* opt,
                                     const int32_t* out_pairs, const int32_t* out_count) {
  VO_REQUIRE(opt && out_pairs && out_count, VO_ERR_ARG, "%s: null options or outputs", fn);
  VO_REQUIRE(n0 >= 0 && n1 >= 0 && dim >= 1, VO_ERR_ARG, "%s: bad shape n0=%d n1=%d dim=%d", fn, n0, n1, dim);
  VO_REQUIRE((opt->flags & ~(VO_MATCH_DEVICE_PTRS | VO_MATCH_GATE_UNIQUE)) == 0, VO_ERR_ARG,
             "%s: unknown flags 0x%x", fn, opt->flags);
  VO_REQUIRE(opt->reserved == 0, VO_ERR_ARG, "%s: reserved must be 0", fn);
  VO_REQUIRE(std::isfinite(opt->ratio) && opt->ratio >= 0.0 && std::isfinite(opt->max_dist) && opt->max_dist >= 0.0,
             VO_ERR_ARG, "%s: ratio and max_dist must be finite and >= 0", fn);
  vo::GateHostArgs g{};
  g.radius = opt->radius;
  g.kp1 = opt->kp1;
  g.radius0 = opt->radius0;
  g.width = opt->width;
  g.height = opt->height;
  g.ratio = opt->ratio;
  g.max_dist = opt->max_dist;
  g.unique = (opt->flags & VO_MATCH_GATE_UNIQUE) != 0;
  g.dev = (opt->flags & VO_MATCH_DEVICE_PTRS) != 0;
  return g;
}

// The rest of the two entries: the arrays' checks, then the context and the device ranges.
static void gate_call(const char* fn, vo_ctx* ctx, const float* des0, int n0, const float* des1, int n1, int dim,
                      const vo::GateHostArgs& g, int32_t* out_pairs, float* out_dist, int32_t* out_count) {
  VO_REQUIRE((n0 == 0 || (des0 && g.query)) && (n1 == 0 || (des1 && g.kp1)), VO_ERR_ARG,
             "%s: null array with a nonzero size", fn);
  vo::bind(ctx);
  if (g.dev) {  // as vo_match_knn2_ratio_dev: refused before any launch
    vo::check_device_range(ctx, des1, (size_t)n1 * dim * 4, "des1");
    vo::check_device_range(ctx, g.kp1, (size_t)n1 * 8, "kp1");
  }
  *out_count = 0;
  if (n0 == 0 || n1 == 0) return;
  vo::match_gate_host(ctx, des0, n0, des1, n1, dim, g, out_pairs, out_dist, out_count);
}

extern "C" {

int vo_abi_version(void) { return VO_ABI_VERSION; }

const char* vo_last_error(void) { return vo::last_error(); }

vo_ctx* vo_create(int device, int flags) {
  (void)flags;
  vo_ctx* out = nullptr;
  int rc = guarded([&] {
    int n = 0;
    VO_HIP_CHECK(hipGetDeviceCount(&n));
    VO_REQUIRE(device >= 0 && device < n, VO_ERR_NODEV, "vo_create: device %d not present (%d devices)",
               device, n);
    hipDeviceProp_t prop;
    VO_HIP_CHECK(hipGetDeviceProperties(&prop, device));
    VO_REQUIRE(std::strncmp(prop.gcnArchName, "gfx950", 6) == 0, VO_ERR_NODEV,
               "vo_create: device %d is %s; this library is built for gfx950 only", device,
               prop.gcnArchName);
    VO_HIP_CHECK(hipSetDevice(device));
    std::unique_ptr<vo_ctx> c(new vo_ctx);
    c->device = device;
    c->num_cus = prop.multiProcessorCount;
    VO_HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    out = c.release();
  });
  return rc == VO_OK ? out : nullptr;
}

void vo_destroy(vo_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  delete ctx;
}

void* vo_stream(vo_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int vo_synchronize(vo_ctx* ctx) {
  return guarded([&] {
    vo::bind(ctx);
    VO_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  });
}

void* vo_device_alloc(vo_ctx* ctx, uint64_t bytes) {
  void* p = nullptr;
  int rc = guarded([&] {
    vo::bind(ctx);
    VO_HIP_CHECK(hipMalloc(&p, bytes ? bytes : 16));
  });
  return rc == VO_OK ? p : nullptr;
}

int vo_device_free(vo_ctx* ctx, void* ptr) {
  return guarded([&] {
    vo::bind(ctx);
    VO_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (ptr) VO_HIP_CHECK(hipFree(ptr));
  });
}

int vo_memcpy_h2d(vo_ctx* ctx, void* dst, const void* src, uint64_t bytes) {
  return guarded([&] {
    vo::bind(ctx);
    VO_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    VO_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  });
}

int vo_memcpy_d2h(vo_ctx* ctx, void* dst, const void* src, uint64_t bytes) {
  return guarded([&] {
    vo::bind(ctx);
    VO_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    VO_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  });
}

int vo_match_knn2_ratio(vo_ctx* ctx, const float* des0, int n0, const float* des1, int n1,
                        int dim, double ratio, int32_t* out_pairs, int32_t* out_count) {
  return guarded([&] {
    vo::bind(ctx);
    VO_REQUIRE(out_pairs && out_count, VO_ERR_ARG, "vo_match_knn2_ratio: null outputs");
    vo::match_host(ctx, des0, n0, des1, n1, dim, ratio, out_pairs, out_count, nullptr, nullptr);
  });
}

int vo_match_knn2_ratio_q(vo_ctx* ctx, const float* des0, int n0, uint64_t des0_tag, const float* des1, int n1,
                          int dim, double ratio, int32_t* out_pairs, int32_t* out_count) {
  return guarded([&] {
    vo::bind(ctx);
    VO_REQUIRE(out_pairs && out_count, VO_ERR_ARG, "vo_match_knn2_ratio_q: null outputs");
    vo::match_host(ctx, des0, n0, des1, n1, dim, ratio, out_pairs, out_count, nullptr, nullptr, des0_tag, false);
  });
}

int vo_match_knn2_ratio_dev(vo_ctx* ctx, const float* d_des0, int n0, uint64_t des0_tag, const float* d_des1,
                            int n1, int dim, double ratio, int32_t* out_pairs, int32_t* out_count) {
  return guarded([&] {
    vo::bind(ctx);
    VO_REQUIRE(out_pairs && out_count, VO_ERR_ARG, "vo_match_knn2_ratio_dev: null outputs");
    VO_REQUIRE(n0 >= 0 && n1 >= 0 && dim >= 1, VO_ERR_ARG, "vo_match_knn2_ratio_dev: bad shape");
    // no kernel reads a pointer this runtime does not know as device memory of the context's GPU
    // covering the rows (a pointer of another HIP runtime instance, or of host memory, is refused)
    vo::check_device_range(ctx, d_des0, (size_t)n0 * dim * 4, "des0");
    vo::check_device_range(ctx, d_des1, (size_t)n1 * dim * 4, "des1");
    vo::match_host(ctx, d_des0, n0, d_des1, n1, dim, ratio, out_pairs, out_count, nullptr, nullptr, des0_tag, true);
  });
}

int vo_match_knn2(vo_ctx* ctx, const float* des0, int n0, const float* des1, int n1, int dim,
                  int32_t* idx_out, float* dist_out) {
  return guarded([&] {
    vo::bind(ctx);
    VO_REQUIRE(idx_out && dist_out, VO_ERR_ARG, "vo_match_knn2: null outputs");
    vo::match_host(ctx, des0, n0, des1, n1, dim, 0.0, nullptr, nullptr, idx_out, dist_out);
  });
}

int vo_triangulate(vo_ctx* ctx, const double* P1, const double* P2, const double* T_cw2,
                   const double* K, const float* pts1, const float* pts2, int n,
                   double min_depth, double max_reproj_err, float* pts3d_out, uint8_t* mask_out) {
  return guarded([&] {
    vo::bind(ctx);
    VO_REQUIRE(P1 && P2 && T_cw2 && K && n >= 0, VO_ERR_ARG, "vo_triangulate: bad arguments");
    if (n == 0) return;
    VO_REQUIRE(pts1 && pts2 && pts3d_out && mask_out, VO_ERR_ARG, "vo_triangulate: null arrays");
    vo::triangulate_host(ctx, P1, P2, T_cw2, K, pts1, pts2, n, min_depth, max_reproj_err, pts3d_out, mask_out);
  });
}

int vo_triangulate_async(vo_ctx* ctx, const double* P1, const double* P2, const double* T_cw2,
                         const double* K, const float* d_pts1, const float* d_pts2, int n,
                         double min_depth, double max_reproj_err, float* d_pts3d, uint8_t* d_mask) {
  return guarded([&] {
    vo::bind(ctx);
    VO_REQUIRE(P1 && P2 && T_cw2 && K && n >= 0, VO_ERR_ARG, "vo_triangulate_async: bad arguments");
    if (n == 0) return;
    VO_REQUIRE(d_pts1 && d_pts2 && d_pts3d && d_mask, VO_ERR_ARG, "vo_triangulate_async: null arrays");
    vo::tri_run(ctx, P1, P2, T_cw2, K, d_pts1, d_pts2, n, min_depth, max_reproj_err, d_pts3d, d_mask);
  });
}

int vo_pnp_ransac(vo_ctx* ctx, const float* objpts, const float* imgpts, int n, const double* K,
                  int iterations, double reproj_err, double confidence, double* rvec_out,
                  double* tvec_out, uint8_t* mask_out, int32_t* success_out) {
  return guarded([&] {
    vo::bind(ctx);
    VO_REQUIRE(K && n >= 0 && rvec_out && tvec_out && success_out, VO_ERR_ARG,
               "vo_pnp_ransac: bad arguments");
    VO_REQUIRE(n == 0 || (objpts && imgpts && mask_out), VO_ERR_ARG, "vo_pnp_ransac: null arrays");
    *success_out = 0;
    for (int k = 0; k < 3; ++k) rvec_out[k] = tvec_out[k] = 0.0;
    if (n == 0) return;
    vo::pnp_ransac_host(ctx, objpts, imgpts, n, K, iterations, reproj_err, confidence, rvec_out, tvec_out, mask_out,
                        success_out);
  });
}

int vo_pnp_ransac_batch_async(vo_ctx* ctx, const float* d_objpts, const float* d_imgpts,
                              const int32_t* offsets, int batch, const double* K, int iterations,
                              double reproj_err, double confidence, double* d_pose, uint8_t* d_mask,
                              int32_t* d_status) {
  return guarded([&] {
    vo::bind(ctx);
    VO_REQUIRE(offsets && K && batch >= 0 && d_pose && d_status, VO_ERR_ARG,
               "vo_pnp_ransac_batch_async: bad arguments");
    VO_REQUIRE(batch == 0 || offsets[batch] == 0 || (d_objpts && d_imgpts && d_mask), VO_ERR_ARG,
               "vo_pnp_ransac_batch_async: null arrays");
    vo::pnp_run(ctx, d_objpts, d_imgpts, offsets, batch, K, iterations, reproj_err, confidence, d_pose,
                d_mask, d_status);
  });
}

int vo_essential_ransac(vo_ctx* ctx, const float* pts1, const float* pts2, int n, const double* K, int max_iters,
                        double threshold, double prob, double* E_out, uint8_t* mask_out, int32_t* success_out,
                        int32_t* inliers_out) {
  return guarded([&] {
    vo::bind(ctx);
    VO_REQUIRE(K && n >= 0 && E_out && success_out && inliers_out, VO_ERR_ARG, "vo_essential_ransac: bad arguments");
    VO_REQUIRE(n == 0 || (pts1 && pts2 && mask_out), VO_ERR_ARG, "vo_essential_ransac: null arrays");
    vo::essential_ransac_host(ctx, pts1, pts2, n, K, max_iters, threshold, prob, E_out, mask_out, success_out,
                              inliers_out);
  });
}

int vo_recover_pose(vo_ctx* ctx, const double* E, const float* pts1, const float* pts2, int n, const double* K,
                    double distance_thresh, double* R_out, double* t_out, uint8_t* mask_out, int32_t* good_out) {
  return guarded([&] {
    vo::bind(ctx);
    VO_REQUIRE(E && K && n >= 0 && R_out && t_out && good_out, VO_ERR_ARG, "vo_recover_pose: bad arguments");
    VO_REQUIRE(n == 0 || (pts1 && pts2 && mask_out), VO_ERR_ARG, "vo_recover_pose: null arrays");
    vo::recover_pose_host(ctx, E, pts1, pts2, n, K, distance_thresh, R_out, t_out, mask_out, good_out);
  });
}

int vo_klt_track(vo_ctx* ctx, const uint8_t* img0, uint64_t tag0, const uint8_t* img1, uint64_t tag1, int h, int w,
                 const float* pts0, float* pts1, int n, const vo_klt_options* opt, uint8_t* status, float* err,
                 int32_t* n_tracked) {
  return guarded([&] {
    // the arguments' own checks first: they need no device (nor a context)
    VO_REQUIRE(opt && pts1 && status, VO_ERR_ARG, "vo_klt_track: null options or outputs");
    VO_REQUIRE(n >= 0 && h >= 1 && w >= 1, VO_ERR_ARG, "vo_klt_track: bad shape n=%d h=%d w=%d", n, h, w);
    VO_REQUIRE(n == 0 || pts0, VO_ERR_ARG, "vo_klt_track: null pts0 with n > 0");
    VO_REQUIRE((img0 || tag0) && (img1 || tag1), VO_ERR_ARG, "vo_klt_track: null image with tag 0");
    VO_REQUIRE(opt->win_radius >= 1 && opt->win_radius <= 15, VO_ERR_ARG, "vo_klt_track: win_radius %d outside 1..15",
               opt->win_radius);
    VO_REQUIRE(opt->levels >= 1 && opt->levels <= 8, VO_ERR_ARG, "vo_klt_track: levels %d outside 1..8", opt->levels);
    VO_REQUIRE(opt->max_iters >= 1 && opt->max_iters <= 100, VO_ERR_ARG, "vo_klt_track: max_iters %d outside 1..100",
               opt->max_iters);
    auto good = [](float v) { return std::isfinite(v) && v >= 0.f; };
    VO_REQUIRE(good(opt->eps), VO_ERR_ARG, "vo_klt_track: eps must be finite and >= 0");
    VO_REQUIRE(good(opt->min_eig), VO_ERR_ARG, "vo_klt_track: min_eig must be finite and >= 0");
    VO_REQUIRE(good(opt->fb_thresh), VO_ERR_ARG, "vo_klt_track: fb_thresh must be finite and >= 0");
    VO_REQUIRE(good(opt->max_err), VO_ERR_ARG, "vo_klt_track: max_err must be finite and >= 0");
    VO_REQUIRE((opt->flags & ~(VO_KLT_GUESS | VO_KLT_FB)) == 0, VO_ERR_ARG, "vo_klt_track: unknown flags 0x%x",
               opt->flags);
    VO_REQUIRE(opt->reserved == 0, VO_ERR_ARG, "vo_klt_track: reserved must be 0");
    if (n_tracked) *n_tracked = 0;
    if (n == 0) return;
    vo::bind(ctx);
    vo::klt_track_host(ctx, img0, tag0, img1, tag1, h, w, pts0, pts1, n, opt, status, err, n_tracked);
  });
}

int vo_klt_pyramid(vo_ctx* ctx, const uint8_t* img, int h, int w, int levels, uint8_t* out, int64_t cap,
                   int32_t* levels_out) {
  return guarded([&] {
    VO_REQUIRE(img && out && h >= 1 && w >= 1 && levels >= 1 && levels <= 8, VO_ERR_ARG,
               "vo_klt_pyramid: bad arguments");
    vo::bind(ctx);
    vo::klt_pyramid_host(ctx, img, h, w, levels, out, cap, levels_out);
  });
}

int vo_klt_layout(int h, int w, int levels, int win_radius, int64_t* out, int n) {
  int count = 0;
  const int rc = guarded([&] {
    VO_REQUIRE(h >= 1 && w >= 1 && levels >= 1 && levels <= 8 && win_radius >= 0 && win_radius <= 15 && n >= 0 &&
                   (n == 0 || out),
               VO_ERR_ARG, "vo_klt_layout: bad arguments");
    count = vo::klt_layout(h, w, levels, win_radius, out, n);
  });
  return rc == VO_OK ? count : rc;
}

int vo_good_features(vo_ctx* ctx, const uint8_t* img, uint64_t tag, int h, int w, const uint8_t* mask,
                     const float* keep, int n_keep, const vo_corner_options* opt, float* corners, float* resp,
                     int32_t* n_out) {
  return guarded([&] {
    // the arguments' own checks first: they need no device (nor a context)
    VO_REQUIRE(opt && corners && n_out, VO_ERR_ARG, "vo_good_features: null options or outputs");
    VO_REQUIRE(n_keep >= 0 && h >= 1 && w >= 1, VO_ERR_ARG, "vo_good_features: bad shape n_keep=%d h=%d w=%d", n_keep,
               h, w);
    VO_REQUIRE((int64_t)h * w <= (int64_t)1 << 30, VO_ERR_ARG, "vo_good_features: bad shape, %d x %d is above 2^30 pixels",
               h, w);
    VO_REQUIRE(n_keep == 0 || keep, VO_ERR_ARG, "vo_good_features: null keep with n_keep > 0");
    VO_REQUIRE(img || tag, VO_ERR_ARG, "vo_good_features: null image with tag 0");
    VO_REQUIRE(opt->max_corners >= 1 && (int64_t)opt->max_corners <= (int64_t)h * w, VO_ERR_ARG,
               "vo_good_features: max_corners %d outside 1..h*w", opt->max_corners);
    VO_REQUIRE(opt->block_radius >= 1 && opt->block_radius <= 3, VO_ERR_ARG,
               "vo_good_features: block_radius %d outside 1..3", opt->block_radius);
    VO_REQUIRE(std::isfinite(opt->quality) && opt->quality > 0.f && opt->quality <= 1.f, VO_ERR_ARG,
               "vo_good_features: quality must be finite, > 0 and <= 1");
    VO_REQUIRE(std::isfinite(opt->min_distance) && opt->min_distance >= 0.f && opt->min_distance <= 1024.f, VO_ERR_ARG,
               "vo_good_features: min_distance must be finite and in 0..1024");
    VO_REQUIRE(opt->flags == 0, VO_ERR_ARG, "vo_good_features: unknown flags 0x%x", opt->flags);
    VO_REQUIRE(opt->reserved == 0, VO_ERR_ARG, "vo_good_features: reserved must be 0");
    *n_out = 0;
    if (h < 3 || w < 3) return;  // no interior pixel: no corners
    vo::bind(ctx);
    vo::good_features_host(ctx, img, tag, h, w, mask, keep, n_keep, opt, corners, resp, n_out);
  });
}

int vo_corner_response(vo_ctx* ctx, const uint8_t* img, int h, int w, int block_radius, float* out) {
  return guarded([&] {
    VO_REQUIRE(img && out, VO_ERR_ARG, "vo_corner_response: null image or output");
    VO_REQUIRE(h >= 1 && w >= 1 && (int64_t)h * w <= (int64_t)1 << 30, VO_ERR_ARG,
               "vo_corner_response: bad shape h=%d w=%d", h, w);
    VO_REQUIRE(block_radius >= 1 && block_radius <= 3, VO_ERR_ARG, "vo_corner_response: block_radius %d outside 1..3",
               block_radius);
    vo::bind(ctx);
    vo::corner_response_host(ctx, img, h, w, block_radius, out);
  });
}

int vo_corner_select(vo_ctx* ctx, const int32_t* xy, const float* resp, int n, const float* keep, int n_keep,
                     float min_distance, int max_corners, int32_t* out_idx, int32_t* n_out) {
  return guarded([&] {
    VO_REQUIRE(out_idx && n_out, VO_ERR_ARG, "vo_corner_select: null outputs");
    VO_REQUIRE(n >= 0 && n_keep >= 0, VO_ERR_ARG, "vo_corner_select: negative count n=%d n_keep=%d", n, n_keep);
    VO_REQUIRE(n == 0 || (xy && resp), VO_ERR_ARG, "vo_corner_select: null candidates with n > 0");
    VO_REQUIRE(n_keep == 0 || keep, VO_ERR_ARG, "vo_corner_select: null keep with n_keep > 0");
    VO_REQUIRE(std::isfinite(min_distance) && min_distance >= 0.f && min_distance <= 1024.f, VO_ERR_ARG,
               "vo_corner_select: min_distance must be finite and in 0..1024");
    VO_REQUIRE(max_corners >= 1, VO_ERR_ARG, "vo_corner_select: max_corners %d below 1", max_corners);
    for (int i = 0; i < n; ++i) {
      VO_REQUIRE(std::isfinite(resp[i]), VO_ERR_ARG, "vo_corner_select: resp[%d] is not finite", i);
      VO_REQUIRE(std::abs((int64_t)xy[2 * (size_t)i]) <= (1 << 24) && std::abs((int64_t)xy[2 * (size_t)i + 1]) <= (1 << 24),
                 VO_ERR_ARG, "vo_corner_select: coordinates of row %d outside +-2^24", i);
    }
    *n_out = 0;
    if (n == 0) return;
    vo::bind(ctx);
    vo::corner_select_host(ctx, xy, resp, n, keep, n_keep, min_distance, max_corners, out_idx, n_out);
  });
}

int vo_corner_stats(vo_ctx* ctx, int32_t out[4]) {
  return guarded([&] {
    VO_REQUIRE(ctx && out, VO_ERR_ARG, "vo_corner_stats: null arguments");
    vo::corner_stats(ctx, out);
  });
}

int vo_brief_describe(vo_ctx* ctx, const uint8_t* img, uint64_t tag, int h, int w, const float* pts, int n, int flags,
                      uint32_t* des_out, int32_t* bin_out, uint8_t* status_out) {
  return guarded([&] {
    // the arguments' own checks first: they need no device (nor a context)
    VO_REQUIRE(des_out, VO_ERR_ARG, "vo_brief_describe: null des_out");
    VO_REQUIRE(n >= 0 && h >= 1 && w >= 1, VO_ERR_ARG, "vo_brief_describe: bad shape n=%d h=%d w=%d", n, h, w);
    VO_REQUIRE((int64_t)h * w <= (int64_t)1 << 30, VO_ERR_ARG,
               "vo_brief_describe: bad shape, %d x %d is above 2^30 pixels", h, w);
    VO_REQUIRE(n == 0 || pts, VO_ERR_ARG, "vo_brief_describe: null pts with n > 0");
    VO_REQUIRE(img || tag, VO_ERR_ARG, "vo_brief_describe: null image with tag 0");
    VO_REQUIRE(flags == 0, VO_ERR_ARG, "vo_brief_describe: unknown flags 0x%x", flags);
    if (n == 0) return;
    vo::bind(ctx);
    vo::brief_describe_host(ctx, img, tag, h, w, pts, n, des_out, bin_out, status_out);
  });
}

int vo_brief_pattern(int8_t out[32 * 256 * 4], int32_t dir_out[64]) {
  return guarded([&] {
    VO_REQUIRE(out && dir_out, VO_ERR_ARG, "vo_brief_pattern: null outputs");
    vo::brief_pattern(out, dir_out);
  });
}

int vo_match_hamming(vo_ctx* ctx, const uint32_t* des0, int n0, const uint32_t* des1, int n1, int words,
                     const vo_match_hamming_options* opt, int32_t* out_pairs, int32_t* out_dist, int32_t* out_count,
                     int32_t* knn_idx, int32_t* knn_dist) {
  return guarded([&] {
    // the arguments' own checks first: they need no device (nor a context)
    VO_REQUIRE(opt && out_pairs && out_count, VO_ERR_ARG, "vo_match_hamming: null options or outputs");
    VO_REQUIRE(n0 >= 0 && n1 >= 0 && words >= 1 && words <= 16, VO_ERR_ARG,
               "vo_match_hamming: bad shape n0=%d n1=%d words=%d", n0, n1, words);
    VO_REQUIRE((opt->flags & ~(VO_MATCH_DEVICE_PTRS | VO_MATCH_HAMMING_MUTUAL)) == 0, VO_ERR_ARG,
               "vo_match_hamming: unknown flags 0x%x", opt->flags);
    VO_REQUIRE(opt->reserved == 0, VO_ERR_ARG, "vo_match_hamming: reserved must be 0");
    VO_REQUIRE(std::isfinite(opt->ratio) && opt->ratio >= 0.0 && opt->max_dist >= 0, VO_ERR_ARG,
               "vo_match_hamming: ratio must be finite and >= 0, max_dist >= 0");
    VO_REQUIRE((n0 == 0 || des0) && (n1 == 0 || des1), VO_ERR_ARG, "vo_match_hamming: null array with a nonzero size");
    *out_count = 0;
    if (n0 == 0) return;
    if (n1 == 0) {  // no neighbour exists
      for (size_t k = 0; k < 2 * (size_t)n0; ++k) {
        if (knn_idx) knn_idx[k] = -1;
        if (knn_dist) knn_dist[k] = INT32_MAX;
      }
      return;
    }
    vo::bind(ctx);
    const bool dev = (opt->flags & VO_MATCH_DEVICE_PTRS) != 0;
    if (dev) {  // as vo_match_mutual: refused before any launch
      vo::check_device_range(ctx, des0, (size_t)n0 * words * 4, "des0");
      vo::check_device_range(ctx, des1, (size_t)n1 * words * 4, "des1");
    }
    vo::match_hamming_host(ctx, des0, n0, des1, n1, words, opt->ratio, opt->max_dist,
                           (opt->flags & VO_MATCH_HAMMING_MUTUAL) != 0, dev, out_pairs, out_dist, out_count, knn_idx,
                           knn_dist);
  });
}

int vo_sift_detect(vo_ctx* ctx, const uint8_t* img, int h, int w, double contrast, double edge, double sigma,
                   int n_layers, int capacity, float* kp_f, int32_t* kp_i, int32_t* count) {
  return guarded([&] {
    vo::bind(ctx);
    VO_REQUIRE(img && count && capacity >= 0 && (capacity == 0 || (kp_f && kp_i)), VO_ERR_ARG,
               "vo_sift_detect: bad arguments");
    VO_REQUIRE(h >= 1 && w >= 1, VO_ERR_ARG, "vo_sift_detect: empty image %dx%d", h, w);
    vo::sift_detect_host(ctx, img, h, w, contrast, edge, sigma, n_layers, capacity, kp_f, kp_i, count);
  });
}

int vo_sift_detect_batch_async(vo_ctx* ctx, const uint8_t* d_imgs, int batch, int h, int w, double contrast,
                               double edge, double sigma, int n_layers, int capacity, float* d_kpf,
                               int32_t* d_kpi, int32_t* d_count) {
  return guarded([&] {
    vo::bind(ctx);
    VO_REQUIRE(d_imgs && d_count && capacity >= 0 && (capacity == 0 || (d_kpf && d_kpi)), VO_ERR_ARG,
               "vo_sift_detect_batch_async: bad arguments");
    vo::sift_run(ctx, d_imgs, batch, h, w, contrast, edge, sigma, n_layers, capacity, d_kpf, d_kpi, d_count,
                 nullptr, nullptr, nullptr);
  });
}

int vo_sift_pyramid(vo_ctx* ctx, const uint8_t* img, int h, int w, double sigma, int n_layers, float* g_out,
                    int64_t g_floats, float* d_out, int64_t d_floats) {
  return guarded([&] {
    vo::bind(ctx);
    VO_REQUIRE(img && g_out && d_out && h >= 1 && w >= 1, VO_ERR_ARG, "vo_sift_pyramid: bad arguments");
    vo::sift_pyramid_host(ctx, img, h, w, sigma, n_layers, g_out, g_floats, d_out, d_floats);
  });
}

int vo_sift_detect_and_compute(vo_ctx* ctx, const uint8_t* img, int h, int w, int nfeatures, double contrast,
                               double edge, double sigma, int n_layers, int capacity, vo_sift_keypoint* kps,
                               float* desc, int32_t* count) {
  return guarded([&] {
    vo::bind(ctx);
    VO_REQUIRE(img && kps && desc && count && capacity >= 1 && h >= 1 && w >= 1, VO_ERR_ARG,
               "vo_sift_detect_and_compute: bad arguments");
    vo::sift_detect_and_compute_host(ctx, img, h, w, nfeatures, contrast, edge, sigma, n_layers, capacity, kps, desc,
                                     count, false, "vo_sift_detect_and_compute");
  });
}

int vo_sift_detect_and_compute_dev(vo_ctx* ctx, const uint8_t* img, int h, int w, int nfeatures, double contrast,
                                   double edge, double sigma, int n_layers, int capacity, vo_sift_keypoint* d_kps,
                                   float* d_desc, int32_t* count) {
  return guarded([&] {
    vo::bind(ctx);
    VO_REQUIRE(img && d_kps && d_desc && count && capacity >= 1 && h >= 1 && w >= 1, VO_ERR_ARG,
               "vo_sift_detect_and_compute_dev: bad arguments");
    // the caller's buffers: device memory of this runtime on the context's GPU, capacity entries each
    vo::check_device_range(ctx, d_kps, (size_t)capacity * sizeof(vo_sift_keypoint), "kps");
    vo::check_device_range(ctx, d_desc, (size_t)capacity * 128 * sizeof(float), "desc");
    vo::sift_detect_and_compute_host(ctx, img, h, w, nfeatures, contrast, edge, sigma, n_layers, capacity, d_kps, d_desc,
                                     count, true, "vo_sift_detect_and_compute_dev");
  });
}

int vo_sift_detect_and_compute_batch_async(vo_ctx* ctx, const uint8_t* d_imgs, int batch, int h, int w,
                                           int nfeatures, double contrast, double edge, double sigma,
                                           int n_layers, int capacity, vo_sift_keypoint* d_kps, float* d_desc,
                                           int32_t* d_counts) {
  return guarded([&] {
    vo::bind(ctx);
    vo::sift_detect_and_compute_run(ctx, d_imgs, batch, h, w, nfeatures, contrast, edge, sigma, n_layers, capacity, d_kps,
                                    d_desc, d_counts);
  });
}

int vo_sift_layout(int h, int w, int n_layers, int64_t* out, int n) {
  int rc = 0;
  const int st = guarded([&] {
    VO_REQUIRE(h >= 1 && w >= 1 && n_layers >= 1 && out && n >= 0, VO_ERR_ARG, "vo_sift_layout: bad arguments");
    rc = vo::sift_layout(h, w, n_layers, out, n);
  });
  return st == VO_OK ? rc : st;
}

int vo_pnp_subsets(int count, int iterations, int32_t* out) {
  return guarded([&] {
    VO_REQUIRE(count > 5 && iterations >= 0 && out, VO_ERR_ARG, "vo_pnp_subsets: need count > 5");
    vo::pnp_subsets(count, iterations, out);
  });
}

int vo_match_batch_async(vo_ctx* ctx, const float* d_des0, const float* d_des1, int batch,
                         int n0, int n1, int dim, double ratio, int32_t* d_best) {
  return guarded([&] {
    vo::bind(ctx);
    VO_REQUIRE(d_best && (n0 == 0 || d_des0) && (n1 == 0 || d_des1), VO_ERR_ARG,
               "vo_match_batch_async: null pointers");
    vo::match_run(ctx, d_des0, d_des1, batch, n0, n1, dim, ratio, d_best, nullptr, nullptr);
  });
}

int vo_match_mutual(vo_ctx* ctx, const float* des0, int n0, uint64_t des0_tag, const float* des1, int n1, int dim,
                    double ratio, int flags, int32_t* out_pairs, int32_t* out_count) {
  return guarded([&] {
    vo::bind(ctx);
    VO_REQUIRE(out_pairs && out_count, VO_ERR_ARG, "vo_match_mutual: null outputs");
    VO_REQUIRE(n0 >= 0 && n1 >= 0 && dim >= 1, VO_ERR_ARG, "vo_match_mutual: bad shape");
    VO_REQUIRE((flags & ~VO_MATCH_DEVICE_PTRS) == 0, VO_ERR_ARG, "vo_match_mutual: unknown flags 0x%x", flags);
    const bool dev = (flags & VO_MATCH_DEVICE_PTRS) != 0;
    if (dev) {  // as vo_match_knn2_ratio_dev: refused before any launch
      vo::check_device_range(ctx, des0, (size_t)n0 * dim * 4, "des0");
      vo::check_device_range(ctx, des1, (size_t)n1 * dim * 4, "des1");
    }
    vo::match_host(ctx, des0, n0, des1, n1, dim, ratio, out_pairs, out_count, nullptr, nullptr, des0_tag, dev, true);
  });
}

int vo_match_gated(vo_ctx* ctx, const float* des0, int n0, const float* des1, int n1, int dim,
                   const vo_match_gate_options* opt, int32_t* out_pairs, float* out_dist, int32_t* out_count) {
  return guarded([&] {
    vo::GateHostArgs g = gate_options("vo_match_gated", n0, n1, dim, opt, out_pairs, out_count);
    g.query = opt->pred;
    g.qcols = 2;
    gate_call("vo_match_gated", ctx, des0, n0, des1, n1, dim, g, out_pairs, out_dist, out_count);
  });
}

int vo_match_segment(vo_ctx* ctx, const float* des0, int n0, const float* des1, int n1, int dim,
                     const vo_match_segment_options* opt, int32_t* out_pairs, float* out_dist, int32_t* out_count) {
  return guarded([&] {
    vo::GateHostArgs g = gate_options("vo_match_segment", n0, n1, dim, opt, out_pairs, out_count);
    g.query = opt->seg;
    g.qcols = 4;
    gate_call("vo_match_segment", ctx, des0, n0, des1, n1, dim, g, out_pairs, out_dist, out_count);
  });
}

int vo_match_mutual_batch_async(vo_ctx* ctx, const float* d_des0, const float* d_des1, int batch, int n0, int n1,
                                int dim, double ratio, int32_t* d_best) {
  return guarded([&] {
    vo::bind(ctx);
    VO_REQUIRE(d_best && (n0 == 0 || d_des0) && (n1 == 0 || d_des1), VO_ERR_ARG,
               "vo_match_mutual_batch_async: null pointers");
    VO_REQUIRE(batch >= 1 && n0 >= 0 && n1 >= 0 && dim >= 1, VO_ERR_ARG, "vo_match_mutual_batch_async: bad shape");
    vo::match_mutual_batch(ctx, d_des0, d_des1, batch, n0, n1, dim, ratio, d_best);
  });
}

int vo_match_hint(vo_ctx* ctx, int kind) {
  return guarded([&] {
    vo::bind(ctx);
    VO_REQUIRE(kind == VO_DESC_AUTO || kind == VO_DESC_SIFT || kind == VO_DESC_FLOAT, VO_ERR_ARG,
               "vo_match_hint: unknown kind %d", kind);
    ctx->match.kind_hint = kind;
  });
}

int vo_ba_setup(vo_ctx* ctx, const vo_ba_problem* prob, uint64_t* session_out) {
  return guarded([&] {
    vo::bind(ctx);
    VO_REQUIRE(session_out, VO_ERR_ARG, "vo_ba_setup: null session_out");
    *session_out = 0;
    *session_out = vo::ba_setup(ctx, prob);
  });
}

int vo_ba_reserve(vo_ctx* ctx, int n_poses, int n_points, int64_t n_obs, int n_fixed) {
  return guarded([&] {
    vo::bind(ctx);
    vo::ba_reserve(ctx, n_poses, n_points, n_obs, n_fixed);
  });
}

int vo_ba_setup_prior(vo_ctx* ctx, const vo_ba_problem* prob, const vo_ba_pose_prior* prior, uint64_t* session_out) {
  if (!prior) return vo_ba_setup(ctx, prob, session_out);
  return guarded([&] {
    // the prior's own fields first: they need no device (nor a context)
    const std::string bad = vo::pose_prior_error(prob, prior);
    VO_REQUIRE(bad.empty(), VO_ERR_ARG, "%s", bad.c_str());
    vo::bind(ctx);
    VO_REQUIRE(session_out, VO_ERR_ARG, "vo_ba_setup_prior: null session_out");
    *session_out = 0;
    *session_out = vo::ba_setup(ctx, prob, prior);
  });
}

int vo_ba_setup_factors(vo_ctx* ctx, const vo_ba_problem* prob, const vo_ba_pose_prior* prior,
                        const vo_ba_pose_factor* factors, int32_t n_factors, uint64_t* session_out) {
  if (n_factors == 0) return vo_ba_setup_prior(ctx, prob, prior, session_out);
  return guarded([&] {
    // the factors' and the prior's own fields first: they need no device (nor a context)
    std::string bad = vo::pose_factor_error(prob, factors, n_factors);
    if (bad.empty() && prior) bad = vo::pose_prior_error(prob, prior);
    VO_REQUIRE(bad.empty(), VO_ERR_ARG, "%s", bad.c_str());
    vo::bind(ctx);
    VO_REQUIRE(session_out, VO_ERR_ARG, "vo_ba_setup_factors: null session_out");
    *session_out = 0;
    *session_out = vo::ba_setup(ctx, prob, prior, factors, n_factors);
  });
}

int vo_ba_set_state(vo_ctx* ctx, uint64_t session, const double* poses, const double* points) {
  return ba_call(ctx, session, [&] { vo::ba_set_state(ctx, poses, points); },
                 poses && points ? nullptr : "vo_ba_set_state: null arrays");
}

int vo_ba_get_state(vo_ctx* ctx, uint64_t session, double* poses, double* points) {
  return ba_call(ctx, session, [&] { vo::ba_get_state(ctx, poses, points); },
                 poses && points ? nullptr : "vo_ba_get_state: null arrays");
}

int vo_ba_run(vo_ctx* ctx, uint64_t session, int iters, double* cost_out) {
  return ba_call(ctx, session, [&] { return vo::ba_run(ctx, iters, cost_out, true); });
}

int vo_ba_run_async(vo_ctx* ctx, uint64_t session, int iters) {
  return ba_call(ctx, session, [&] { vo::ba_run(ctx, iters, nullptr, false); });
}

int vo_ba_gn_step(vo_ctx* ctx, uint64_t session, double* S_out, double* b_out, double* dc_out,
                  double* cost_out) {
  return ba_call(ctx, session, [&] { return vo::ba_gn_step(ctx, S_out, b_out, dc_out, cost_out); });
}

int vo_ba_run_lm(vo_ctx* ctx, uint64_t session, int iters, const vo_ba_lm_options* opt, double* cost_out,
                 double* lambda_out, double* trial_out, uint8_t* accepted_out) {
  return ba_call(ctx, session,
                 [&] { return vo::ba_run_lm(ctx, iters, opt, cost_out, lambda_out, trial_out, accepted_out, true); });
}

int vo_ba_run_lm_async(vo_ctx* ctx, uint64_t session, int iters, const vo_ba_lm_options* opt) {
  return ba_call(ctx, session, [&] { vo::ba_run_lm(ctx, iters, opt, nullptr, nullptr, nullptr, nullptr, false); });
}

int vo_ba_lm_log(vo_ctx* ctx, uint64_t session, int n, double* cost_out, double* lambda_out, double* trial_out,
                 uint8_t* accepted_out) {
  return ba_call(ctx, session, [&] { return vo::ba_lm_log(ctx, n, cost_out, lambda_out, trial_out, accepted_out); });
}

int vo_ba_set_lm_stop(vo_ctx* ctx, uint64_t session, const vo_ba_lm_stop* stop) {
  return ba_call(ctx, session, [&] { vo::ba_set_lm_stop(ctx, stop); });
}

int vo_ba_lm_stop_info(vo_ctx* ctx, uint64_t session, int32_t* trials_out, int32_t* reason_out) {
  return ba_call(ctx, session, [&] { vo::ba_lm_stop_info(ctx, trials_out, reason_out); });
}

int vo_ba_set_robust(vo_ctx* ctx, uint64_t session, double huber_delta) {
  return ba_call(ctx, session, [&] { vo::ba_set_robust(ctx, huber_delta); });
}

int vo_ba_residuals(vo_ctx* ctx, uint64_t session, double* err2_out, double* depth_out) {
  return ba_call(ctx, session, [&] { vo::ba_residuals(ctx, err2_out, depth_out); });
}

int vo_ba_covariance(vo_ctx* ctx, uint64_t session, double lambda, double* pose_cov_out, double* pose_dense_out,
                     double* point_cov_out) {
  return ba_call(ctx, session,
                 [&] { return vo::ba_covariance(ctx, lambda, pose_cov_out, pose_dense_out, point_cov_out); });
}

int vo_ba_marginalize(vo_ctx* ctx, uint64_t session, int n_drop, double lambda, int32_t* n_prior_out, double* info_out,
                      double* rhs_out, double* poses0_out, double* cost0_out, uint8_t* point_marg_out) {
  return ba_call(ctx, session, [&] {
    return vo::ba_marginalize(ctx, n_drop, lambda, n_prior_out, info_out, rhs_out, poses0_out, cost0_out, point_marg_out);
  });
}

int vo_ba_set_obs_weights(vo_ctx* ctx, uint64_t session, const double* w) {
  return ba_call(ctx, session, [&] { vo::ba_set_obs_weights(ctx, w); });
}

int vo_ba_get_obs_weights(vo_ctx* ctx, uint64_t session, double* w_out) {
  return ba_call(ctx, session, [&] { vo::ba_get_obs_weights(ctx, w_out); },
                 w_out ? nullptr : "vo_ba_get_obs_weights: null output");
}

int vo_ba_cull(vo_ctx* ctx, uint64_t session, const vo_ba_cull_options* opt, int32_t* n_culled_out,
               int32_t* n_active_out) {
  return ba_call(ctx, session, [&] { vo::ba_cull(ctx, opt, n_culled_out, n_active_out, true); });
}

int vo_ba_cull_async(vo_ctx* ctx, uint64_t session, const vo_ba_cull_options* opt) {
  return ba_call(ctx, session, [&] { vo::ba_cull(ctx, opt, nullptr, nullptr, false); });
}

int vo_ba_solve(vo_ctx* ctx, const vo_ba_problem* prob, double* poses, double* points, int iters,
                double* cost_out) {
  uint64_t s = 0;
  int rc = vo_ba_setup(ctx, prob, &s);
  if (rc) return rc;
  rc = vo_ba_set_state(ctx, s, poses, points);
  if (rc) return rc;
  const int run_rc = vo_ba_run(ctx, s, iters, cost_out);
  if (run_rc && run_rc != VO_ERR_NOT_SPD) return run_rc;
  rc = vo_ba_get_state(ctx, s, poses, points);
  return rc ? rc : run_rc;
}

int vo_ba_plan_stats(vo_ctx* ctx, int64_t* out, int n) {
  int k = 0;
  int g = guarded([&] {
    vo::bind(ctx);
    k = vo::ba_stats(ctx, out, n);
  });
  return g != VO_OK ? g : k;
}

int vo_profile_enable(vo_ctx* ctx, int on) {
  return guarded([&] {
    vo::bind(ctx);
    VO_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    ctx->prof.on = on != 0;
    ctx->prof.recs.clear();
    ctx->prof.used = 0;
  });
}

int vo_profile_read(vo_ctx* ctx, double* ms_out, int64_t* counts_out) {
  return guarded([&] {
    vo::bind(ctx);
    VO_REQUIRE(ms_out && counts_out, VO_ERR_ARG, "vo_profile_read: null outputs");
    VO_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    ctx->prof.read(ms_out, counts_out);
  });
}

int vo_ba_debug_stamps(vo_ctx* ctx, uint64_t* out, int n) {
  int k = 0;
  int g = guarded([&] {
    vo::bind(ctx);
    k = vo::ba_stamps(ctx, out, n);
  });
  return g != VO_OK ? g : k;
}

int vo_ba_plan_digest(const vo_ba_problem* prob, int target_segments, uint64_t* digest) {
  return guarded([&] {
    VO_REQUIRE(prob && digest, VO_ERR_ARG, "vo_ba_plan_digest: null argument");
    vo::BAPlan P;
    const std::string err = vo::plan_window(P, prob, vo::seg_obs_for(prob->n_obs, target_segments));
    VO_REQUIRE(err.empty(), VO_ERR_ARG, "vo_ba_plan_digest: %s", err.c_str());
    *digest = vo::plan_digest(P);
  });
}

int vo_ba_testing_plan_slide(const vo_ba_problem* prev, const vo_ba_problem* cur, int seg_obs, int seg_chunks,
                             uint64_t* digest, int64_t* reused_chunks) {
  return guarded([&] {
    VO_REQUIRE(cur && digest && seg_obs >= 1, VO_ERR_ARG, "vo_ba_testing_plan_slide: bad argument");
    vo::BAPlan A, B;
    std::string err = prev ? vo::plan_window(A, prev, seg_obs, nullptr, seg_chunks) : "";
    if (err.empty()) err = vo::plan_window(B, cur, seg_obs, prev ? &A : nullptr, seg_chunks);
    VO_REQUIRE(err.empty(), VO_ERR_ARG, "vo_ba_testing_plan_slide: %s", err.c_str());
    *digest = vo::plan_digest(B);
    if (reused_chunks) *reused_chunks = B.reused_chunks;
  });
}

int vo_ba_group_by_point(int n_points, int n_obs, const int32_t* obs_pt, int32_t* order, int32_t* point_ptr) {
  bool grouped = true;
  const int rc = guarded([&] {
    const std::string err = vo::group_by_point(n_points, n_obs, obs_pt, order, point_ptr, grouped);
    VO_REQUIRE(err.empty(), VO_ERR_ARG, "%s", err.c_str());
  });
  return rc == VO_OK && !grouped ? 1 : rc;
}

int vo_ba_plan_probe(const vo_ba_problem* prob, int target_segments, int64_t* out, int n) {
  int k = 0;
  int g = guarded([&] {
    VO_REQUIRE(prob && out, VO_ERR_ARG, "vo_ba_plan_probe: null argument");
    vo::BAPlan P;
    const std::string err = vo::plan_window(P, prob, vo::seg_obs_for(prob->n_obs, target_segments));
    VO_REQUIRE(err.empty(), VO_ERR_ARG, "vo_ba_plan_probe: %s", err.c_str());
    // (the table stays here: the band split is declared in ba_band.h, which needs HIP)
    int64_t max_pairs = 0, max_slots = 0, max_cams = 0;
    for (int c = 0, s = 0; c < P.n_chunks(); ++c) {
      while (s + 1 < P.n_segments() + 1 && P.seg_chunk[s + 1] <= c) ++s;
      const int ns = P.seg_slot_off[s + 1] - P.seg_slot_off[s];
      const int b = P.chunk_slot_base[c];
      max_pairs = std::max<int64_t>(max_pairs, P.slot_ptr[b + ns] - P.slot_ptr[b]);
    }
    for (int s = 0; s < P.n_segments(); ++s) {
      max_slots = std::max<int64_t>(max_slots, P.seg_slot_off[s + 1] - P.seg_slot_off[s]);
      max_cams = std::max<int64_t>(max_cams, P.seg_cam_off[s + 1] - P.seg_cam_off[s]);
    }
    int span = 0;
    for (int r = 0; r < P.n_free; ++r) span = std::max(span, r - P.prof_first[r]);
    std::vector<int> first(P.prof_first.begin(), P.prof_first.end());
    const vo::BandSplit T = vo::band_split(P.n_free, first);
    const int64_t v[14] = {P.n_chunks(), P.n_segments(), P.n_slab_slots(), P.n_prof_blocks(),
                           P.n_te, max_pairs, max_slots, max_cams, P.n_free, span,
                           vo::band_supported(P.n_free, T.w, P.n_poses) ? 1 : 0, T.m, T.s, T.nb};
    k = std::min(n, 14);
    for (int i = 0; i < k; ++i) out[i] = v[i];
  });
  return g != VO_OK ? g : k;
}

int vo_comm_unique_id(char out[128]) {
  return guarded([&] { vo::comm_unique_id(out); });
}

int vo_comm_init(vo_ctx* ctx, int nranks, int rank, const char id[128]) {
  return guarded([&] {
    vo::bind(ctx);
    vo::comm_init(ctx, nranks, rank, id);
  });
}

// test-only (include/vo_hip_testing.h)
int vo_ba_split_reduce(vo_ctx* ctx, int on) {
  return guarded([&] {
    VO_REQUIRE(ctx != nullptr, VO_ERR_ARG, "vo_ba_split_reduce: null context");
    ctx->ba_split_reduce = on != 0;
  });
}

int vo_ba_testing_drop_reducers(vo_ctx* ctx, int n) {
  return guarded([&] {
    VO_REQUIRE(ctx != nullptr, VO_ERR_ARG, "vo_ba_testing_drop_reducers: null context");
    VO_REQUIRE(n >= 0, VO_ERR_ARG, "vo_ba_testing_drop_reducers: n < 0");
    ctx->ba_drop_reducers = n;
  });
}

int vo_ba_testing_no_split(vo_ctx* ctx, int on) {
  return guarded([&] {
    VO_REQUIRE(ctx != nullptr, VO_ERR_ARG, "vo_ba_testing_no_split: null context");
    ctx->ba_no_split = on != 0;
  });
}

int vo_ba_testing_no_chain(vo_ctx* ctx, int on) {
  return guarded([&] {
    VO_REQUIRE(ctx != nullptr, VO_ERR_ARG, "vo_ba_testing_no_chain: null context");
    ctx->ba_no_chain = on != 0;
  });
}

int vo_ba_testing_last_run(vo_ctx* ctx, int* chained, int* launches) {
  return guarded([&] {
    VO_REQUIRE(ctx != nullptr, VO_ERR_ARG, "vo_ba_testing_last_run: null context");
    vo::bind(ctx);
    vo::ba_last_run(ctx, chained, launches);
  });
}

int vo_ba_testing_chain_poll(vo_ctx* ctx, int replicas) {
  return guarded([&] {
    VO_REQUIRE(ctx != nullptr, VO_ERR_ARG, "vo_ba_testing_chain_poll: null context");
    VO_REQUIRE(replicas == 0 || replicas == 1 || replicas == 8, VO_ERR_ARG,
               "vo_ba_testing_chain_poll: %d replicas (0, 1 or 8)", replicas);
    ctx->ba_chain_poll = replicas;
  });
}

int vo_ba_testing_chain_stamps(vo_ctx* ctx, int on, uint64_t* out, int n) {
  int k = 0;
  int g = guarded([&] {
    VO_REQUIRE(ctx != nullptr, VO_ERR_ARG, "vo_ba_testing_chain_stamps: null context");
    vo::bind(ctx);
    ctx->ba_chain_stamps = on != 0;
    if (out && n > 0) k = vo::ba_chain_stamps(ctx, out, n);
  });
  return g != VO_OK ? g : k;
}

int vo_ba_testing_k1(vo_ctx* ctx, int variant) {
  return guarded([&] {
    VO_REQUIRE(ctx != nullptr, VO_ERR_ARG, "vo_ba_testing_k1: null context");
    VO_REQUIRE(variant >= -1 && variant <= vo::kWaveMaxChunks, VO_ERR_ARG, "vo_ba_testing_k1: variant %d outside -1..%d",
               variant, vo::kWaveMaxChunks);
    ctx->ba_k1_variant = variant;
  });
}

int vo_pnp_testing_group(vo_ctx* ctx, int mode) {
  return guarded([&] {
    VO_REQUIRE(ctx != nullptr, VO_ERR_ARG, "vo_pnp_testing_group: null context");
    VO_REQUIRE(mode >= -1 && mode <= 1, VO_ERR_ARG, "vo_pnp_testing_group: mode %d outside -1..1", mode);
    ctx->pnp_group = mode;
  });
}

int vo_pnp_testing_split(vo_ctx* ctx, int h1) {
  return guarded([&] {
    VO_REQUIRE(ctx != nullptr, VO_ERR_ARG, "vo_pnp_testing_split: null context");
    VO_REQUIRE(h1 >= -1, VO_ERR_ARG, "vo_pnp_testing_split: h1 %d < -1", h1);
    ctx->pnp_split = h1;
  });
}

int vo_pnp_testing_last_split(vo_ctx* ctx, int* h1, int* tail_frames) {
  return guarded([&] {
    VO_REQUIRE(ctx != nullptr && h1 && tail_frames, VO_ERR_ARG, "vo_pnp_testing_last_split: bad arguments");
    vo::bind(ctx);
    vo::pnp_last_split(ctx, h1, tail_frames);
  });
}

int vo_sift_testing_select(vo_ctx* ctx, const float* okp, const int32_t* counts, int batch, int cap_img,
                           int nfeatures, uint32_t* sel, int32_t* sel_count) {
  return guarded([&] {
    VO_REQUIRE(ctx != nullptr, VO_ERR_ARG, "vo_sift_testing_select: null context");
    VO_REQUIRE(okp && counts && sel && sel_count && nfeatures >= 0, VO_ERR_ARG,
               "vo_sift_testing_select: bad arguments");
    vo::bind(ctx);
    vo::sift_testing_select(ctx, okp, counts, batch, cap_img, nfeatures, sel, sel_count);
  });
}

int vo_comm_init_loopback(vo_ctx* ctx, int nranks, int rank, const char id[128]) {
  return guarded([&] {
    vo::bind(ctx);
    vo::comm_init_loopback(ctx, nranks, rank, id);
  });
}

}  // extern "C"
