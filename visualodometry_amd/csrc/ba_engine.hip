// The BA host engine: plans a window (ba_plan.h), keeps its device buffers and enqueues the
// Gauss-Newton iterations on the context stream -- K1, K2 and the profile K3 through ba.hip's
// launches (ba_kernels.h), the banded K3 (with K2 fused into its launch) through ba_band.hip's.
// No kernel is defined here.
#include "ba_engine.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ba_band.h"
#include "ba_comm.h"
#include "ba_cov.h"
#include "ba_kernels.h"
#include "ba_plan.h"
#include "ba_prior.h"
#include "ba_tables.h"
#include "ba_weights.h"
#include "vo_ctx.h"

#ifndef VO_BA_CHAIN
#define VO_BA_CHAIN 1  // tuning build: 0 never chains the next K1 into the solve launch
#endif
#ifndef VO_BA_CHAIN_POLL
#define VO_BA_CHAIN_POLL 8  // replicas of the chained launch's publish word (1 or 8)
#endif
#ifndef VO_BA_FUSE
#define VO_BA_FUSE 1  // tuning build: 0 launches K2 on its own
#endif
// Planner target: K1 segments per CU = K1's residency (three workgroups per CU), so the
// whole launch is one round; a tuning build may override it at compile time.
#ifndef VO_BA_SEGMENTS_PER_CU
#define VO_BA_SEGMENTS_PER_CU 3
#endif

namespace vo {

void* plan_host_alloc(size_t bytes, bool pinned) {
  void* p = nullptr;
  if (pinned) {
    if (hipHostMalloc(&p, std::max<size_t>(bytes, 64), hipHostMallocDefault) != hipSuccess) throw std::bad_alloc();
    return p;
  }
  return ::operator new(std::max<size_t>(bytes, 64), std::align_val_t(64));
}

void plan_host_free(void* p, bool pinned) noexcept {
  if (!p) return;
  if (pinned) (void)hipHostFree(p);
  else ::operator delete(p, std::align_val_t(64));
}

namespace {

template <class T, class A>
void upload(DevBuf& buf, const std::vector<T, A>& v, hipStream_t st) {
  buf.reserve(std::max<size_t>(v.size(), 1) * sizeof(T));
  if (!v.empty())
    VO_HIP_CHECK(hipMemcpyAsync(buf.ptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st));
}

// A view into a device buffer owned by someone else (the packed tables, the misc block).
struct DevView {
  void* ptr = nullptr;
  template <class T>
  T* as() const {
    return static_cast<T*>(ptr);
  }
};
// The plan's small tables packed into one device buffer: their places (256-byte aligned), their
// host sources and the views that receive their device addresses.
struct TablePack {
  struct Part {
    size_t off;
    const void* src;
    size_t n;
    DevView* view;
  };
  std::vector<Part> parts;
  size_t bytes = 0;
  template <class V>
  void add(const V& v, DevView& view) {
    const size_t off = (bytes + 255) & ~(size_t)255, n = v.size() * sizeof(v[0]);
    parts.push_back({off, v.data(), n, &view});
    bytes = off + std::max<size_t>(n, 16);
  }
};

std::atomic<uint64_t> g_ba_sessions{0};  // session ids, unique in the process

static_assert(kTabTranspose == kRedTranspose, "ba_tables.h restates K2's transpose flag");

}  // namespace

class BAEngine {
 public:
  explicit BAEngine(vo_ctx* ctx) : ctx_(ctx) {}
  ~BAEngine() {
    if (h_state_ev_) {
      (void)hipEventSynchronize(h_state_ev_);
      (void)hipEventDestroy(h_state_ev_);
    }
  }

  // Returns the new session id.  Every argument and plan check completes before any
  // collective: with a communicator, all ranks then agree (min all-reduce of [ok, F, -F])
  // and fail together, so one rank's bad shard is an error everywhere, not a hang.
  // prior: a pose prior over the leading free poses (vo_ba_setup_prior; its fields checked by the
  // caller, ba_tables.h pose_prior_error), null for none.
  // factors: n_factors pose factors (vo_ba_setup_factors; checked by the caller, pose_factor_error).
  uint64_t setup(const vo_ba_problem* prob, const vo_ba_pose_prior* prior = nullptr,
                 const vo_ba_pose_factor* factors = nullptr, int n_factors = 0) {
    PLAN_T_START();
    for (int64_t& v : setup_clock().ns) v = 0;
    // the previous setup's chunk-image DMA may still read the page-locked images the
    // planner is about to rewrite (a setup that failed after its upload returns unsynced)
    VO_HIP_CHECK(hipStreamSynchronize(ctx_->stream));
    PLAN_T(0, "setup: sync");
    have_problem_ = false;
    have_state_ = false;
    std::string err = check_problem(prob);
    // the last plan whose images reached the device: the next window's plan takes over its
    // unchanged first-camera groups (ba_plan.h build_plan)
    const bool prev_ok = plan_ok_;
    plan_ok_ = false;
    VO_REQUIRE(!prior || !sharded(), VO_ERR_STATE,
               "vo_ba_setup_prior: not with a communicator of more than one rank");
    VO_REQUIRE(n_factors <= 0 || !sharded(), VO_ERR_STATE,
               "vo_ba_setup_factors: not with a communicator of more than one rank");
    if (err.empty()) err = plan_window(*prob, prev_ok);  // sections 1 - 4
    agree_on_plan(err);
    VO_REQUIRE(err.empty(), VO_ERR_ARG, "vo_ba_setup: %s", err.c_str());
    PLAN_T(5, "setup: planned");
    upload_images();
    PLAN_T(6, "setup: images");
    std::vector<int32_t> first = local_profile_first(plan_);
    allreduce_min(first);
    // a pose prior couples its poses pairwise: a dense leading triangle of the profile
    const int prior_k = prior ? prior->n_poses : 0;
    VO_REQUIRE(prior_k <= plan_.n_free && prior_lds_bytes(prior_k) <= kPriorLdsMax, VO_ERR_ARG,
               "vo_ba_setup_prior: a prior over %d poses (free poses: %d)", prior_k, plan_.n_free);
    for (int i = 0; i < prior_k; ++i) first[i] = 0;
    // a between factor couples its two free poses
    FactorRows fac;
    if (n_factors > 0) {
      factor_free_cams(plan_.n_fixed, factors, n_factors, fac);
      factor_lower_first(fac, first);
    }
    // banded K3 when the block bandwidth and F fit it (decided on first[], before the
    // profile, whose step tables only the profile solver reads); the profile solver otherwise
    const int F = plan_.n_free;
    band_ = band_split(F, std::vector<int>(first.begin(), first.end()));
    band_on_ = F > 0 && band_supported(F, band_.w, plan_.n_poses);
    build_profile(plan_, first, !band_on_, prior_k, n_factors > 0 ? &fac : nullptr);
    PLAN_T(7, "setup: profile");
    prob_ = *prob;
    prob_.point_ptr = nullptr;
    prob_.obs_cam = nullptr;
    prob_.obs_uv = nullptr;

    const BAPlan& P = plan_;
    // the plan's small tables, placed in one device buffer and sent with one copy (upload_tables)
    TablePack pack;
    pack.add(P.chunk_hdr, d_chunk_hdr_);
    pack.add(P.slab_pos, d_slab_pos_);
    pack.add(P.cam_pos, d_cam_pos_);
    pack.add(P.seg_hdr, d_seg_hdr_);
    d_solve_tab_.ptr = d_band_tab_.ptr = nullptr;  // whichever K3 runs adds its own
    PLAN_T(8, "setup: uploads");
    d_points_.reserve(std::max(1, P.n_points) * 24ull);
    d_pose_[0].reserve(P.n_poses * 96ull);
    d_pose_[1].reserve(P.n_poses * 96ull);
    d_dc_.reserve(std::max(1, F) * 48ull);
    // (with a prior: its slab rows, rhs entries and cost entry behind K1's, build_profile)
    // (pose factors: theirs between K1's and the prior's, one cost entry per factor workgroup)
    const bool extra = prior_k || n_factors > 0;
    d_slab_.reserve(std::max(1, extra ? P.prof_src_ptr.back() : P.n_slab_slots()) * 288ull);
    d_slab_b_.reserve(std::max<size_t>(1, extra ? P.camb_ptr.back() : P.segcam_f.size()) * 48ull);
    d_slab_cost_.reserve((std::max(1, P.n_segments()) + (prior_k ? 1 : 0) + factor_blocks(std::max(0, n_factors))) * 8ull);
    if (!band_on_) {
      pack.add(P.solve_tab, d_solve_tab_);
      const SolveTableLayout& TL = P.solve_layout;
      const SolveLds in_lds = solve_lds_layout(true, P.n_prof_blocks(), F, TL.max_panel, TL.len, P.n_poses);
      solve_lds_ = in_lds.total <= kSolveLdsMax;
      solve_layout_ = solve_lds_ ? in_lds : solve_lds_layout(false, P.n_prof_blocks(), F, TL.max_panel, TL.len, P.n_poses);
      VO_REQUIRE(solve_layout_.total <= kSolveLdsMax, VO_ERR_ARG,
                 "vo_ba_setup: %d free poses / panel of %d blocks exceed the solver's LDS budget", F,
                 TL.max_panel);
      solve_lds_size_ = solve_layout_.total;
      solve_max_panel_ = std::max(1, TL.max_panel);
      solve_max_row_span_ = 0;
      for (int k = 0; k < F; ++k) solve_max_row_span_ = std::max(solve_max_row_span_, k - P.prof_first[k]);
    }
    PLAN_T(9, "setup: bufs");
    reduce_tables(pack);
    upload_tables(pack);
    PLAN_T(10, "setup: band");
    if (!band_on_) profile_solve_set_attributes(solve_lds_size_);
    PLAN_T(11, "setup: attrs");
    std::copy(setup_clock().ns, setup_clock().ns + kSetupSections, setup_ns_);
    // no sync: everything above is stream-ordered before the first iteration, pageable
    // sources are staged when their copy is issued, and the page-locked chunk images are
    // only rewritten after the sync at the top of the next setup
    have_problem_ = true;
    have_state_ = false;
    pending_ = false;
    cur_ = 0;
    sess_ = Session{};  // nothing of the previous problem's settings, lazy tables or LM run
    prior_k_ = 0;
    if (prior_k) upload_prior(*prior);
    if (n_factors > 0) upload_factors(factors, n_factors, fac);
    session_ = ++g_ba_sessions;
    return session_;
  }

  // The prior's arrays -- Lambda with its lower triangle mirrored, eta, the linearisation poses --
  // and the slab rows build_profile gave it, in one buffer: [Lambda | eta | poses0 | rows (ints)].
  void upload_prior(const vo_ba_pose_prior& pr) {
    const BAPlan& P = plan_;
    hipStream_t st = ctx_->stream;
    const int K = pr.n_poses;
    const size_t n = 6ull * K, nblk = (size_t)K * (K + 1) / 2;
    std::vector<double> h(n * n + n + 12ull * K + (nblk + K + 1) / 2 + 1);
    for (size_t r = 0; r < n; ++r)
      for (size_t c = 0; c <= r; ++c) h[r * n + c] = h[c * n + r] = pr.info[r * n + c];
    std::copy(pr.rhs, pr.rhs + n, h.begin() + n * n);
    std::copy(pr.poses0, pr.poses0 + 12ull * K, h.begin() + n * n + n);
    int32_t* rows = reinterpret_cast<int32_t*>(h.data() + n * n + n + 12ull * K);
    for (int i = 0; i < K; ++i) {
      for (int j = 0; j <= i; ++j) rows[(size_t)i * (i + 1) / 2 + j] = P.prof_src_ptr[P.prof_off[i] + j + 1] - 1;
      rows[nblk + i] = P.camb_ptr[i + 1] - 1;
    }
    upload(d_prior_, h, st);
    VO_HIP_CHECK(hipStreamSynchronize(st));  // the host vector ends here
    prior_k_ = K;
    prior_staged_ = false;
    prior_cost0_ = pr.cost0;
  }

  // The factors' arrays in one buffer: [Z | Lambda (mirrored), entry e of factor f at e n + f |
  // cam_i, cam_j | the rows build_profile gave them (ints)].
  void upload_factors(const vo_ba_pose_factor* fs, int n, const FactorRows& fac) {
    hipStream_t st = ctx_->stream;
    std::vector<double> h(48ull * n + (7ull * n + 1) / 2);
    int32_t* ints = reinterpret_cast<int32_t*>(h.data() + 48ull * n);
    for (int f = 0; f < n; ++f) {
      for (int e = 0; e < 12; ++e) h[(size_t)e * n + f] = fs[f].meas[e];
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c <= r; ++c)
          h[(size_t)(12 + 6 * r + c) * n + f] = h[(size_t)(12 + 6 * c + r) * n + f] = fs[f].info[6 * r + c];
      ints[f] = fs[f].cam_i;
      ints[n + f] = fs[f].cam_j;
    }
    std::copy(fac.rows.begin(), fac.rows.end(), ints + 2 * (size_t)n);
    upload(d_factors_, h, st);
    VO_HIP_CHECK(hipStreamSynchronize(st));  // the host vector ends here
    sess_.n_factors = n;
  }

  // The prior's and the pose factors' kernel, one launch for both, behind a K1 launch (or in its
  // place, in a window without segments): their slab sources and cost entries at the poses K1
  // linearised at.  n_drop > 0 (marginalize): only the factors that touch a dropped camera.
  void enqueue_prior(const int* status, int n_drop = 0) {
    if (!prior_k_ && !sess_.n_factors) return;
    FactorArgs Fa{};
    if (sess_.n_factors) {
      const size_t nf = (size_t)sess_.n_factors;
      Fa.n = sess_.n_factors;
      Fa.n_drop = n_drop;
      Fa.data = d_factors_.as<double>();
      Fa.cams = reinterpret_cast<const int*>(Fa.data + 48 * nf);
      Fa.rows = Fa.cams + 2 * nf;
      Fa.poses = d_pose_[cur_].as<double>();
      Fa.slab = d_slab_.as<double>();
      Fa.slab_b = d_slab_b_.as<double>();
      Fa.cost = d_slab_cost_.as<double>() + std::max(1, plan_.n_segments()) + (prior_k_ ? 1 : 0);
      Fa.status = status;
    }
    PriorArgs A{};
    if (!prior_k_) {
      launch_prior(A, Fa, ctx_->stream);
      VO_HIP_CHECK(hipGetLastError());
      return;
    }
    const size_t n = 6ull * prior_k_, nblk = (size_t)prior_k_ * (prior_k_ + 1) / 2;
    A.K = prior_k_;
    A.n_fixed = plan_.n_fixed;
    A.stage = prior_staged_ ? 0 : 1;  // Lambda's slab rows: written once, nothing else touches them
    prior_staged_ = true;
    A.cost0 = prior_cost0_;
    A.info = d_prior_.as<double>();
    A.rhs = A.info + n * n;
    A.poses0 = A.rhs + n;
    A.poses = d_pose_[cur_].as<double>();
    A.blk_row = reinterpret_cast<const int*>(A.poses0 + 12ull * prior_k_);
    A.cam_row = A.blk_row + nblk;
    A.slab = d_slab_.as<double>();
    A.slab_b = d_slab_b_.as<double>();
    A.cost = d_slab_cost_.as<double>() + std::max(1, plan_.n_segments());
    A.status = status;
    launch_prior(A, Fa, ctx_->stream);
    VO_HIP_CHECK(hipGetLastError());
  }
  // The cost entries K2, the LM decision and finalize_cost sum: the segments', the prior's and the
  // pose factors' (one per workgroup of theirs).
  int cost_entries() const {
    return std::max(1, plan_.n_segments()) + (prior_k_ ? 1 : 0) + factor_blocks(sess_.n_factors);
  }

  // Pre-sizes what a window of about (n_poses, n_points, n_obs) needs, outside the keyframe
  // calls: both plan objects' host arrays (plan_ and prev_plan_ alternate between setups; the
  // page-locked chunk images included), every device buffer, the kernels' LDS attributes (the
  // first one also loads the library's code object) and the state staging buffer.  It sets a
  // synthetic window of that size up twice -- landmark p seen by a run of consecutive cameras,
  // the runs spread over the window -- and then drops it: the context has no problem after it,
  // and the next setup takes nothing over from it.  A later, larger window still grows what it
  // needs (every array keeps a quarter of headroom).
  void reserve(int n_poses, int n_points, int64_t n_obs, int n_fixed) {
    VO_REQUIRE(n_poses >= 2 && n_points >= 1 && n_obs >= 2 * (int64_t)n_points && n_obs <= INT32_MAX &&
                   n_fixed >= 0 && n_fixed < n_poses,
               VO_ERR_ARG, "vo_ba_reserve: bad sizes");
    VO_REQUIRE(!sharded(), VO_ERR_STATE,
               "vo_ba_reserve: before vo_comm_init (a setup with a communicator is collective)");
    const ReserveWindow W = reserve_window(n_poses, n_points, n_obs);
    const std::vector<int32_t>&ptr = W.point_ptr, &cam = W.obs_cam;
    std::vector<float> uv(2 * cam.size(), 0.0f);
    vo_ba_problem pr{};
    pr.n_poses = n_poses;
    pr.n_points = n_points;
    pr.n_obs = (int32_t)cam.size();
    pr.n_fixed = n_fixed;
    pr.fx = pr.fy = 500.0;
    pr.lambda = 1.0;
    pr.point_ptr = ptr.data();
    pr.obs_cam = cam.data();
    pr.obs_uv = uv.data();
    for (int k = 0; k < 2; ++k) setup(&pr);
    h_state_.reserve((3ull * n_points + 12ull * n_poses) * 8);
    d_cost_.reserve(64 * 8);
    // step control (run_lm): the landmark snapshot and a log of up to 64 iterations
    d_lm_snap_.reserve(24ull * n_points);
    d_lm_log_.reserve(LmLog{64}.bytes());
    VO_HIP_CHECK(hipStreamSynchronize(ctx_->stream));
    plan_ok_ = false;  // nothing of the synthetic plan is taken over
    have_problem_ = false;
    have_state_ = false;
  }

  // The caller's session must be the engine's current problem (VO_ERR_STATE otherwise):
  // a later vo_ba_setup on the same context replaces it, and its sizes with it.
  void check_session(uint64_t s) const {
    VO_REQUIRE(have_problem_ && s == session_, VO_ERR_STATE,
               "BA session %llu is not this context's current problem (%llu): another vo_ba_setup replaced it",
               (unsigned long long)s, (unsigned long long)session_);
  }

  void set_state(const double* poses, const double* points) {
    VO_REQUIRE(have_problem_, VO_ERR_STATE, "vo_ba_set_state before vo_ba_setup");
    const BAPlan& P = plan_;
    hipStream_t st = ctx_->stream;
    // points gathered into internal order in the page-locked staging buffer, poses behind them
    const size_t np = 3ull * P.n_points;
    if (h_state_busy_) VO_HIP_CHECK(hipEventSynchronize(h_state_ev_));  // previous set_state's DMA
    h_state_busy_ = false;
    h_state_.reserve((np + 12ull * P.n_poses) * 8);
    double* pts = h_state_.as<double>();
    for (int q = 0; q < P.n_points; ++q)
      for (int e = 0; e < 3; ++e) pts[3ull * q + e] = points[3ull * P.pt_perm[q] + e];
    std::memcpy(pts + np, poses, P.n_poses * 96ull);
    VO_HIP_CHECK(hipMemcpyAsync(d_pose_[0].ptr, pts + np, P.n_poses * 96ull, hipMemcpyHostToDevice, st));
    if (P.n_points) VO_HIP_CHECK(hipMemcpyAsync(d_points_.ptr, pts, np * 8, hipMemcpyHostToDevice, st));
    // not synchronised here: the next writer of the staging buffer waits for this event
    if (!h_state_ev_) VO_HIP_CHECK(hipEventCreateWithFlags(&h_state_ev_, hipEventDisableTiming));
    VO_HIP_CHECK(hipEventRecord(h_state_ev_, st));
    h_state_busy_ = true;
    VO_HIP_CHECK(hipMemsetAsync(d_status_.ptr, 0, sizeof(int), st));
    if (fuse_ok_) VO_HIP_CHECK(hipMemsetAsync(d_colcnt_.ptr, 0, colcnt_bytes_, st));  // after a timed-out solve
    cur_ = 0;
    pending_ = false;
    have_state_ = true;
  }

  void get_state(double* poses, double* points) {
    require_state();
    finalize();
    const BAPlan& P = plan_;
    hipStream_t st = ctx_->stream;
    const size_t np = 3ull * P.n_points;
    if (h_state_busy_) VO_HIP_CHECK(hipEventSynchronize(h_state_ev_));  // before reserve() may free it
    h_state_busy_ = false;
    h_state_.reserve((np + 12ull * P.n_poses) * 8);
    double* pts = h_state_.as<double>();
    VO_HIP_CHECK(hipMemcpyAsync(pts + np, d_pose_[cur_].ptr, P.n_poses * 96ull, hipMemcpyDeviceToHost, st));
    if (P.n_points) VO_HIP_CHECK(hipMemcpyAsync(pts, d_points_.ptr, np * 8, hipMemcpyDeviceToHost, st));
    VO_HIP_CHECK(hipStreamSynchronize(st));
    std::memcpy(poses, pts + np, P.n_poses * 96ull);
    for (int q = 0; q < P.n_points; ++q)
      for (int e = 0; e < 3; ++e) points[3ull * P.pt_perm[q] + e] = pts[3ull * q + e];
  }

  // The Huber delta of the later linearisations (0: the plain cost and its kernels).  A pending
  // step was solved under the old delta: its landmark back substitution is enqueued first.
  void set_robust(double delta) {
    VO_REQUIRE(have_problem_, VO_ERR_STATE, "vo_ba_set_robust before vo_ba_setup");
    VO_REQUIRE(std::isfinite(delta) && delta >= 0.0, VO_ERR_ARG, "vo_ba_set_robust: huber_delta must be finite and >= 0");
    if (delta == sess_.huber) return;
    apply_pending();
    sess_.huber = delta;
  }

  // Raw squared reprojection error and camera-frame depth of every observation, in the order of
  // the problem's obs_cam, at the device state (a pending back substitution applied first).  The
  // problem-order observation arrays go to the device on a session's first call: rebuilt from the
  // plan's internal-order copies (the caller's arrays are not kept), so setup uploads nothing
  // for them.
  void residuals(double* err2_out, double* depth_out) {
    require_state();
    apply_pending();
    const BAPlan& P = plan_;
    hipStream_t st = ctx_->stream;
    const size_t M = (size_t)P.n_obs;
    if (M == 0) return;
    upload_obs();
    d_obs_out_.reserve(2 * M * 8);
    ObsResidualArgs A;
    A.n_obs = (int)M;
    A.fx = prob_.fx; A.fy = prob_.fy; A.cx = prob_.cx; A.cy = prob_.cy;
    A.obs_cam = d_obs_cam_.as<int>();
    A.obs_pt = d_obs_pt_.as<int>();
    A.obs_uv = d_obs_uv_.as<float2>();
    A.poses = d_pose_[cur_].as<double>();
    A.points = d_points_.as<double>();
    A.err2 = d_obs_out_.as<double>();
    A.depth = d_obs_out_.as<double>() + M;
    launch_obs_residual(A, st);
    VO_HIP_CHECK(hipGetLastError());
    if (err2_out) VO_HIP_CHECK(hipMemcpyAsync(err2_out, A.err2, M * 8, hipMemcpyDeviceToHost, st));
    if (depth_out) VO_HIP_CHECK(hipMemcpyAsync(depth_out, A.depth, M * 8, hipMemcpyDeviceToHost, st));
    VO_HIP_CHECK(hipStreamSynchronize(st));
  }

  // Pose and landmark covariance at the device state (include/vo_hip.h vo_ba_covariance, DESIGN.md
  // §Covariance): K1 in accumulate mode and the stand-alone K2 under this call's lambda leave S in
  // d_sys_ (nothing is solved; the problem's lambda, the status word, the LM state and the state
  // itself are not written), then ba_cov.hip's kernels invert S densely and form the landmark
  // blocks.  Any output may be null.
  int covariance(double lambda, double* pose_cov_out, double* pose_dense_out, double* point_cov_out) {
    require_state();
    VO_REQUIRE(std::isfinite(lambda) && lambda >= 0.0, VO_ERR_ARG, "vo_ba_covariance: lambda must be finite and >= 0");
    VO_REQUIRE(!sharded(), VO_ERR_STATE, "vo_ba_covariance: not with a communicator of more than one rank");
    require_weighted_layout("vo_ba_covariance");
    const BAPlan& P = plan_;
    const int F = P.n_free, L = P.n_points;
    const size_t n = 6ull * F;
    VO_REQUIRE(cov_solve_lds_bytes(F) <= kCovSolveLdsMax, VO_ERR_ARG,
               "vo_ba_covariance: %d free poses exceed the solve kernel's LDS", F);
    hipStream_t st = ctx_->stream;
    apply_pending();
    upload_cov_tables();
    int fail = 0;
    if (F > 0) {
      // the system: enqueue_lin / enqueue_reduce without their profiler brackets, status tests and
      // LM damping
      K1Launch k1;
      if (prepare_k1(k1)) {
        k1.A.lambda = lambda;
        k1.A.lm_lambda = nullptr;
        k1.A.status = nullptr;
        launch_k1(k1.A, kAccum, k1.wave_chunks, "vo_ba_covariance");
        VO_HIP_CHECK(hipGetLastError());
      }
      enqueue_prior(nullptr);  // the prior is part of S
      ReduceArgs R = reduce_args();
      R.lambda = lambda;
      R.lm_lambda = nullptr;
      R.status = nullptr;
      launch_reduce(R, R.nprof + 1, st);
      VO_HIP_CHECK(hipGetLastError());
      d_cov_l_.reserve(n * n * 8);
      d_cov_.reserve(n * n * 8);
      VO_HIP_CHECK(hipMemsetAsync(d_cov_l_.ptr, 0, n * n * 8, st));
      CovPoseArgs C;
      C.F = F;
      C.first = d_cov_first_.as<int>();
      C.off = d_cov_off_.as<int>();
      C.last = d_cov_last_.as<int>();
      C.dst = d_cov_dst_.as<int>();
      C.sys = d_sys_.as<double>();
      C.L = d_cov_l_.as<double>();
      C.cov = d_cov_.as<double>();
      C.fail = d_cov_fail_.as<int>();
      launch_cov_factor(C, st);
      VO_HIP_CHECK(hipGetLastError());
      launch_cov_solve(C, st);
      VO_HIP_CHECK(hipGetLastError());
      VO_HIP_CHECK(hipMemcpyAsync(&fail, C.fail, sizeof(int), hipMemcpyDeviceToHost, st));
      VO_HIP_CHECK(hipStreamSynchronize(st));
    }
    if (fail) {
      if (pose_cov_out) std::fill(pose_cov_out, pose_cov_out + 36ull * F, (double)NAN);
      if (pose_dense_out) std::fill(pose_dense_out, pose_dense_out + n * n, (double)NAN);
      if (point_cov_out) std::fill(point_cov_out, point_cov_out + 9ull * L, (double)NAN);
      set_error("vo_ba_covariance: reduced camera system not positive definite at block column %d", fail - 1);
      return VO_ERR_NOT_SPD;
    }
    if (point_cov_out && L > 0) {
      d_cov_pts_.reserve(9ull * L * 8);
      CovPointArgs Q;
      Q.n_points = L;
      Q.n_fixed = P.n_fixed;
      Q.F = F;
      Q.fx = prob_.fx; Q.fy = prob_.fy; Q.cx = prob_.cx; Q.cy = prob_.cy;
      Q.lambda = lambda;
      Q.huber = sess_.huber;
      Q.huber2 = sess_.huber * sess_.huber;
      Q.point_ptr = d_cov_ptr_.as<int>();
      Q.pt_inv = d_cov_inv_.as<int>();
      Q.obs_cam = d_obs_cam_.as<int>();
      Q.obs_uv = d_obs_uv_.as<float2>();
      Q.poses = d_pose_[cur_].as<double>();
      Q.points = d_points_.as<double>();
      Q.cov = d_cov_.as<double>();
      Q.sqrt_w = sess_.weighted ? d_sqw_obs_.as<double>() : nullptr;
      Q.out = d_cov_pts_.as<double>();
      launch_cov_points(Q, st);
      VO_HIP_CHECK(hipGetLastError());
      VO_HIP_CHECK(hipMemcpyAsync(point_cov_out, Q.out, 9ull * L * 8, hipMemcpyDeviceToHost, st));
    }
    std::vector<double> tmp;
    const double* dense = pose_dense_out;
    if (F > 0 && (pose_dense_out || pose_cov_out)) {
      if (!pose_dense_out) tmp.resize(n * n);
      double* dst = pose_dense_out ? pose_dense_out : tmp.data();
      dense = dst;
      VO_HIP_CHECK(hipMemcpyAsync(dst, d_cov_.ptr, n * n * 8, hipMemcpyDeviceToHost, st));
    }
    VO_HIP_CHECK(hipStreamSynchronize(st));
    if (pose_cov_out)  // the diagonal blocks, copied from the dense matrix
      for (int f = 0; f < F; ++f)
        for (int r = 0; r < 6; ++r)
          std::copy(dense + (6ull * f + r) * n + 6ull * f, dense + (6ull * f + r) * n + 6ull * f + 6,
                    pose_cov_out + 36ull * f + 6 * r);
    return VO_OK;
  }

  // vo_ba_marginalize (include/vo_hip.h, DESIGN.md §Pose prior): the prior a slide by n_drop cameras
  // leaves, at the device state.  A kernel marks P_D and builds the masked weights; K1 in accumulate
  // mode under them (lambda on the landmark blocks), the session's prior and the stand-alone K2
  // (no camera damping) leave the marginalised factors' system and cost in d_sys_; then the dense
  // gather and the Schur complement of the eliminated poses (ba_prior.hip).  As in covariance(),
  // nothing is solved and nothing but the pending update is written to the state.
  int marginalize(int n_drop, double lambda, int32_t* n_prior_out, double* info_out, double* rhs_out,
                  double* poses0_out, double* cost0_out, uint8_t* mask_out) {
    require_state();
    VO_REQUIRE(!sharded(), VO_ERR_STATE, "vo_ba_marginalize: not with a communicator of more than one rank");
    const BAPlan& P = plan_;
    VO_REQUIRE(n_drop >= 1 && n_drop < P.n_poses, VO_ERR_ARG, "vo_ba_marginalize: n_drop must be in 1 .. n_poses - 1");
    VO_REQUIRE(std::isfinite(lambda) && lambda >= 0.0, VO_ERR_ARG, "vo_ba_marginalize: lambda must be finite and >= 0");
    const int F = P.n_free, L = P.n_points, m = std::max(0, n_drop - P.n_fixed), R = F - m;
    VO_REQUIRE(R >= 1, VO_ERR_ARG, "vo_ba_marginalize: no free pose remains");
    VO_REQUIRE(marg_lds_bytes(F, m) <= kMargLdsMax, VO_ERR_ARG,
               "vo_ba_marginalize: the panel of %d x %d doubles (with the eliminated block) exceeds 160 KiB of LDS",
               6 * R, 6 * m);
    const int nw = plan_is_wave(P.seg_obs) ? P.seg_chunks : 0;
    VO_REQUIRE(P.n_segments() <= 0 || lin_weighted_covers(nw), VO_ERR_STATE,
               "vo_ba_marginalize: this K1 layout has no weighted instantiation (the observation mask acts as weights)");
    hipStream_t st = ctx_->stream;
    apply_pending();
    upload_cov_tables();
    upload_weight_tables();
    const size_t M = (size_t)P.n_obs, n = 6ull * F, nr = 6ull * R;
    // scratch: [masked sqrt(w), plan order (M) | b (6F) | rhs (6R) | rdst (ints, F) | fail (int) | mask (L bytes)]
    const size_t ints_off = (M + n + nr) * 8, mask_off = ints_off + ((size_t)F + 2) * 4;
    d_marg_.reserve(mask_off + std::max(1, L));
    double* d_sqw = d_marg_.as<double>();
    int* d_rdst = reinterpret_cast<int*>(d_marg_.as<char>() + ints_off);
    int* d_fail = d_rdst + F;
    unsigned char* d_mask = reinterpret_cast<unsigned char*>(d_marg_.as<char>() + mask_off);
    VO_HIP_CHECK(hipMemcpyAsync(d_rdst, red_.rdst.data(), (size_t)F * 4, hipMemcpyHostToDevice, st));  // (a session-long source)
    VO_HIP_CHECK(hipMemsetAsync(d_fail, 0, sizeof(int), st));
    MargMaskArgs K;
    K.n_points = L;
    K.n_drop = n_drop;
    K.point_ptr = d_cov_ptr_.as<int>();
    K.obs_cam = d_obs_cam_.as<int>();
    K.obs_pos = d_obs_pos_.as<int>();
    K.sqw_obs = sess_.weighted ? d_sqw_obs_.as<double>() : nullptr;
    K.sqw_plan = d_sqw;
    K.mask = d_mask;
    launch_marg_mask(K, st);
    VO_HIP_CHECK(hipGetLastError());
    K1Launch k1;
    if (prepare_k1(k1)) {
      k1.A.lambda = lambda;
      k1.A.lm_lambda = nullptr;
      k1.A.status = nullptr;
      if (!(sess_.huber > 0.0)) {
        k1.A.huber = kWeightedNoHuber;
        k1.A.huber2 = kWeightedNoHuber * kWeightedNoHuber;
      }
      const bool ok = launch_lin_weighted(k1.A, d_sqw, kAccum, k1.wave_chunks, k1.A.nseg, st);
      VO_REQUIRE(ok, VO_ERR_STATE, "vo_ba_marginalize: no weighted K1 instantiation for this layout");
      VO_HIP_CHECK(hipGetLastError());
    }
    // the session's prior is marginalised in full, of its pose factors those on a dropped camera
    enqueue_prior(nullptr, n_drop);
    ReduceArgs Rd = reduce_args();
    Rd.lambda = 0.0;  // the damping goes on the eliminated blocks only (ba_marg_kernel)
    Rd.lm_lambda = nullptr;
    Rd.status = nullptr;
    launch_reduce(Rd, Rd.nprof + 1, st);
    VO_HIP_CHECK(hipGetLastError());
    d_cov_l_.reserve(n * n * 8);
    d_cov_.reserve(n * n * 8);
    VO_HIP_CHECK(hipMemsetAsync(d_cov_l_.ptr, 0, n * n * 8, st));
    MargArgs A;
    A.F = F;
    A.m = m;
    A.lambda = lambda;
    A.first = d_cov_first_.as<int>();
    A.off = d_cov_off_.as<int>();
    A.dst = d_cov_dst_.as<int>();
    A.rdst = d_rdst;
    A.sys = d_sys_.as<double>();
    A.dense = d_cov_l_.as<double>();
    A.bvec = d_sqw + M;
    A.info = d_cov_.as<double>();
    A.rhs = d_sqw + M + n;
    A.fail = d_fail;
    launch_marg_gather(A, st);
    VO_HIP_CHECK(hipGetLastError());
    launch_marg(A, st);
    VO_HIP_CHECK(hipGetLastError());
    int fail = 0;
    std::vector<double> info(nr * nr), rhs(nr);
    std::vector<uint8_t> mask(std::max(1, L));
    double cost0 = 0.0;
    VO_HIP_CHECK(hipMemcpyAsync(&fail, d_fail, sizeof(int), hipMemcpyDeviceToHost, st));
    VO_HIP_CHECK(hipMemcpyAsync(info.data(), A.info, nr * nr * 8, hipMemcpyDeviceToHost, st));
    VO_HIP_CHECK(hipMemcpyAsync(rhs.data(), A.rhs, nr * 8, hipMemcpyDeviceToHost, st));
    VO_HIP_CHECK(hipMemcpyAsync(&cost0, A.sys + red_.cost_off, 8, hipMemcpyDeviceToHost, st));
    if (L) VO_HIP_CHECK(hipMemcpyAsync(mask.data(), d_mask, L, hipMemcpyDeviceToHost, st));
    if (poses0_out)
      VO_HIP_CHECK(hipMemcpyAsync(poses0_out, d_pose_[cur_].as<double>() + 12ull * (P.n_fixed + m), 96ull * R,
                                  hipMemcpyDeviceToHost, st));
    VO_HIP_CHECK(hipStreamSynchronize(st));
    if (mask_out) std::copy(mask.begin(), mask.begin() + L, mask_out);
    if (fail) {
      if (info_out) std::fill(info_out, info_out + nr * nr, (double)NAN);
      if (rhs_out) std::fill(rhs_out, rhs_out + nr, (double)NAN);
      if (poses0_out) std::fill(poses0_out, poses0_out + 12ull * R, (double)NAN);
      if (cost0_out) *cost0_out = NAN;
      if (n_prior_out) *n_prior_out = 0;
      set_error("vo_ba_marginalize: the eliminated pose block is not positive definite at row %d", fail - 1);
      return VO_ERR_NOT_SPD;
    }
    int k = 0;  // 1 + the last remaining pose the prior touches
    for (size_t e = 0; e < nr * nr; ++e)
      if (info[e] != 0.0) k = std::max(k, (int)(e / nr / 6) + 1);
    if (n_prior_out) *n_prior_out = k;
    if (info_out) std::copy(info.begin(), info.end(), info_out);
    if (rhs_out) std::copy(rhs.begin(), rhs.end(), rhs_out);
    if (cost0_out) *cost0_out = cost0;
    return VO_OK;
  }

  // covariance()'s tables, sent on a session's first call: the profile of S and K2's block
  // offsets, the problem-order CSR (rebuilt from the plan like upload_obs's arrays) and the
  // problem landmark -> internal landmark map.
  void upload_cov_tables() {
    upload_obs();
    if (sess_.cov_uploaded) return;
    const BAPlan& P = plan_;
    hipStream_t st = ctx_->stream;
    // (host sources that live as long as the session: the copies need no synchronisation, and the
    // vectors are rewritten only behind the next setup's)
    csr_tables(P, h_cov_ptr_, h_cov_inv_);
    upload(d_cov_ptr_, h_cov_ptr_, st);
    upload(d_cov_inv_, h_cov_inv_, st);
    upload(d_cov_first_, P.prof_first, st);
    upload(d_cov_off_, P.prof_off, st);
    upload(d_cov_last_, P.prof_last, st);
    upload(d_cov_dst_, red_.dst, st);
    d_cov_fail_.reserve(sizeof(int));
    sess_.cov_uploaded = true;
  }

  // The problem-order observation arrays of residuals() and covariance(), sent on a session's
  // first use: rebuilt from the plan's internal-order copies (the caller's arrays are not kept).
  void upload_obs() {
    if (sess_.obs_uploaded) return;
    const BAPlan& P = plan_;
    hipStream_t st = ctx_->stream;
    VO_REQUIRE(P.obs_order.size() >= (size_t)P.n_obs, VO_ERR_STATE, "BA read-out: the plan has no observation order");
    // (session-long host sources, as upload_cov_tables')
    obs_tables(P, h_obs_cam_, h_obs_pt_, h_obs_uv_);
    upload(d_obs_cam_, h_obs_cam_, st);
    upload(d_obs_pt_, h_obs_pt_, st);
    upload(d_obs_uv_, h_obs_uv_, st);
    sess_.obs_uploaded = true;
  }

  // vo_ba_set_obs_weights: information weights in problem order, null for all ones (the session
  // then has no weights again).  sqrt(w) is taken here, in IEEE double; the device only multiplies.
  void set_obs_weights(const double* w) {
    VO_REQUIRE(have_problem_, VO_ERR_STATE, "vo_ba_set_obs_weights before vo_ba_setup");
    VO_REQUIRE(!sharded(), VO_ERR_STATE, "vo_ba_set_obs_weights: not with a communicator of more than one rank");
    const BAPlan& P = plan_;
    const size_t M = (size_t)P.n_obs;
    if (w)
      for (size_t o = 0; o < M; ++o)
        VO_REQUIRE(std::isfinite(w[o]) && w[o] >= 0.0, VO_ERR_ARG,
                   "vo_ba_set_obs_weights: weight %zu is negative or not finite", o);
    apply_pending();  // under the weights the step was solved with
    if (!w) {
      sess_.weighted = false;
      return;
    }
    upload_weight_tables();
    hipStream_t st = ctx_->stream;
    std::vector<double> ww(w, w + M), so(M), sp(M);
    for (size_t o = 0; o < M; ++o) so[o] = std::sqrt(w[o]);
    for (size_t pos = 0; pos < M; ++pos) sp[pos] = so[(size_t)P.obs_order[pos]];
    upload(d_w_, ww, st);
    upload(d_sqw_obs_, so, st);
    upload(d_sqw_plan_, sp, st);
    VO_HIP_CHECK(hipStreamSynchronize(st));  // the host vectors end here
    sess_.weighted = true;
  }

  // vo_ba_get_obs_weights: synchronises; what was set, the culled observations at 0.
  void get_obs_weights(double* w_out) {
    VO_REQUIRE(have_problem_, VO_ERR_STATE, "vo_ba_get_obs_weights before vo_ba_setup");
    VO_REQUIRE(w_out, VO_ERR_ARG, "vo_ba_get_obs_weights: null output");
    const size_t M = (size_t)plan_.n_obs;
    hipStream_t st = ctx_->stream;
    if (sess_.weighted && M) VO_HIP_CHECK(hipMemcpyAsync(w_out, d_w_.ptr, M * 8, hipMemcpyDeviceToHost, st));
    VO_HIP_CHECK(hipStreamSynchronize(st));
    if (!sess_.weighted) std::fill(w_out, w_out + M, 1.0);
  }

  // vo_ba_cull / _async (vo_hip.h): two kernels on the stream at the device state, nothing but the
  // weight arrays and the counters written.  From here on the session has weights (a synchronous
  // cull of a session without them that culled nothing leaves it without).
  void cull(const vo_ba_cull_options* opt, int32_t* n_culled_out, int32_t* n_active_out, bool sync) {
    const char* who = sync ? "vo_ba_cull" : "vo_ba_cull_async";
    VO_REQUIRE(opt, VO_ERR_ARG, "%s: null options", who);
    VO_REQUIRE(std::isfinite(opt->max_chi2) && std::isfinite(opt->min_depth), VO_ERR_ARG, "%s: non-finite option", who);
    VO_REQUIRE(opt->max_chi2 >= 0.0, VO_ERR_ARG, "%s: max_chi2 < 0", who);
    VO_REQUIRE(opt->reserved == 0, VO_ERR_ARG, "%s: reserved must be 0", who);
    require_state();
    VO_REQUIRE(!sharded(), VO_ERR_STATE, "%s: not with a communicator of more than one rank", who);
    apply_pending();
    const BAPlan& P = plan_;
    hipStream_t st = ctx_->stream;
    const int M = P.n_obs;
    upload_cov_tables();  // the problem-order observation arrays and CSR
    upload_weight_tables();
    const bool was_weighted = sess_.weighted;
    if (!sess_.weighted) {
      launch_fill(d_w_.as<double>(), M, 1.0, st);
      launch_fill(d_sqw_obs_.as<double>(), M, 1.0, st);
      launch_fill(d_sqw_plan_.as<double>(), M, 1.0, st);
      VO_HIP_CHECK(hipGetLastError());
      sess_.weighted = true;
    }
    VO_HIP_CHECK(hipMemsetAsync(d_cull_cnt_.ptr, 0, 2 * sizeof(int), st));
    CullArgs C;
    C.n_obs = M;
    C.n_points = P.n_points;
    C.min_track = opt->min_track;
    C.fx = prob_.fx; C.fy = prob_.fy; C.cx = prob_.cx; C.cy = prob_.cy;
    C.max_chi2 = opt->max_chi2;
    C.min_depth = opt->min_depth;
    C.obs_cam = d_obs_cam_.as<int>();
    C.obs_pt = d_obs_pt_.as<int>();
    C.obs_uv = d_obs_uv_.as<float2>();
    C.obs_pos = d_obs_pos_.as<int>();
    C.point_ptr = d_cov_ptr_.as<int>();
    C.poses = d_pose_[cur_].as<double>();
    C.points = d_points_.as<double>();
    C.w = d_w_.as<double>();
    C.sqw_obs = d_sqw_obs_.as<double>();
    C.sqw_plan = d_sqw_plan_.as<double>();
    C.count = d_cull_cnt_.as<int>();
    launch_cull(C, st);
    VO_HIP_CHECK(hipGetLastError());
    if (!sync) return;
    int cnt[2] = {0, 0};
    VO_HIP_CHECK(hipMemcpyAsync(cnt, d_cull_cnt_.ptr, sizeof(cnt), hipMemcpyDeviceToHost, st));
    VO_HIP_CHECK(hipStreamSynchronize(st));
    if (n_culled_out) *n_culled_out = cnt[0];
    if (n_active_out) *n_active_out = cnt[1];
    if (!was_weighted && cnt[0] == 0) sess_.weighted = false;  // still all ones
  }

  // The weight arrays and the problem observation -> plan position map, on a session's first use.
  void upload_weight_tables() {
    if (sess_.wt_tables) return;
    const BAPlan& P = plan_;
    const size_t M = (size_t)P.n_obs;
    VO_REQUIRE(P.obs_order.size() >= M, VO_ERR_STATE, "BA weights: the plan has no observation order");
    obs_positions(P, h_obs_pos_);  // (a session-long host source: no synchronisation)
    upload(d_obs_pos_, h_obs_pos_, ctx_->stream);
    d_w_.reserve(std::max<size_t>(M, 1) * 8);
    d_sqw_obs_.reserve(std::max<size_t>(M, 1) * 8);
    d_sqw_plan_.reserve(std::max<size_t>(M, 1) * 8);
    d_cull_cnt_.reserve(2 * sizeof(int));
    sess_.wt_tables = true;
  }

  // iters GN iterations; sync=true finalises and reads the costs back.
  int run(int iters, double* cost_out, bool sync) {
    require_state();
    VO_REQUIRE(iters >= 0, VO_ERR_ARG, "vo_ba_run: iters < 0");
    require_weighted_layout("vo_ba_run");
    hipStream_t st = ctx_->stream;
    d_cost_.reserve((iters + 1) * 8ull);
    // Chained (chain_ok): a stand-alone K1, then iters - 1 solve launches that each carry the next
    // iteration's K1 behind its pose gate, then one plain fused launch (the last iteration has no
    // successor; finalize keeps its back-substitute-only K1).
    const bool chain = iters >= 2 && chain_ok();
    last_chained_ = chain;
    const int launches0 = launches_;
    for (int it = 0; it < iters; ++it) iteration(d_cost_.as<double>() + it, it + 1, chain && it > 0, chain && it + 1 < iters);
    last_launches_ = launches_ - launches0;  // K1 and solve launches of the iterations
    if (!sync) return VO_OK;
    finalize_cost(d_cost_.as<double>() + iters);
    std::vector<double> costs(iters + 1);
    StatusRead sr;
    VO_HIP_CHECK(hipMemcpyAsync(costs.data(), d_cost_.ptr, costs.size() * 8, hipMemcpyDeviceToHost, st));
    sr.enqueue(*this);
    VO_HIP_CHECK(hipStreamSynchronize(st));
    const auto [status, timed_out] = sr.settle(*this);
    if (status)  // iteration `status` (1-based) failed: the state is its linearisation point
      for (int k = status; k <= iters; ++k) costs[k] = NAN;
    if (cost_out) std::copy(costs.begin(), costs.end(), cost_out);
    VO_REQUIRE(!timed_out, VO_ERR_HIP, "vo_ba_run: fused reduction timed out at iteration %d (a reducer workgroup never arrived)", status - 1);
    if (status) {
      set_error("vo_ba_run: reduced camera system not positive definite at iteration %d",
                status - 1);
      return VO_ERR_NOT_SPD;
    }
    return VO_OK;
  }

  // Levenberg-Marquardt step control (include/vo_hip.h vo_ba_run_lm, DESIGN.md §Step control):
  // iters trial steps enqueued on the stream, accepted or rejected on the device.  Per trial: K1
  // accumulate, K2 + K3 (as a GN iteration, the damping read from the log's entry k), a
  // back-substitute-only K1 that lands the landmark update and leaves the trial state's cost
  // partials, and ba_lm_decide, after which the flipped pose buffer and the points hold the
  // accepted state and no step is pending.  sync: reads the log back (lm_read).
  int run_lm(int iters, const vo_ba_lm_options* opt, double* cost_out, double* lambda_out, double* trial_out,
             uint8_t* accepted_out, bool sync) {
    require_state();
    VO_REQUIRE(iters >= 0, VO_ERR_ARG, "vo_ba_run_lm: iters < 0");
    VO_REQUIRE(!sharded(), VO_ERR_STATE, "vo_ba_run_lm: not with a communicator of more than one rank");
    require_weighted_layout("vo_ba_run_lm");
    vo_ba_lm_options o;
    const std::string bad = lm_options(opt, prob_.lambda, o);
    VO_REQUIRE(bad.empty(), VO_ERR_ARG, "%s", bad.c_str());
    hipStream_t st = ctx_->stream;
    apply_pending();  // a pending GN step: under the lambda and delta it was solved with
    const LmLog log{iters};
    d_lm_log_.reserve(log.bytes());
    d_lm_snap_.reserve(24ull * std::max(1, plan_.n_points));
    // termination (set_lm_stop): with a criterion set, the decide instantiation that tests it
    const vo_ba_lm_stop& crit = sess_.lm_stop;
    const bool stop = crit.ftol > 0.0 || crit.xtol > 0.0 || crit.max_rejects > 0;
    sess_.lm = LmRun{};  // this run's record: unread, ran all until its first read says otherwise
    sess_.lm.iters = sess_.lm.trials = iters;
    sess_.lm.unread = true;
    sess_.lm.stop_on = stop;
    char* const base = d_lm_log_.as<char>();
    LmDecideArgs D{};
    D.nseg = cost_entries();
    D.n_points = plan_.n_points;
    D.n_poses = plan_.n_poses;
    D.lambda0 = o.lambda0; D.up = o.up; D.down = o.down; D.lambda_min = o.lambda_min; D.lambda_max = o.lambda_max;
    D.slab_cost = d_slab_cost_.as<double>();
    D.cost = reinterpret_cast<double*>(base + log.cost_off());
    D.lambda = reinterpret_cast<double*>(base + log.lambda_off());
    D.trial = reinterpret_cast<double*>(base + log.trial_off());
    D.accepted = reinterpret_cast<int*>(base + log.accepted_off());
    D.points = d_points_.as<double>();
    D.snap = d_lm_snap_.as<double>();
    D.status = d_status_.as<int>();
    D.ftol = crit.ftol;
    D.xtol = crit.xtol;
    D.max_rejects = crit.max_rejects;
    D.n_dc = 6 * plan_.n_free;
    D.dc = d_dc_.as<double>();
    D.stop = reinterpret_cast<int*>(base + log.stop_off());
    auto decide = [&](int k) {
      D.k = k;
      D.pose_cur = d_pose_[cur_ ^ 1].as<double>();
      D.pose_next = d_pose_[cur_].as<double>();
      ctx_->prof.begin(st, kKBaReduce);  // (no id of its own: vo_hip.h, kernel timing)
      launch_lm_decide(D, stop, st);
      ctx_->prof.end(st);
      VO_HIP_CHECK(hipGetLastError());
    };
    enqueue_lin(0);  // the cost at the start state
    decide(-1);
    struct Scope {  // the kLm kernels only between here and the end of the loop
      const double*& p;
      ~Scope() { p = nullptr; }
    } scope{lm_lambda_};
    for (int k = 0; k < iters; ++k) {
      lm_lambda_ = D.lambda + k;
      enqueue_lin(kAccum);
      enqueue_reduce();
      enqueue_solve(k + 1);
      cur_ ^= 1;
      enqueue_lin(kBacksub);  // the trial landmarks, and the cost partials at the trial state
      decide(k);
    }
    lm_lambda_ = nullptr;
    if (stop) {  // a stop word goes back to zero on the device: the next run needs no read in between
      ctx_->prof.begin(st, kKBaReduce);
      launch_lm_finish(d_status_.as<int>(), st);
      ctx_->prof.end(st);
      VO_HIP_CHECK(hipGetLastError());
    }
    if (!sync) return VO_OK;
    return lm_read(iters, cost_out, lambda_out, trial_out, accepted_out, "vo_ba_run_lm");
  }

  // Synchronises and returns the first n iterations of the last run_lm's log.  A failed
  // iteration f (non-SPD system or a timed-out fused reduction: run()'s contract) leaves the
  // state at the last accepted one; its trial and decision and every later entry are NaN / 0.
  int lm_read(int n, double* cost_out, double* lambda_out, double* trial_out, uint8_t* accepted_out,
              const char* who) {
    const LmRun& lm = sess_.lm;
    VO_REQUIRE(lm.iters >= 0, VO_ERR_STATE, "%s: no vo_ba_run_lm on this session", who);
    VO_REQUIRE(n >= 0 && n <= lm.iters, VO_ERR_ARG, "%s: n = %d outside the last run's 0..%d iterations", who, n,
               lm.iters);
    hipStream_t st = ctx_->stream;
    const LmLog log{lm.iters};
    std::vector<double> vals(log.accepted_off() / 8);
    std::vector<int> acc(std::max(1, log.n));
    VO_HIP_CHECK(hipMemcpyAsync(vals.data(), d_lm_log_.ptr, log.accepted_off(), hipMemcpyDeviceToHost, st));
    if (log.n)
      VO_HIP_CHECK(hipMemcpyAsync(acc.data(), d_lm_log_.as<char>() + log.accepted_off(), log.n * sizeof(int),
                                  hipMemcpyDeviceToHost, st));
    lm_settle();
    log.decode(vals.data(), acc.data(), n, lm.fail ? lm.fail - 1 : lm.trials, !lm.fail && lm.reason != VO_BA_LM_RAN_ALL,
               cost_out, lambda_out, trial_out, accepted_out);
    VO_REQUIRE(!lm.timeout, VO_ERR_HIP, "%s: fused reduction timed out at iteration %d (a reducer workgroup never arrived)",
               who, lm.fail - 1);
    if (lm.fail) {
      set_error("%s: reduced camera system not positive definite at iteration %d", who, lm.fail - 1);
      return VO_ERR_NOT_SPD;
    }
    return VO_OK;
  }

  // Synchronises; on the first read after an LM run also takes the status word (a failure is
  // cleared as after any run) and, from a run with a termination criterion, the two control words
  // behind the log.
  void lm_settle() {
    hipStream_t st = ctx_->stream;
    LmRun& lm = sess_.lm;
    StatusRead sr;
    int words[2] = {0, 0};
    if (lm.unread) {
      sr.enqueue(*this);
      if (lm.stop_on)
        VO_HIP_CHECK(hipMemcpyAsync(words, d_lm_log_.as<char>() + LmLog{lm.iters}.stop_off(), sizeof(words),
                                    hipMemcpyDeviceToHost, st));
    }
    VO_HIP_CHECK(hipStreamSynchronize(st));
    if (!lm.unread) return;
    const auto [failed, timed_out] = sr.settle(*this);
    lm.timeout = timed_out;
    lm.fail = failed;
    lm.unread = false;
    if (lm.fail) {
      lm.trials = lm.fail - 1;
      lm.reason = VO_BA_LM_FAILED;
    } else if (words[1] != VO_BA_LM_RAN_ALL) {
      lm.trials = words[0];
      lm.reason = words[1];
    }
  }

  // vo_ba_lm_stop_info: how the session's last LM run ended.
  void lm_stop_info(int32_t* trials_out, int32_t* reason_out) {
    VO_REQUIRE(sess_.lm.iters >= 0, VO_ERR_STATE, "vo_ba_lm_stop_info: no vo_ba_run_lm on this session");
    lm_settle();
    if (trials_out) *trials_out = sess_.lm.trials;
    if (reason_out) *reason_out = sess_.lm.reason;
  }

  // The termination criteria of the later LM runs (vo_hip.h vo_ba_set_lm_stop); null: never stop.
  void set_lm_stop(const vo_ba_lm_stop* s) {
    VO_REQUIRE(have_problem_, VO_ERR_STATE, "vo_ba_set_lm_stop before vo_ba_setup");
    const vo_ba_lm_stop v = s ? *s : vo_ba_lm_stop{};
    VO_REQUIRE(std::isfinite(v.ftol) && std::isfinite(v.xtol), VO_ERR_ARG, "vo_ba_set_lm_stop: non-finite tolerance");
    VO_REQUIRE(v.ftol >= 0.0 && v.ftol < 1.0, VO_ERR_ARG, "vo_ba_set_lm_stop: ftol must be in [0, 1)");
    VO_REQUIRE(v.xtol >= 0.0, VO_ERR_ARG, "vo_ba_set_lm_stop: xtol < 0");
    VO_REQUIRE(v.max_rejects >= 0, VO_ERR_ARG, "vo_ba_set_lm_stop: max_rejects < 0");
    VO_REQUIRE(v.reserved == 0, VO_ERR_ARG, "vo_ba_set_lm_stop: reserved must be 0");
    sess_.lm_stop = v;
  }

  // One read-back of the status word (run, gn_step, lm_settle): enqueue() the copy, synchronise
  // (the caller's, with its other copies), then settle().  After a failed fused launch (any
  // non-zero status; kBandStatusTimeout: the solver gave up waiting for its reducers) the
  // reducer counter is re-zeroed -- the stream is synchronised, so every late reducer has counted
  // itself by now -- and the timeout flag is stripped from the status word's iteration; a failed
  // iteration's status word is re-zeroed on the device and the stream synchronised.
  struct StatusRead {
    int word = 0;
    struct Result {
      int failed;      // the iteration that failed (1-based), 0: none
      bool timed_out;  // a timeout was recorded
    };
    void enqueue(BAEngine& e) {
      VO_HIP_CHECK(hipMemcpyAsync(&word, e.d_status_.ptr, sizeof(int), hipMemcpyDeviceToHost, e.ctx_->stream));
    }
    Result settle(BAEngine& e) const {
      hipStream_t st = e.ctx_->stream;
      int status = word;
      if (status && e.fuse_ok_) VO_HIP_CHECK(hipMemsetAsync(e.d_colcnt_.ptr, 0, e.colcnt_bytes_, st));
      const bool timed_out = status & kBandStatusTimeout;
      // (an LM stop word is only ever seen here with a later launch's timeout flag on it: ba_lm_finish)
      status &= ~(kBandStatusTimeout | kLmStatusStopped);
      if (status) {
        VO_HIP_CHECK(hipMemsetAsync(e.d_status_.ptr, 0, sizeof(int), st));
        VO_HIP_CHECK(hipStreamSynchronize(st));
      }
      return {status, timed_out};
    }
  };

  int gn_step(double* S_out, double* b_out, double* dc_out, double* cost_out) {
    require_state();
    require_weighted_layout("vo_ba_gn_step");
    hipStream_t st = ctx_->stream;
    const BAPlan& P = plan_;
    const int F = P.n_free;
    d_cost_.reserve(8);
    enqueue_lin(pending_ ? (kBacksub | kAccum) : kAccum);
    enqueue_reduce();
    std::vector<double> sys(red_.sys_len);
    // the reduced system as K2 wrote it: before the solve (the profile solver factors it in
    // place), or after the fused K2 + K3 launch (the banded K3 only reads it)
    if (!fused()) VO_HIP_CHECK(hipMemcpyAsync(sys.data(), d_sys_.ptr, sys.size() * 8, hipMemcpyDeviceToHost, st));
    enqueue_solve(1);
    if (fused()) VO_HIP_CHECK(hipMemcpyAsync(sys.data(), d_sys_.ptr, sys.size() * 8, hipMemcpyDeviceToHost, st));
    std::vector<double> dc(6ull * F);
    StatusRead sr;
    if (F) VO_HIP_CHECK(hipMemcpyAsync(dc.data(), d_dc_.ptr, dc.size() * 8, hipMemcpyDeviceToHost, st));
    sr.enqueue(*this);
    VO_HIP_CHECK(hipStreamSynchronize(st));
    cur_ ^= 1;
    pending_ = true;
    dense_system(P, red_, sys.data(), S_out, b_out);  // K2's output layout back to the dense symmetric S, and b
    if (dc_out) std::copy(dc.begin(), dc.end(), dc_out);
    if (cost_out) *cost_out = sys[red_.cost_off];
    const auto [status, timed_out] = sr.settle(*this);
    if (status) {
      VO_REQUIRE(!timed_out, VO_ERR_HIP, "vo_ba_gn_step: fused reduction timed out (a reducer workgroup never arrived)");
      set_error("vo_ba_gn_step: reduced camera system not positive definite");
      return VO_ERR_NOT_SPD;
    }
    return VO_OK;
  }

  void last_run(int* chained, int* launches) const {
    if (chained) *chained = last_chained_ ? 1 : 0;
    if (launches) *launches = last_launches_;
  }

  // Diagnostic build: the last chained launch's realtime stamps (100 MHz ticks), [published,
  // launch start | start, prefix done, gate passed, end per K1 workgroup]; returns the count.
  int read_chain_stamps(uint64_t* out, int n) {
    if (!stamps_on_ || !d_stamps_k1_.ptr || !last_chained_) return 0;
    const int k = std::min(n, 2 + 4 * plan_.n_segments());
    VO_HIP_CHECK(hipStreamSynchronize(ctx_->stream));
    VO_HIP_CHECK(hipMemcpy(out, d_stamps_k1_.ptr, (size_t)k * 8, hipMemcpyDeviceToHost));
    return k;
  }

  int stats(int64_t* out, int n) const {
    const BAPlan& P = plan_;
    int64_t v[12 + kSetupSections] = {P.n_chunks(), P.n_segments(), P.n_slab_slots(), (int64_t)P.slot_i.size(),
                                      P.n_prof_blocks(), P.n_te, P.algorithmic_bytes_per_iter(), band_on_ ? 1 : 0,
                                      P.reused_groups, P.reused_chunks, P.seg_obs};
    for (int i = 0; i < kSetupSections; ++i) v[11 + i] = setup_ns_[i];  // the last setup's sections
    // the banded K3's layout: 0 none (profile solver), 1 full, 2 ring, 3 split (two workgroups)
    v[11 + kSetupSections] = !band_on_ ? 0 : band_lds_.split ? 3 : band_lds_.full ? 1 : 2;
    const int k = std::min(n, 12 + kSetupSections);
    for (int i = 0; i < k; ++i) out[i] = v[i];
    return k;
  }

 private:
  void require_state() const {
    VO_REQUIRE(have_problem_, VO_ERR_STATE, "BA: no problem set up");
    VO_REQUIRE(have_state_, VO_ERR_STATE, "BA: no state set");
  }

  // ---- setup's steps, in its order ----------------------------------------------------------
  static std::string check_problem(const vo_ba_problem* prob) {
    if (!prob) return "null problem";
    if (!(prob->n_poses >= 1 && prob->n_points >= 0 && prob->n_obs >= 0)) return "bad sizes";
    if (!(prob->lambda >= 0.0)) return "lambda must be >= 0";
    if (!((prob->n_points == 0 || prob->point_ptr) && (prob->n_obs == 0 || (prob->obs_cam && prob->obs_uv))))
      return "null arrays";
    if (prob->n_points == 0 && prob->n_obs != 0) return "observations without points";
    return "";
  }

  // Plans the window into plan_ (the previous plan moves to prev_plan_, its device images to
  // d_chunk_img_prev_).  Returns the planner's error message, empty on success.
  std::string plan_window(const vo_ba_problem& pr, bool prev_ok) {
    // K1 variant (a plan property, ba_plan.h plan_is_wave): the one-wave K1 at every size --
    // cfg4's 13.7k chunks run in nine rounds of six per CU, faster than the four-wave K1's one
    // round of two-chunk segments (148 against 222 us) -- with wave_chunks()
    // chunks per segment; the four-wave K1 over multi-chunk segments only under the testing
    // switch (vo_ba_testing_k1).  The packing target is a function of this window alone, so a
    // plan that takes groups over from the previous one is the plan a scratch setup builds
    // (take-over needs equal targets: build_plan checks).
    const bool wave = ctx_->ba_k1_variant >= 0;
    const int nw = wave ? wave_chunks(pr.n_obs) : 1;
    std::vector<int32_t> zero_ptr(1, 0);
    const int32_t* pp = pr.n_points ? pr.point_ptr : zero_ptr.data();
    std::swap(plan_, prev_plan_);
    d_chunk_img_.swap(d_chunk_img_prev_);
    const BAPlan* prev = prev_ok ? &prev_plan_ : nullptr;
    auto plan = [&](int seg_obs, int seg_chunks) {
      return build_plan(plan_, pr.n_poses, pr.n_points, pr.n_obs, pr.n_fixed, pp, pr.obs_cam, pr.obs_uv, seg_obs, prev,
                        seg_chunks);
    };
    const int seg_obs = seg_obs_grid(seg_obs_for(pr.n_obs, segments_target(ctx_->num_cus, wave)));
    std::string err = plan(seg_obs, nw);
    // six-chunk segments beyond one round (one workgroup per CU): plan with three
    if (err.empty() && wave && ctx_->ba_k1_variant == 0 && nw == kWaveChunksOneRound &&
        plan_.n_segments() > ctx_->num_cus)
      err = plan(seg_obs, kWaveChunksRounds);
    PLAN_T(4, "setup: returned");
    // four-wave K1: every first-camera group ends in a partial segment, so the packing target
    // may give more segments than one round holds; then pack once more, proportionally wider
    // (on the grid; a function of the plan, which does not depend on prev)
    const int round = segments_target(ctx_->num_cus, false);
    for (int k = 0; k < 4 && err.empty() && !plan_is_wave(plan_.seg_obs) && plan_.n_segments() > round; ++k)
      err = plan(seg_obs_grid((int64_t)plan_.seg_obs * plan_.n_segments() / round + 1), 1);
    return err;
  }

  bool sharded() const { return ctx_->comm && ctx_->comm->nranks > 1; }

  // Element-wise minimum of a small host vector over the ranks (nothing on one rank): upload,
  // all-reduce on the stream, download, synchronise.
  void allreduce_min(std::vector<int32_t>& v) {
    if (!sharded() || v.empty()) return;
    DevBuf tmp;
    upload(tmp, v, ctx_->stream);
    ctx_->comm->allreduce(tmp.as<int32_t>(), v.size(), true, ctx_->stream);
    VO_HIP_CHECK(hipMemcpyAsync(v.data(), tmp.ptr, v.size() * 4, hipMemcpyDeviceToHost, ctx_->stream));
    VO_HIP_CHECK(hipStreamSynchronize(ctx_->stream));
  }

  // The cross-rank agreement on [ok, F, -F]: a rank whose checks passed takes over the error
  // of one whose did not.
  void agree_on_plan(std::string& err) {
    if (!sharded()) return;
    const int32_t F = err.empty() ? plan_.n_free : 0;
    std::vector<int32_t> agree = {err.empty() ? 1 : 0, F, -F};
    allreduce_min(agree);
    if (err.empty() && agree[0] == 0) err = "another rank's shard failed its checks";
    if (err.empty() && agree[1] != -agree[2]) err = "ranks disagree on the number of free poses";
  }

  // The largest plan array first: from page-locked memory the copy runs while the host
  // builds the profile and the K3 tables.  Images taken over from the previous plan are
  // copied on the device, in runs of consecutive chunks.
  void upload_images() {
    const BAPlan& P = plan_;
    const int nch = (int)P.chunk_img.size();
    d_chunk_img_.reserve(std::max(nch, 1) * sizeof(ChunkImg));
    ImgRuns R{};
    int copied = 0;
    auto flush = [&]() {
      if (R.n == 0) return;
      launch_img_copy(d_chunk_img_prev_.as<uint4>(), d_chunk_img_.as<uint4>(), R, copied, ctx_->stream);
      VO_HIP_CHECK(hipGetLastError());
      R.n = 0;
      copied = 0;
    };
    image_runs(P, img_runs_);
    for (const ImageRun& r : img_runs_) {
      if (r.src >= 0) {  // taken over: a run of the copy kernel
        if (R.n == kImgRuns) flush();
        R.src[R.n] = r.src;
        R.dst[R.n] = r.dst;
        copied += r.count;
        R.end[R.n++] = copied;
      } else {  // built by this plan: from the page-locked images
        VO_HIP_CHECK(hipMemcpyAsync(d_chunk_img_.as<ChunkImg>() + r.dst, P.chunk_img.data() + r.dst,
                                    (size_t)r.count * sizeof(ChunkImg), hipMemcpyHostToDevice, ctx_->stream));
      }
    }
    flush();
    plan_ok_ = true;
  }

  // K2's output layout (ba_tables.h reduce_layout) with the banded K3's own layout and tables,
  // the system buffer, and whether K2 rides in K3's launch.
  void reduce_tables(TablePack& pack) {
    const BAPlan& P = plan_;
    hipStream_t st = ctx_->stream;
    const int F = P.n_free, w = band_.w;
    reduce_layout(P, band_on_, w, band_.m + band_.s, band_col_stride(w), red_);
    size_t pad = 0;
    if (band_on_) {
      pad = band_slot_stride(w);  // the ring loader's last LDS-DMA piece reads past the end
      band_lds_ = band_lds_layout(F, band_, P.n_poses, !ctx_->ba_no_split);
      band_tab_ = band_tables(F, band_, band_lds_);
      pack.add(band_tab_.tab, d_band_tab_);
      band_set_attributes(band_lds_);  // (a no-op unless the LDS size grows)
      if (!band_lds_.full || band_lds_.split) d_fac_.reserve(band_fac_doubles(F, w) * 8);
      if (band_lds_.split) {  // the split hand-offs' exchange area (front of fac); flags start clear
        const SplitXch x = split_xch(band_tab_.n_merge, band_.s);
        VO_REQUIRE((size_t)x.end() <= band_fac_doubles(F, w), VO_ERR_STATE, "band split: exchange area");
        VO_HIP_CHECK(hipMemsetAsync(d_fac_.as<double>() + x.flag, 0, 3 * 16 * sizeof(double), st));
      }
    }
    d_sys_.reserve((red_.sys_len + pad) * 8);
    // entries K2 never writes (outside the profile, the bottom side's separator) stay 0
    VO_HIP_CHECK(hipMemsetAsync(d_sys_.ptr, 0, (red_.sys_len + pad) * 8, st));
    pack.add(red_.meta, d_red_meta_);
    pack.add(red_.out, d_red_out_);
    pack.add(red_.col, d_red_col_);
    pack.add(red_.col_need, d_col_need_);
    // K2 fused into the banded K3's launch when every workgroup of it fits one round at
    // one per CU (the solver's LDS): cfg3's 356 blocks make 178 reducers + the solver on
    // MI355X's 256 CUs (fewer CUs, e.g. a partitioned device: K2 stays a launch of its own)
    // (full mode only: the ring-mode solver reads sys with plain loads, so it must come from an
    // earlier launch)
    fuse_ok_ = VO_BA_FUSE && band_on_ && band_lds_.full && !band_lds_.split &&
               band_fused_workgroups(P.n_prof_blocks()) + 1 <= ctx_->num_cus;
  }

  // One page-locked staging buffer, one device buffer, one copy (each table a pageable
  // copy of its own cost several µs of host time apiece); both are rewritten only after the
  // stream sync at the top of the next setup.  Then the tables' views, and the small zeroed
  // buffers beside them.
  void upload_tables(const TablePack& pack) {
    hipStream_t st = ctx_->stream;
    h_tab_.reserve(pack.bytes);
    d_tab_.reserve(pack.bytes);
    for (const TablePack::Part& q : pack.parts)
      if (q.n) std::memcpy(h_tab_.as<char>() + q.off, q.src, q.n);
    VO_HIP_CHECK(hipMemcpyAsync(d_tab_.ptr, h_tab_.ptr, pack.bytes, hipMemcpyHostToDevice, st));
    for (const TablePack::Part& q : pack.parts) q.view->ptr = d_tab_.as<char>() + q.off;
    // the status word, K2's fused-round counter and the zero block (masked prefetches)
    d_misc_.reserve(kMiscBytes);
    d_status_.ptr = d_misc_.ptr;
    d_zero_.ptr = d_misc_.as<char>() + 256;
    VO_HIP_CHECK(hipMemsetAsync(d_misc_.ptr, 0, kMiscBytes, st));
    colcnt_bytes_ = band_col_count_bytes(plan_.n_free);
    d_colcnt_.reserve(colcnt_bytes_);
    VO_HIP_CHECK(hipMemsetAsync(d_colcnt_.ptr, 0, colcnt_bytes_, st));
    // the chained launches' publish word, its replicas on lines of their own (a stale word is
    // another launch's sequence number: never a match)
    d_pub_.reserve(kBandPubReplicas * kBandPubStride * sizeof(unsigned));
    VO_HIP_CHECK(hipMemsetAsync(d_pub_.ptr, 0, kBandPubReplicas * kBandPubStride * sizeof(unsigned), st));
  }

  // Planner target of one K1 round: as many segments as resident workgroups (three per CU,
  // K1's __launch_bounds__ and LDS image).  A segment's time is about its chunk count times
  // the per-chunk latency, so one round of longer segments beats two rounds of shorter ones
  // (cfg4: 766 segments instead of 985; the cfg3 plan packs 678 either way).  Round 1's
  // sweep (profiles/r01_segment_sweep.md) predates the three-per-CU K1.
  // The one-wave K1 runs one chunk per segment: the largest target packs every
  // segment as one chunk (seg_obs = 1).
  static int segments_target(int num_cus, bool wave) {
    return wave ? (1 << 30) : VO_BA_SEGMENTS_PER_CU * std::max(1, num_cus);
  }
  // Chunks per segment of the one-wave K1's plan (the testing switch's value if it sets one).
  // Three instead of one: a third of the slab rows K2 reads for a barrier per segment; cfg3
  // 14.89k -> 15.27k GN-iters/s (42 148 -> 15 538 rows), cfg4 3.91k -> 4.04k (K2 34 -> 16 us,
  // K1 148 -> 158 us); two chunks sit between (profiles/r05_k1g).  Six (one 153 KB workgroup
  // per CU, the same six waves per CU) halves the rows again, which pays while the segments fit
  // one round: cfg3 15.71k -> 15.94k (246 segments, 8 175 rows; K1 24.7 -> 24.0 us, the fused
  // K3 43.7 -> 43.3 us), but cfg4's nine rounds of single workgroups lose the overlap of one
  // workgroup's combine with another's chunks: 4.09k -> 3.69k (profiles/r05_ab/k1_six_chunks).
  // So six for windows whose six-chunk segments are predicted to fit one round (56 observations
  // per chunk with padding, cfg3's; setup re-plans with three when they do not), else three.
  // (48-observation chunks, tuning builds: eight waves per CU, two per SIMD)
  static constexpr int kWaveChunksOneRound = std::min(kChunkObs >= 64 ? 6 : 8, kWaveMaxChunks),
                       kWaveChunksRounds = std::min(3, kWaveMaxChunks);
  int wave_chunks(int64_t n_obs) const {
    if (ctx_->ba_k1_variant >= 1) return std::min(ctx_->ba_k1_variant, kWaveMaxChunks);
    const int64_t one_round_obs = (int64_t)ctx_->num_cus * kWaveChunksOneRound * (kChunkObs * 7 / 8);
    return n_obs * 10 <= one_round_obs * 11 ? kWaveChunksOneRound : kWaveChunksRounds;
  }

  LinArgs lin_args() {
    const BAPlan& P = plan_;
    LinArgs A;
    A.n_fixed = P.n_fixed;
    A.fx = prob_.fx; A.fy = prob_.fy; A.cx = prob_.cx; A.cy = prob_.cy;
    A.lambda = prob_.lambda;
    A.chunk_hdr = d_chunk_hdr_.as<int4>();
    A.chunk_img = d_chunk_img_.as<ChunkImg>();
    A.slab_pos = d_slab_pos_.as<int>();
    A.cam_pos = d_cam_pos_.as<int>();
    A.seg_hdr = d_seg_hdr_.as<int>();
    A.points = d_points_.as<double>();
    A.slab = d_slab_.as<double>();
    A.slab_b = d_slab_b_.as<double>();
    A.slab_cost = d_slab_cost_.as<double>();
    A.pose_old = d_pose_[cur_ ^ 1].as<double>();
    A.pose_new = d_pose_[cur_].as<double>();
    A.dc = d_dc_.as<double>();
    A.status = d_status_.as<int>();
    A.stamps = nullptr;
    A.huber = sess_.huber;
    A.huber2 = sess_.huber * sess_.huber;
    A.lm_lambda = lm_lambda_;
    return A;
  }

  // The pending step's landmark update alone (a back-substitute-only K1 under the delta the step
  // was solved with): no reduction, no collective, no synchronisation.
  void apply_pending() {
    if (!pending_) return;
    enqueue_lin(kBacksub);
    pending_ = false;
  }

  // What a K1 launch needs: its arguments (nseg set) and the chunks per segment of the one-wave
  // K1 (0: the four-wave K1).  False without segments (no landmarks: empty slabs, and the zero
  // cost is written here).
  struct K1Launch {
    LinArgs A;
    int wave_chunks;
  };
  bool prepare_k1(K1Launch& k) {
    const int nseg = plan_.n_segments();
    if (nseg <= 0) {
      VO_HIP_CHECK(hipMemsetAsync(d_slab_cost_.ptr, 0, 8, ctx_->stream));
      return false;
    }
    k.A = lin_args();
    // one-wave K1 for plans of one chunk per segment (the chunk image of segment s is chunk s)
    const bool wave = plan_is_wave(plan_.seg_obs);
    const int nw = wave ? plan_.seg_chunks : 1;
    VO_REQUIRE(!wave || ((int64_t)nseg * nw == plan_.n_chunks() && nw >= 1 && nw <= kWaveMaxChunks), VO_ERR_STATE,
               "K1: segments of seg_chunks chunks expected");
    k.A.nseg = nseg;
    k.wave_chunks = wave ? nw : 0;
    return true;
  }

  // mode: kBacksub | kAccum; the Huber instantiations are chosen in launch_k1 (a delta > 0).
  void enqueue_lin(int mode) {
    K1Launch k;
    if (!prepare_k1(k)) return enqueue_prior(d_status_.as<int>());
    ++launches_;
    ctx_->prof.begin(ctx_->stream, kKBaLin);
    if (stamps_on_) {  // one row per chunk (one-wave K1) or segment (four-wave K1)
      d_stamps_.reserve((size_t)plan_.n_chunks() * kPhCount * 8);
      k.A.stamps = d_stamps_.as<unsigned long long>();
    }
    // inside an LM run (lm_lambda_ set) the modes that use the damping read it from the device
    if (lm_lambda_ && mode != 0) mode |= kLm;
    launch_k1(k.A, mode, k.wave_chunks, "BA");
    ctx_->prof.end(ctx_->stream);
    VO_HIP_CHECK(hipGetLastError());
    enqueue_prior(k.A.status);
  }

  // A session with observation weights on a K1 layout without a weighted form: refused before
  // anything is enqueued or any run state is touched.
  void require_weighted_layout(const char* who) const {
    if (!sess_.weighted || plan_.n_segments() <= 0) return;
    const int nw = plan_is_wave(plan_.seg_obs) ? plan_.seg_chunks : 0;
    VO_REQUIRE(lin_weighted_covers(nw), VO_ERR_STATE,
               "%s: the session has observation weights, and its K1 layout (%s) has no weighted instantiation", who,
               nw ? "one-wave, too many chunks per segment" : "four-wave");
  }

  // K1 of one mode (kBacksub | kAccum | kLm) on the context stream: the Huber instantiations under
  // a robust cost, and for a session with observation weights the weighted ones (ba_weights.hip),
  // which exist for the one-wave K1 only -- any other layout refuses the run, it never drops the
  // weights.
  void launch_k1(LinArgs& A, int mode, int wave_chunks, const char* who) {
    if (!sess_.weighted) {
      launch_lin(A, sess_.huber > 0.0 ? mode | kRobust : mode, wave_chunks, A.nseg, ctx_->stream);
      return;
    }
    if (!(sess_.huber > 0.0)) {
      A.huber = kWeightedNoHuber;
      A.huber2 = kWeightedNoHuber * kWeightedNoHuber;
    }
    const bool ok = launch_lin_weighted(A, d_sqw_plan_.as<double>(), mode, wave_chunks, A.nseg, ctx_->stream);
    VO_REQUIRE(ok, VO_ERR_STATE,
               "%s: the session has observation weights, and this K1 layout (chunks per segment %d, mode %d) has no "
               "weighted instantiation",
               who, wave_chunks, mode);
  }

  // K2 runs inside the banded K3's launch (one rank: no all-reduce between them)
  bool fused() const { return fuse_ok_ && !ctx_->ba_split_reduce && !sharded(); }

  ReduceArgs reduce_args() const {
    const BAPlan& P = plan_;
    ReduceArgs R;
    R.nprof = P.n_prof_blocks();
    R.F = P.n_free;
    R.nseg = cost_entries();
    // damping on the camera diagonal: added once -- by rank 0 only when the partial
    // systems of the landmark shards are all-reduced
    R.lambda = (ctx_->comm && ctx_->comm->rank > 0) ? 0.0 : prob_.lambda;
    R.meta = d_red_meta_.as<int4>();
    R.out = d_red_out_.as<int2>();
    R.slab = d_slab_.as<double>();
    R.slab_b = d_slab_b_.as<double>();
    R.slab_cost = d_slab_cost_.as<double>();
    R.sys = d_sys_.as<double>();
    R.cost_off = red_.cost_off;
    R.status = d_status_.as<int>();
    R.lm_lambda = lm_lambda_;
    return R;
  }

  void enqueue_reduce() {
    if (fused()) return;  // K3's reducer workgroups do it
    const ReduceArgs R = reduce_args();
    ctx_->prof.begin(ctx_->stream, kKBaReduce);
    launch_reduce(R, R.nprof + 1, ctx_->stream);
    ctx_->prof.end(ctx_->stream);
    VO_HIP_CHECK(hipGetLastError());
    if (sharded())
      ctx_->comm->allreduce(d_sys_.as<double>(), red_.sys_len, false, ctx_->stream);
  }

  // K3 of one iteration (iter_tag: its 1-based number in the status word) on the context stream;
  // cost_slot, if set, receives the cost of its linearisation; chain_next: iteration().
  void enqueue_solve(int iter_tag, double* cost_slot = nullptr, bool chain_next = false) {
    ctx_->prof.begin(ctx_->stream, kKBaSolve);
    ++launches_;
    if (band_on_) enqueue_band_solve(iter_tag, cost_slot, chain_next);
    else enqueue_profile_solve(iter_tag, cost_slot);
    ctx_->prof.end(ctx_->stream);
    VO_HIP_CHECK(hipGetLastError());
  }

  void enqueue_band_solve(int iter_tag, double* cost_slot, bool chain_next) {
    const BAPlan& P = plan_;
    BandArgs B;
    B.F = P.n_free;
    B.w = band_.w;
    B.m = band_.m;
    B.nb = band_.nb;
    B.s = band_.s;
    B.nprof = P.n_prof_blocks();
    B.n_poses = P.n_poses;
    B.n_fixed = P.n_fixed;
    B.iter_tag = iter_tag;
    B.cost_off = red_.cost_off;
    B.merge = band_tab_.merge;
    B.n_merge = band_tab_.n_merge;
    B.tab = d_band_tab_.as<int>();
    B.sys = d_sys_.as<double>();
    B.zero = d_zero_.as<double>();
    B.fac = band_lds_.full && !band_lds_.split ? nullptr : d_fac_.as<double>();
    // split hand-off flags and the chained launch's publish word (seq << 1 | verdict): new every
    // launch, the low 31 bits never zero
    while ((++band_seq_ & 0x7fffffffu) == 0) {
    }
    B.seq = band_seq_;
    B.cost_out = cost_slot;
    B.dc = d_dc_.as<double>();
    B.pose_cur = d_pose_[cur_].as<double>();
    B.pose_next = d_pose_[cur_ ^ 1].as<double>();
    B.status = d_status_.as<int>();
    B.stamps = nullptr;
    B.nred = fused() ? band_fused_workgroups(B.nprof) : 0;
    B.red_drop = B.nred > 0 ? ctx_->ba_drop_reducers : 0;
    B.red_count = d_colcnt_.as<unsigned>();
    B.red_col = d_red_col_.as<int>();
    B.col_need = d_col_need_.as<int>();
    B.red = reduce_args();
    if (stamps_on_) {  // per wave phase cycles, then realtime stamps of the solver and each reducer
      d_stamps3_.reserve((8 * kBandStamps + 8 + 4 * (B.nred + 1)) * 8);
      B.stamps = d_stamps3_.as<unsigned long long>();
    }
    if (chain_next) {
      // the next iteration's K1 (iteration() flips cur_ behind this launch): its pending step's
      // linearisation point is this solve's input, its own the poses this solve writes
      B.lin = lin_args();
      std::swap(B.lin.pose_old, B.lin.pose_new);
      B.lin.nseg = B.k1_nseg = plan_.n_segments();
      B.pub_mask = (ctx_->ba_chain_poll ? ctx_->ba_chain_poll : kChainPollReplicas) - 1;
      B.pub = d_pub_.as<unsigned>();
      if (stamps_on_) {  // [published, launch start | start, prefix done, gate passed, end per K1 workgroup]
        d_stamps_k1_.reserve((2 + 4 * (size_t)B.k1_nseg) * 8);
        B.k1_stamps = d_stamps_k1_.as<unsigned long long>();
      }
    }
    launch_band_solve(B, band_lds_, ctx_->stream);
  }

  void enqueue_profile_solve(int iter_tag, double* cost_slot) {
    const BAPlan& P = plan_;
    SolveArgs A;
    A.F = P.n_free;
    A.nprof = P.n_prof_blocks();
    A.n_poses = P.n_poses;
    A.n_fixed = P.n_fixed;
    A.iter_tag = iter_tag;
    A.max_panel = solve_max_panel_;
    A.max_row_span = solve_max_row_span_;
    A.lds_kf = (long)solve_layout_.kf;
    A.lds_y = (long)solve_layout_.y;
    A.lds_panel = (long)solve_layout_.panel;
    A.lds_tab = (long)solve_layout_.tab;
    A.lds_pose = (long)solve_layout_.pose;
    A.tl = P.solve_layout;
    A.tab = d_solve_tab_.as<int>();
    A.cost_out = cost_slot;
    A.sys = d_sys_.as<double>();
    A.dc = d_dc_.as<double>();
    A.pose_cur = d_pose_[cur_].as<double>();
    A.pose_next = d_pose_[cur_ ^ 1].as<double>();
    A.status = d_status_.as<int>();
    A.stamps = nullptr;
    if (stamps_on_) {
      d_stamps3_.reserve(kS3Count * 8);
      A.stamps = d_stamps3_.as<unsigned long long>();
    }
    launch_profile_solve(A, solve_lds_, solve_lds_size_, ctx_->stream);
  }

  // lin_done: this iteration's K1 rode in the previous solve launch; chain_next: this solve
  // launch carries the next iteration's K1 (run()).
  void iteration(double* d_cost_slot, int iter_tag, bool lin_done = false, bool chain_next = false) {
    if (!lin_done) enqueue_lin(pending_ ? (kBacksub | kAccum) : kAccum);
    enqueue_reduce();
    enqueue_solve(iter_tag, d_cost_slot, chain_next);  // K3 also stores the cost (no extra copy node)
    cur_ ^= 1;
    pending_ = true;
  }

  // Whether a run's solve launches may carry the next iteration's K1: the
  // fused K2 + K3 launch of the full layout, a wave plan of six chunks per segment, every K1
  // workgroup resident beside the solver with a CU left for the reducers to pass through
  // (nseg + 2 <= CUs: the launch then completes under any dispatch order), one rank, and neither
  // kernel profiling nor stamps (a stamped build chains only when a tool asks for it).
  bool chain_ok() const {
    const int nseg = plan_.n_segments();
    return VO_BA_CHAIN && !ctx_->ba_no_chain && band_on_ && fused() && band_lds_.full && !band_lds_.split &&
           plan_is_wave(plan_.seg_obs) && plan_.seg_chunks == kBandChainChunks && nseg > 0 &&
           (int64_t)nseg * kBandChainChunks == plan_.n_chunks() && nseg + 2 <= ctx_->num_cus && !lm_lambda_ &&
           !sess_.weighted &&  // observation weights: the separate K1 launch (the chained K1 has no weighted form)
           !prior_k_ &&        // a pose prior: its kernel runs between K1 and the solve launch
           !sess_.n_factors &&  // pose factors: the same kernel
           !ctx_->prof.on && (!stamps_on_ || ctx_->ba_chain_stamps) && !sharded();
  }

  // Applies the pending point update (if any) and writes the cost at the
  // resulting state into d_cost_slot.
  void finalize_cost(double* d_cost_slot) {
    enqueue_lin(pending_ ? kBacksub : 0);
    pending_ = false;
    // cost-only reduction (S/b untouched): reuse K2's last block
    ReduceArgs R{};
    R.nprof = 0;
    R.F = 0;
    R.nseg = cost_entries();
    R.slab_cost = d_slab_cost_.as<double>();
    R.sys = d_cost_tmp();
    R.cost_off = 0;
    R.status = d_status_.as<int>();
    launch_reduce(R, 1, ctx_->stream);
    VO_HIP_CHECK(hipGetLastError());
    if (sharded())
      ctx_->comm->allreduce(R.sys, 1, false, ctx_->stream);
    VO_HIP_CHECK(hipMemcpyAsync(d_cost_slot, R.sys, 8, hipMemcpyDeviceToDevice, ctx_->stream));
  }

  void finalize() {
    if (!pending_) return;
    d_cost_.reserve(8);
    finalize_cost(d_cost_.as<double>());
    VO_HIP_CHECK(hipStreamSynchronize(ctx_->stream));
  }

  double* d_cost_tmp() {
    d_cost_tmp_.reserve(16);
    return d_cost_tmp_.as<double>();
  }

  vo_ctx* ctx_;
  BAPlan plan_{true};  // page-locked chunk images (async upload)
  BAPlan prev_plan_{true};  // the previous window's plan (group take-over), or scratch
  bool plan_ok_ = false;    // plan_ built and its images in d_chunk_img_
  int64_t setup_ns_[kSetupSections] = {};  // the last setup's host sections (vo_ba_plan_stats)
  vo_ba_problem prob_{};
  bool have_problem_ = false, have_state_ = false, pending_ = false, solve_lds_ = false;
  uint64_t session_ = 0;
  int cur_ = 0;
  size_t solve_lds_size_ = 0;
  int solve_max_panel_ = 1, solve_max_row_span_ = 0;  // the profile K3's SolveArgs constants (setup)
  SolveLds solve_layout_{};
  BandSplit band_{};
  bool band_on_ = false;
  bool fuse_ok_ = false;  // K2 fused into K3's launch (see fused())
  unsigned band_seq_ = 0;  // split-mode K3 launches so far (their hand-off flag values)
  BandLds band_lds_;
  BandTables band_tab_;
  // the plan's small tables (one upload per setup) and the views into them
  HostBuf h_tab_;
  DevBuf d_tab_;
  DevView d_chunk_hdr_, d_seg_hdr_, d_slab_pos_, d_cam_pos_, d_solve_tab_, d_band_tab_, d_red_meta_, d_red_out_;
  static constexpr size_t kMiscBytes = 256 + 512;
  DevBuf d_misc_;  // [status | zero block (512 B)]
  DevView d_status_, d_zero_;
  DevBuf d_colcnt_;  // the fused launch's column readiness counters (band_col_count_bytes)
  DevBuf d_pub_;     // the chained launches' publish word (kBandPubReplicas lines)
  DevBuf d_stamps_k1_;  // diagnostic build: the chained K1 workgroups' realtime stamps
  // replicas of the publish word the K1 workgroups poll (one word against eight)
  static constexpr int kChainPollReplicas = VO_BA_CHAIN_POLL;
  bool last_chained_ = false;  // the last run(): chained, and the solve launches it made
  int last_launches_ = 0, launches_ = 0;
  size_t colcnt_bytes_ = 0;
  DevView d_red_col_, d_col_need_;
  ReduceLayout red_;  // K2's output layout and tables (host copies: gn_step, covariance)
  std::vector<ImageRun> img_runs_;  // upload_images' runs
  DevBuf d_fac_;
  HostBuf h_state_;  // page-locked staging of set_state / get_state
  hipEvent_t h_state_ev_ = nullptr;  // set_state's upload from h_state_ done
  bool h_state_busy_ = false;
  DevBuf d_chunk_img_;  // K1's plan (the chunk images hold every list)
  DevBuf d_chunk_img_prev_;  // the previous plan's images (prev_plan_)
  DevBuf d_stamps_, d_stamps3_;
  static constexpr bool stamps_on_ = kBaStamps;

 public:
  // Diagnostic: per-phase cycle sums of the last K1 launch (VO_BA_STAMPS=1 builds).
  int read_stamps(uint64_t* out, int n) {
    if (!stamps_on_) return 0;
    // rows: chunks of a wave plan, segments of a four-wave plan
    const int nseg = plan_is_wave(plan_.seg_obs) ? plan_.n_chunks() : plan_.n_segments();
    std::vector<unsigned long long> h((size_t)nseg * kPhCount);
    VO_HIP_CHECK(hipStreamSynchronize(ctx_->stream));
    VO_HIP_CHECK(hipMemcpy(h.data(), d_stamps_.ptr, h.size() * 8, hipMemcpyDeviceToHost));
    if (n < 0) {  // raw per-segment rows (kPhCount values each; the last two are absolute times)
      const int k = std::min<int>(-n, (int)h.size());
      std::copy(h.begin(), h.begin() + k, out);
      return k;
    }
    int k = std::min(n, (int)kPhCount);
    for (int i = 0; i < k; ++i) {
      uint64_t acc = 0;
      for (int g = 0; g < nseg; ++g) acc += h[(size_t)g * kPhCount + i];
      out[i] = acc;
    }
    const int n3 = band_on_ ? 8 * kBandStamps : (int)kS3Count;  // K3: banded or profile solver
    if (n >= kPhCount + n3 && d_stamps3_.ptr) {
      // the banded solver's realtime stamps follow when the caller asked for them (fused launch)
      const int nx = band_on_ && fused() ? 8 + 4 * (band_fused_workgroups(plan_.n_prof_blocks()) + 1) : 0;
      const int n3x = n >= kPhCount + n3 + nx ? n3 + nx : n3;
      VO_HIP_CHECK(hipMemcpy(out + kPhCount, d_stamps3_.ptr, n3x * 8, hipMemcpyDeviceToHost));
      k += n3x;
    }
    return k;
  }

 private:
  DevBuf d_points_, d_pose_[2], d_dc_, d_slab_, d_slab_b_, d_slab_cost_, d_sys_;
  DevBuf d_cost_, d_cost_tmp_;
  // What belongs to the current problem and to nothing else: setup() starts every session from
  // Session{}, so nothing here outlives its problem.
  struct LmRun {  // the last vo_ba_run_lm, as lm_read needs it
    int iters = -1;  // -1: no LM run on this session yet
    int fail = 0;    // the failed iteration (1-based), 0: none
    bool timeout = false, unread = false;
    // termination: whether the run tested a criterion, and how it ended (settled at its first read)
    bool stop_on = false;
    int trials = 0, reason = VO_BA_LM_RAN_ALL;
  };
  struct Session {
    double huber = 0.0;  // Huber delta in pixels, 0: plain cost (set_robust)
    // observation weights (set_obs_weights, cull): whether the session has any (false: every
    // launch is the unweighted one, every observation at weight 1)
    bool weighted = false;
    // the lazy tables, each sent on the session's first call that needs it: upload_obs,
    // upload_cov_tables, upload_weight_tables
    bool obs_uploaded = false, cov_uploaded = false, wt_tables = false;
    vo_ba_lm_stop lm_stop{};  // the LM runs' termination criteria (all zero: never stop)
    LmRun lm;
    int n_factors = 0;  // the session's pose factors (setup; their device arrays in d_factors_)
  };
  Session sess_;
  // the session's pose prior (setup): its size (0: none), cost0 and device arrays (upload_prior)
  int prior_k_ = 0;
  bool prior_staged_ = false;
  double prior_cost0_ = 0.0;
  DevBuf d_prior_;
  DevBuf d_factors_;
  DevBuf d_marg_;  // marginalize()'s scratch
  // step control (run_lm): the damping's device address while an LM run enqueues its kernels
  // (null otherwise: the GN kernels), the log and the landmark snapshot
  const double* lm_lambda_ = nullptr;
  DevBuf d_lm_log_, d_lm_snap_;
  // residuals(): the problem-order observation arrays and its output [err2 | depth]
  DevBuf d_obs_cam_, d_obs_pt_, d_obs_uv_, d_obs_out_;
  // covariance(): its tables, the dense factor and inverse of S, the landmark blocks and the
  // factorisation's failure word
  DevBuf d_cov_ptr_, d_cov_inv_, d_cov_first_, d_cov_off_, d_cov_last_, d_cov_dst_;
  DevBuf d_cov_l_, d_cov_, d_cov_pts_, d_cov_fail_;
  // observation weights: w and sqrt(w) in problem order, sqrt(w) in the plan's order (K1), the
  // problem observation -> plan position map and the cull's two counters
  DevBuf d_w_, d_sqw_obs_, d_sqw_plan_, d_obs_pos_, d_cull_cnt_;
  // host sources of the read-outs' and the cull's tables (upload_obs, upload_cov_tables,
  // upload_weight_tables): kept for the session, so their copies need no synchronisation
  std::vector<int32_t> h_obs_cam_, h_obs_pt_, h_cov_ptr_, h_cov_inv_, h_obs_pos_;
  std::vector<float> h_obs_uv_;
};

// ---- entry points used by api.hip -------------------------------------------------
BAEngine* ba_engine(vo_ctx* ctx) {
  if (!ctx->ba) ctx->ba.reset(new BAEngine(ctx));
  return ctx->ba.get();
}
uint64_t ba_setup(vo_ctx* ctx, const vo_ba_problem* p, const vo_ba_pose_prior* prior, const vo_ba_pose_factor* factors,
                  int n_factors) {
  return ba_engine(ctx)->setup(p, prior, factors, n_factors);
}
void ba_reserve(vo_ctx* ctx, int n_poses, int n_points, int64_t n_obs, int n_fixed) {
  ba_engine(ctx)->reserve(n_poses, n_points, n_obs, n_fixed);
}
void ba_check_session(vo_ctx* ctx, uint64_t s) { ba_engine(ctx)->check_session(s); }
void ba_set_state(vo_ctx* ctx, const double* poses, const double* pts) {
  ba_engine(ctx)->set_state(poses, pts);
}
void ba_get_state(vo_ctx* ctx, double* poses, double* pts) { ba_engine(ctx)->get_state(poses, pts); }
int ba_run(vo_ctx* ctx, int iters, double* cost, bool sync) { return ba_engine(ctx)->run(iters, cost, sync); }
int ba_gn_step(vo_ctx* ctx, double* S, double* b, double* dc, double* cost) {
  return ba_engine(ctx)->gn_step(S, b, dc, cost);
}
int ba_run_lm(vo_ctx* ctx, int iters, const vo_ba_lm_options* opt, double* cost, double* lambda, double* trial,
              uint8_t* accepted, bool sync) {
  return ba_engine(ctx)->run_lm(iters, opt, cost, lambda, trial, accepted, sync);
}
int ba_lm_log(vo_ctx* ctx, int n, double* cost, double* lambda, double* trial, uint8_t* accepted) {
  return ba_engine(ctx)->lm_read(n, cost, lambda, trial, accepted, "vo_ba_lm_log");
}
void ba_set_lm_stop(vo_ctx* ctx, const vo_ba_lm_stop* stop) { ba_engine(ctx)->set_lm_stop(stop); }
void ba_lm_stop_info(vo_ctx* ctx, int32_t* trials, int32_t* reason) { ba_engine(ctx)->lm_stop_info(trials, reason); }
void ba_set_robust(vo_ctx* ctx, double delta) { ba_engine(ctx)->set_robust(delta); }
void ba_residuals(vo_ctx* ctx, double* err2, double* depth) { ba_engine(ctx)->residuals(err2, depth); }
int ba_marginalize(vo_ctx* ctx, int n_drop, double lambda, int32_t* n_prior, double* info, double* rhs, double* poses0,
                   double* cost0, uint8_t* mask) {
  return ba_engine(ctx)->marginalize(n_drop, lambda, n_prior, info, rhs, poses0, cost0, mask);
}
int ba_covariance(vo_ctx* ctx, double lambda, double* pose_cov, double* pose_dense, double* point_cov) {
  return ba_engine(ctx)->covariance(lambda, pose_cov, pose_dense, point_cov);
}
void ba_set_obs_weights(vo_ctx* ctx, const double* w) { ba_engine(ctx)->set_obs_weights(w); }
void ba_get_obs_weights(vo_ctx* ctx, double* w_out) { ba_engine(ctx)->get_obs_weights(w_out); }
void ba_cull(vo_ctx* ctx, const vo_ba_cull_options* opt, int32_t* n_culled, int32_t* n_active, bool sync) {
  ba_engine(ctx)->cull(opt, n_culled, n_active, sync);
}
int ba_stats(vo_ctx* ctx, int64_t* out, int n) { return ba_engine(ctx)->stats(out, n); }
int ba_stamps(vo_ctx* ctx, uint64_t* out, int n) { return ba_engine(ctx)->read_stamps(out, n); }
int ba_chain_stamps(vo_ctx* ctx, uint64_t* out, int n) { return ba_engine(ctx)->read_chain_stamps(out, n); }
void ba_last_run(vo_ctx* ctx, int* chained, int* launches) { ba_engine(ctx)->last_run(chained, launches); }

}  // namespace vo

vo_ctx::vo_ctx() = default;

vo_ctx::~vo_ctx() {
  ba.reset();
  comm.reset();
  if (stream) (void)hipStreamDestroy(stream);
}
