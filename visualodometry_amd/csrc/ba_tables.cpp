// The BA engine's host arithmetic (ba_tables.h).
#include "ba_tables.h"

#include <cmath>

namespace vo {

void reduce_layout(const BAPlan& P, bool band_on, int w, int top, int col_stride, ReduceLayout& L) {
  const int F = P.n_free, nprof = P.n_prof_blocks();
  L.dst.assign(std::max(1, nprof), 0);
  L.rdst.assign(std::max(1, F), 0);
  if (band_on) {
    const int CS = col_stride;
    const int s = top < F ? w : 0;  // the separator: w rows of a two-sided split, none one-sided (top = F)
    const int base_b = top * CS;
    for (int i = 0; i < F; ++i) {
      for (int j = P.prof_first[i]; j <= i; ++j) {
        const int b = P.prof_off[i] + j - P.prof_first[i];
        L.dst[b] = i < top ? j * CS + 36 * (i - j) : (base_b + (F - 1 - i) * CS + 36 * (i - j)) | kTabTranspose;
      }
      L.rdst[i] = i < top ? i * CS + 36 * (w + 1) : base_b + (F - 1 - i) * CS + 36 * (w + 1);
    }
    L.sys_len = (size_t)(F + s) * CS + 1;
    L.cost_off = (long)L.sys_len - 1;
  } else {
    for (int b = 0; b < nprof; ++b) L.dst[b] = 36 * b;
    for (int f = 0; f < F; ++f) L.rdst[f] = 36 * nprof + 6 * f;
    L.sys_len = 36ull * nprof + 6ull * F + 1;
    L.cost_off = (long)L.sys_len - 1;
  }
  // K2's per-block table: slab rows, the diagonal blocks' rhs entries, output offsets
  L.meta.assign(4 * (size_t)std::max(1, nprof), 0);
  L.meta[2] = L.meta[3] = -1;
  L.out.assign(2 * (size_t)std::max(1, nprof), 0);
  for (int i = 0; i < F; ++i)
    for (int b = P.prof_off[i]; b < P.prof_off[i + 1]; ++b) {
      const bool diag = P.prof_diag[b] != 0;
      int32_t* m = &L.meta[4 * (size_t)b];
      m[0] = P.prof_src_ptr[b];
      m[1] = P.prof_src_ptr[b + 1];
      m[2] = diag ? P.camb_ptr[i] : -1;
      m[3] = diag ? P.camb_ptr[i + 1] : -1;
      L.out[2 * (size_t)b] = L.dst[b];
      L.out[2 * (size_t)b + 1] = diag ? L.rdst[i] : 0;
    }
  L.col.assign(std::max(1, nprof), 0);
  L.col_need.assign(F + 1, 0);
  if (band_on) {
    for (int i = 0; i < F; ++i)
      for (int b = P.prof_off[i]; b < P.prof_off[i + 1]; ++b) {
        const int j = P.prof_first[i] + (b - P.prof_off[i]);
        L.col[b] = i < top ? j : top + (F - 1 - i);
        ++L.col_need[L.col[b]];
      }
    L.col_need[F] = 1;  // the cost item
  }
}

void dense_system(const BAPlan& P, const ReduceLayout& L, const double* sys, double* S_out, double* b_out) {
  const int F = P.n_free;
  if (S_out) {
    const int n = 6 * F;
    std::fill(S_out, S_out + (size_t)n * n, 0.0);
    for (int i = 0; i < F; ++i)
      for (int j = P.prof_first[i]; j <= i; ++j) {
        const int d = L.dst[P.prof_off[i] + j - P.prof_first[i]];
        const double* blk = sys + (d & ~kTabTranspose);
        const bool tr = d & kTabTranspose;
        for (int r = 0; r < 6; ++r)
          for (int c = 0; c < 6; ++c) {
            const double v = blk[tr ? 6 * c + r : 6 * r + c];
            S_out[(size_t)(6 * i + r) * n + 6 * j + c] = v;
            S_out[(size_t)(6 * j + c) * n + 6 * i + r] = v;
          }
      }
  }
  if (b_out)
    for (int f = 0; f < F; ++f) std::copy(sys + L.rdst[f], sys + L.rdst[f] + 6, b_out + 6 * f);
}

void obs_tables(const BAPlan& P, std::vector<int32_t>& cam, std::vector<int32_t>& pt, std::vector<float>& uv) {
  const size_t M = (size_t)P.n_obs;
  cam.resize(M);
  pt.resize(M);
  uv.resize(2 * M);
  for (size_t pos = 0; pos < M; ++pos) {  // internal position -> problem observation (ba_plan.h)
    const size_t o = (size_t)P.obs_order[pos];
    cam[o] = P.obs_cam[pos];
    pt[o] = P.te_pt[P.obs_te[pos]];
    uv[2 * o] = P.obs_uv[2 * pos];
    uv[2 * o + 1] = P.obs_uv[2 * pos + 1];
  }
}

void csr_tables(const BAPlan& P, std::vector<int32_t>& ptr, std::vector<int32_t>& inv) {
  const size_t M = (size_t)P.n_obs;
  ptr.assign(P.n_points + 1, 0);
  inv.assign(std::max(1, P.n_points), 0);
  for (int q = 0; q < P.n_points; ++q) inv[P.pt_perm[q]] = q;
  for (size_t pos = 0; pos < M; ++pos) ++ptr[P.pt_perm[P.te_pt[P.obs_te[pos]]] + 1];
  for (int p = 0; p < P.n_points; ++p) ptr[p + 1] += ptr[p];
}

void obs_positions(const BAPlan& P, std::vector<int32_t>& pos_of) {
  const size_t M = (size_t)P.n_obs;
  pos_of.assign(std::max<size_t>(M, 1), 0);
  for (size_t pos = 0; pos < M; ++pos) pos_of[(size_t)P.obs_order[pos]] = (int32_t)pos;
}

void image_runs(const BAPlan& P, std::vector<ImageRun>& runs) {
  const int nch = (int)P.chunk_img.size();
  runs.clear();
  for (int c0 = 0; c0 < nch;) {
    const int src = P.chunk_src[c0];
    int c1 = c0 + 1;
    while (c1 < nch && (src < 0 ? P.chunk_src[c1] < 0 : P.chunk_src[c1] == src + (c1 - c0))) ++c1;
    runs.push_back({src < 0 ? -1 : src, c0, c1 - c0});
    c0 = c1;
  }
}

ReserveWindow reserve_window(int n_poses, int n_points, int64_t n_obs) {
  const int len0 = (int)std::min<int64_t>(n_poses, n_obs / n_points);
  const int64_t extra = std::min<int64_t>(n_obs - (int64_t)len0 * n_points, n_points);
  ReserveWindow W;
  std::vector<int32_t>&ptr = W.point_ptr, &cam = W.obs_cam;
  ptr.assign(n_points + 1, 0);
  cam.reserve(n_obs);
  for (int p = 0; p < n_points; ++p) {
    const int len = std::min(n_poses, len0 + (p < extra ? 1 : 0));
    const int c0 = (int)((int64_t)p * (n_poses - len + 1) / n_points);
    for (int c = 0; c < len; ++c) cam.push_back(c0 + c);
    ptr[p + 1] = (int32_t)cam.size();
  }
  return W;
}

void LmLog::decode(const double* doubles, const int* acc, int n_asked, int f, bool stopped, double* cost_out,
                   double* lambda_out, double* trial_out, uint8_t* accepted_out) const {
  const double *cost = doubles, *lam = cost + n + 1, *trial = lam + n + 1;
  for (int k = 0; k <= n_asked; ++k) {
    if (cost_out) cost_out[k] = k <= f ? cost[k] : stopped ? cost[f] : NAN;
    if (lambda_out) lambda_out[k] = k <= f ? lam[k] : stopped ? lam[f] : NAN;
  }
  for (int k = 0; k < n_asked; ++k) {
    if (trial_out) trial_out[k] = k < f ? trial[k] : NAN;
    if (accepted_out) accepted_out[k] = k < f && acc[k] ? 1 : 0;
  }
}

std::string lm_options(const vo_ba_lm_options* opt, double problem_lambda, vo_ba_lm_options& o) {
  o = opt ? *opt : vo_ba_lm_options{};
  if (!(std::isfinite(o.lambda0) && std::isfinite(o.up) && std::isfinite(o.down) && std::isfinite(o.lambda_min) &&
        std::isfinite(o.lambda_max)))
    return "vo_ba_run_lm: non-finite option";
  if (o.up == 0.0) o.up = 10.0;
  if (o.down == 0.0) o.down = 0.1;
  if (o.lambda_min == 0.0) o.lambda_min = 1e-6;
  if (o.lambda_max == 0.0) o.lambda_max = 1e6;
  if (o.lambda0 == 0.0) o.lambda0 = problem_lambda > 0.0 ? problem_lambda : 1e-4;
  if (!(o.lambda0 >= 0.0)) return "vo_ba_run_lm: lambda0 < 0";
  if (!(o.up > 1.0)) return "vo_ba_run_lm: up must be > 1";
  if (!(o.down > 0.0 && o.down < 1.0)) return "vo_ba_run_lm: down must be in (0, 1)";
  if (!(o.lambda_min > 0.0 && o.lambda_min <= o.lambda_max)) return "vo_ba_run_lm: need 0 < lambda_min <= lambda_max";
  o.lambda0 = std::min(std::max(o.lambda0, o.lambda_min), o.lambda_max);
  return "";
}

std::string pose_prior_error(const vo_ba_problem* prob, const vo_ba_pose_prior* pr) {
  if (!prob || !pr) return "vo_ba_setup_prior: null problem or prior";
  if (pr->reserved != 0) return "vo_ba_setup_prior: reserved must be 0";
  if (pr->n_poses < 1) return "vo_ba_setup_prior: a prior covers at least one pose";
  if (prob->n_fixed < 0 || pr->n_poses > prob->n_poses - prob->n_fixed)
    return "vo_ba_setup_prior: the prior covers more poses than the window has free";
  if (!pr->info || !pr->rhs || !pr->poses0) return "vo_ba_setup_prior: null arrays";
  const size_t n = 6ull * pr->n_poses;
  if (!std::isfinite(pr->cost0)) return "vo_ba_setup_prior: cost0 is not finite";
  for (size_t r = 0; r < n; ++r) {
    if (!std::isfinite(pr->rhs[r])) return "vo_ba_setup_prior: rhs is not finite";
    for (size_t c = 0; c <= r; ++c)  // (the upper triangle is not read)
      if (!std::isfinite(pr->info[r * n + c])) return "vo_ba_setup_prior: info is not finite";
  }
  for (size_t e = 0; e < 2 * n; ++e)
    if (!std::isfinite(pr->poses0[e])) return "vo_ba_setup_prior: poses0 is not finite";
  return "";
}

std::string pose_factor_error(const vo_ba_problem* prob, const vo_ba_pose_factor* fs, int n) {
  if (!prob) return "vo_ba_setup_factors: null problem";
  if (n < 0) return "vo_ba_setup_factors: n_factors < 0";
  if (n > 0 && !fs) return "vo_ba_setup_factors: null factors";
  if (n > VO_BA_MAX_POSE_FACTORS)
    return "vo_ba_setup_factors: more than " + std::to_string(VO_BA_MAX_POSE_FACTORS) + " factors";
  for (int k = 0; k < n; ++k) {
    const vo_ba_pose_factor& f = fs[k];
    const std::string at = "vo_ba_setup_factors: factor " + std::to_string(k) + ": ";
    if (f.cam_i < 0 || f.cam_i >= prob->n_poses || f.cam_j >= prob->n_poses) return at + "camera out of range";
    if (f.cam_j < -1) return at + "cam_j must be a camera or -1";
    if (f.cam_i == f.cam_j) return at + "cam_i == cam_j";
    for (double v : f.meas)
      if (!std::isfinite(v)) return at + "meas is not finite";
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c <= r; ++c)  // (the upper triangle is not read)
        if (!std::isfinite(f.info[6 * r + c])) return at + "info is not finite";
  }
  return "";
}

void factor_free_cams(int n_fixed, const vo_ba_pose_factor* fs, int n, FactorRows& R) {
  R.fi.resize(std::max(0, n));
  R.fj.resize(std::max(0, n));
  R.rows.clear();
  for (int k = 0; k < n; ++k) {
    R.fi[k] = fs[k].cam_i >= n_fixed ? fs[k].cam_i - n_fixed : -1;
    R.fj[k] = fs[k].cam_j >= n_fixed ? fs[k].cam_j - n_fixed : -1;
  }
}

void factor_lower_first(const FactorRows& R, std::vector<int32_t>& first) {
  for (size_t k = 0; k < R.fi.size(); ++k)
    if (R.fi[k] >= 0 && R.fj[k] >= 0) {
      const int hi = std::max(R.fi[k], R.fj[k]), lo = std::min(R.fi[k], R.fj[k]);
      first[hi] = std::min(first[hi], lo);
    }
}

std::string plan_window(BAPlan& P, const vo_ba_problem* prob, int seg_obs, const BAPlan* prev, int seg_chunks) {
  const int32_t zero = 0;
  const std::string err = build_plan(P, prob->n_poses, prob->n_points, prob->n_obs, prob->n_fixed,
                                     prob->n_points ? prob->point_ptr : &zero, prob->obs_cam, prob->obs_uv, seg_obs, prev,
                                     seg_chunks);
  if (err.empty()) build_profile(P, local_profile_first(P));
  return err;
}

static std::string obs_pt_error(int o, int32_t p) {
  return "vo_ba_group_by_point: obs_pt[" + std::to_string(o) + "]=" + std::to_string(p) + " out of range";
}

std::string group_by_point(int n_points, int n_obs, const int32_t* obs_pt, int32_t* order, int32_t* point_ptr,
                           bool& grouped) {
  grouped = true;
  if (n_points < 0 || n_obs < 0) return "vo_ba_group_by_point: bad sizes";
  if (!point_ptr || (n_obs != 0 && !obs_pt)) return "vo_ba_group_by_point: null argument";
  if (!order) {  // already grouped (nondecreasing obs_pt)?  then only point_ptr
    const int32_t* __restrict op = obs_pt;
    int32_t* __restrict pp = point_ptr;
    unsigned descending = 0;  // branch-free scan
    for (int o = 1; o < n_obs; ++o) descending |= op[o] < op[o - 1];
    // nondecreasing: in range iff the ends are; otherwise every entry is checked
    unsigned out_of_range = n_obs > 0 && ((unsigned)op[0] >= (unsigned)n_points ||
                                          (unsigned)op[n_obs - 1] >= (unsigned)n_points);
    if (descending)
      for (int o = 0; o < n_obs; ++o) out_of_range |= (unsigned)op[o] >= (unsigned)n_points;
    if (out_of_range) {
      int o = 0;
      while ((unsigned)op[o] < (unsigned)n_points) ++o;
      return obs_pt_error(o, op[o]);
    }
    if (descending) {
      grouped = false;
      return "";
    }
    // grouped: landmark p's run starts at its first observation, or (none) where the next
    // landmark's does.  Branch-free, and no per-observation read-modify-write: the first
    // observations stored from the back, then a running minimum from the last landmark.
    std::fill(pp, pp + n_points + 1, n_obs);
    for (int o = n_obs - 1; o >= 0; --o) pp[op[o]] = o;
    int run = n_obs;
    for (int p = n_points - 1; p >= 0; --p) {
      run = std::min(run, pp[p]);
      pp[p] = run;
    }
    return "";
  }
  std::fill(point_ptr, point_ptr + n_points + 1, 0);
  for (int o = 0; o < n_obs; ++o) {
    if (obs_pt[o] < 0 || obs_pt[o] >= n_points) return obs_pt_error(o, obs_pt[o]);
    ++point_ptr[obs_pt[o] + 1];
  }
  for (int p = 0; p < n_points; ++p) point_ptr[p + 1] += point_ptr[p];
  std::vector<int32_t> next(point_ptr, point_ptr + std::max(n_points, 1));
  for (int o = 0; o < n_obs; ++o) order[next[obs_pt[o]]++] = o;  // stable: caller order within a landmark
  return "";
}

}  // namespace vo
