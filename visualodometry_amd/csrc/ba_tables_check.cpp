// Host check of the BA engine's host tables (ba_tables.h; tests/test_ba_tables.py): plans a
// window as the engine does (build_plan, local_profile_first, build_profile) and checks
//   - the problem-order observation tables, CSR and position map against the caller's arrays;
//   - K2's output layout for the profile solver, the banded solver one-sided and (F >= 2 w + 2)
//     two-sided: no overlap, everything inside [0, sys_len - 1), meta / out consistent with the
//     plan, the readiness counts, and dense_system's round trip through each layout;
//   - image_runs over a scratch plan and over the same window planned again on top of it;
//   - reserve_window on fixed sizes, LmLog's layout and decoding, lm_options' defaults.
// Input (binary): int32 n_poses, n_points, n_obs, n_fixed, seg_obs; point_ptr; obs_cam; obs_uv.
// Optional argv[2]: seg_chunks (wave plans; default 1).
// Optional argv[3] "factors" (tests/test_ba_factor_tables.py): the pose factors' host tables instead
// -- an empty factor list leaves every profile array and the digest as they are; a chain over all
// cameras with a duplicate pair and a unary factor keeps the bandwidth; one more factor between the
// first and the last free pose spans F - 1; every factor row lies in its block's (camera's) source
// range behind K1's sources and ahead of the prior's, none twice; the argument checks and the
// marginalisation's mask rule.  Prints "factors ok <free poses> <bandwidth> <with the chain> <with
// the far factor> <factor slab rows>".
// argv[1] "group" (no input file): group_by_point on small fixed inputs against a counting loop --
// grouped input with empty landmarks at both ends and in the middle, ungrouped input with and
// without order, out-of-range entries at the first, the last and a middle position, no
// observations, no landmarks, the argument checks.  Prints "group ok".
// Prints "ok <free poses> <bandwidth> <layouts checked> <chunks> <chunks taken over>" or the
// first violation.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ba_plan.h"
#include "ba_tables.h"

namespace vo {
void* plan_host_alloc(size_t b, bool) { return ::operator new(b < 64 ? 64 : b, std::align_val_t(64)); }
void plan_host_free(void* p, bool) noexcept {
  if (p) ::operator delete(p, std::align_val_t(64));
}
}  // namespace vo

#define FAIL(...)                      \
  do {                                 \
    std::printf("fail: " __VA_ARGS__); \
    std::printf("\n");                 \
    return false;                      \
  } while (0)

using vo::BAPlan;

static bool check_obs(const BAPlan& P, const std::vector<int32_t>& ptr, const std::vector<int32_t>& cam,
                      const std::vector<float>& uv) {
  const size_t M = cam.size();
  const int L = (int)ptr.size() - 1;
  if (P.obs_order.size() != M) FAIL("obs_order has %zu entries of %zu", P.obs_order.size(), M);
  std::vector<char> seen(M, 0);
  for (size_t pos = 0; pos < M; ++pos) {
    const int32_t o = P.obs_order[pos];
    if (o < 0 || (size_t)o >= M || seen[o]) FAIL("obs_order is no permutation at position %zu", pos);
    seen[o] = 1;
  }
  std::vector<int32_t> c, pt, p2, inv, pos_of;
  std::vector<float> u;
  vo::obs_tables(P, c, pt, u);
  if (c != cam) FAIL("obs_tables: cam differs from the problem's obs_cam");
  if (u != uv) FAIL("obs_tables: uv differs from the problem's obs_uv");
  if (pt.size() != M) FAIL("obs_tables: pt size");
  for (int p = 0; p < L; ++p)
    for (int o = ptr[p]; o < ptr[p + 1]; ++o)
      if (pt[o] < 0 || pt[o] >= L || P.pt_perm[pt[o]] != p) FAIL("obs_tables: observation %d is not landmark %d's", o, p);
  vo::csr_tables(P, p2, inv);
  if (p2 != ptr) FAIL("csr_tables: ptr differs from the problem's point_ptr");
  if ((int)inv.size() != std::max(1, L)) FAIL("csr_tables: inv size");
  for (int q = 0; q < L; ++q)
    if (inv[P.pt_perm[q]] != q) FAIL("csr_tables: inv is not the inverse of pt_perm at %d", q);
  vo::obs_positions(P, pos_of);
  if (pos_of.size() != std::max<size_t>(M, 1)) FAIL("obs_positions: size");
  for (size_t pos = 0; pos < M; ++pos)
    if (pos_of[P.obs_order[pos]] != (int32_t)pos) FAIL("obs_positions: not the inverse of obs_order at %zu", pos);
  return true;
}

// The value of entry (r, c) of block (i, j) in the round trip (diagonal blocks symmetric, as S's are).
static double enc(int F, int i, int j, int r, int c) {
  if (i == j && r < c) std::swap(r, c);
  return 1.0 + 36.0 * ((double)i * F + j) + 6 * r + c;
}

static bool check_layout(const BAPlan& P, bool band_on, int w, int top, const char* what) {
  const int F = P.n_free, nprof = P.n_prof_blocks(), CS = 36 * (w + 1) + 12;  // band_col_stride(w)
  vo::ReduceLayout L;
  vo::reduce_layout(P, band_on, w, top, CS, L);
  if (L.sys_len < 1 || L.cost_off != (long)L.sys_len - 1) FAIL("%s: cost_off %ld, sys_len %zu", what, L.cost_off, L.sys_len);
  const long end = (long)L.sys_len - 1;
  const size_t nb = (size_t)std::max(1, nprof);
  if (L.dst.size() != nb || L.rdst.size() != (size_t)std::max(1, F) || L.meta.size() != 4 * nb || L.out.size() != 2 * nb ||
      L.col.size() != nb || L.col_need.size() != (size_t)F + 1)
    FAIL("%s: table sizes", what);
  std::vector<char> used(end, 0);
  auto claim = [&](long at, int n) {
    if (at < 0 || at + n > end) return false;
    for (int k = 0; k < n; ++k) {
      if (used[at + k]) return false;
      used[at + k] = 1;
    }
    return true;
  };
  std::vector<double> sys(L.sys_len, 0.0);
  for (int i = 0; i < F; ++i) {
    if (P.prof_off[i + 1] - P.prof_off[i] != i - P.prof_first[i] + 1) FAIL("%s: profile row %d", what, i);
    for (int b = P.prof_off[i]; b < P.prof_off[i + 1]; ++b) {
      const int j = P.prof_first[i] + (b - P.prof_off[i]);
      const bool diag = i == j, tr = L.dst[b] & vo::kTabTranspose;
      const long d = L.dst[b] & ~vo::kTabTranspose;
      if ((P.prof_diag[b] != 0) != diag) FAIL("%s: prof_diag of block (%d, %d)", what, i, j);
      if (!claim(d, 36)) FAIL("%s: block (%d, %d) at %ld overlaps or leaves [0, %ld)", what, i, j, d, end);
      // ba_band.h: column v of a side holds block (v + q, v) of the side's coordinates at 36 q, the
      // bottom side's (rows and columns counted from F - 1 down, behind the top columns) transposed
      if (band_on && (tr != (i >= top) || d != (i < top ? (long)j * CS : (long)(top + F - 1 - i) * CS) + 36 * (i - j)))
        FAIL("%s: block (%d, %d) at %ld%s is not where the banded solver reads it", what, i, j, d, tr ? " (transposed)" : "");
      if (band_on && L.col[b] != d / CS) FAIL("%s: block (%d, %d) counts in column %d, stored in %ld", what, i, j, L.col[b], d / CS);
      if (!band_on && (tr || d != 36L * b)) FAIL("%s: block (%d, %d) at %ld", what, i, j, d);
      const int32_t* m = &L.meta[4 * (size_t)b];
      if (m[0] != P.prof_src_ptr[b] || m[1] != P.prof_src_ptr[b + 1] || m[2] != (diag ? P.camb_ptr[i] : -1) ||
          m[3] != (diag ? P.camb_ptr[i + 1] : -1))
        FAIL("%s: meta of block (%d, %d)", what, i, j);
      if (L.out[2 * (size_t)b] != L.dst[b] || L.out[2 * (size_t)b + 1] != (diag ? L.rdst[i] : 0))
        FAIL("%s: out of block (%d, %d)", what, i, j);
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) sys[d + (tr ? 6 * c + r : 6 * r + c)] = enc(F, i, j, r, c);
    }
    if (!claim(L.rdst[i], 6)) FAIL("%s: rhs row %d at %d overlaps or leaves [0, %ld)", what, i, L.rdst[i], end);
    if (L.rdst[i] != (band_on ? (i < top ? i : top + F - 1 - i) * CS + 36 * (w + 1) : 36 * nprof + 6 * i))
      FAIL("%s: rhs row %d at %d is not where the solver reads it", what, i, L.rdst[i]);
    for (int k = 0; k < 6; ++k) sys[L.rdst[i] + k] = -(1.0 + 6 * i + k);
  }
  if (band_on) {
    long sum = 0;
    for (int c = 0; c < F; ++c) {
      if (L.col_need[c] <= 0) FAIL("%s: column %d waits for no item", what, c);
      sum += L.col_need[c];
    }
    if (sum != nprof || L.col_need[F] != 1) FAIL("%s: col_need sums to %ld of %d blocks, cost %d", what, sum, nprof, L.col_need[F]);
    std::vector<int> items(F, 0);
    for (int b = 0; b < nprof; ++b) ++items[L.col[b]];  // (col[b] < F: checked with the block)
    for (int c = 0; c < F; ++c)
      if (items[c] != L.col_need[c]) FAIL("%s: column %d waits for %d items of %d", what, c, L.col_need[c], items[c]);
  }
  // dense_system against the directly built symmetric matrix and rhs
  const size_t n = 6 * (size_t)F;
  std::vector<double> S(n * n, -1.0), b(n, 0.0), want(n * n, 0.0);
  vo::dense_system(P, L, sys.data(), S.data(), b.data());
  for (int i = 0; i < F; ++i)
    for (int j = P.prof_first[i]; j <= i; ++j)
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c)
          want[(6 * (size_t)i + r) * n + 6 * j + c] = want[(6 * (size_t)j + c) * n + 6 * i + r] = enc(F, i, j, r, c);
  if (S != want) FAIL("%s: dense_system's S differs from the directly built matrix", what);
  for (size_t k = 0; k < n; ++k)
    if (b[k] != -(1.0 + (double)k)) FAIL("%s: dense_system's b[%zu]", what, k);
  return true;
}

// runs partition [0, n_chunks) in order; a taken-over run copies consecutive chunks of prev
static bool check_runs(const BAPlan& P, const BAPlan* prev, int* taken) {
  const int nch = P.n_chunks();
  if ((int)P.chunk_src.size() != nch || (int)P.chunk_img.size() != nch)
    FAIL("chunk_src has %zu entries, chunk_img %zu, of %d chunks", P.chunk_src.size(), P.chunk_img.size(), nch);
  std::vector<vo::ImageRun> runs;
  vo::image_runs(P, runs);
  int at = 0;
  *taken = 0;
  for (const vo::ImageRun& r : runs) {
    if (r.dst != at || r.count < 1) FAIL("image run at %d of %d chunks follows %d", r.dst, r.count, at);
    if (r.src < -1) FAIL("image run source %d", r.src);
    for (int k = 0; k < r.count; ++k)
      if (r.src < 0 ? P.chunk_src[at + k] >= 0 : P.chunk_src[at + k] != r.src + k) FAIL("image run at %d: chunk_src", r.dst);
    if (r.src >= 0) {
      if (!prev || r.src + r.count > prev->n_chunks()) FAIL("image run at %d: sources past the previous plan", r.dst);
      *taken += r.count;
    }
    at += r.count;
  }
  if (at != nch) FAIL("image runs cover %d of %d chunks", at, nch);
  if (*taken != P.reused_chunks) FAIL("image runs take over %d chunks, the plan %d", *taken, P.reused_chunks);
  return true;
}

static bool check_reserve(int n_poses, int n_points, int64_t n_obs, size_t want) {
  const vo::ReserveWindow W = vo::reserve_window(n_poses, n_points, n_obs);
  const std::vector<int32_t>&ptr = W.point_ptr, &cam = W.obs_cam;
  if ((int)ptr.size() != n_points + 1 || ptr[0] != 0 || (size_t)ptr[n_points] != cam.size()) FAIL("reserve_window: ptr ends");
  for (int p = 0; p < n_points; ++p) {
    if (ptr[p + 1] < ptr[p]) FAIL("reserve_window: ptr decreases at %d", p);
    for (int o = ptr[p]; o < ptr[p + 1]; ++o)
      if (cam[o] < 0 || cam[o] >= n_poses || (o > ptr[p] && cam[o] != cam[o - 1] + 1))
        FAIL("reserve_window: landmark %d's cameras", p);
  }
  const int len0 = (int)std::min<int64_t>(n_poses, n_obs / n_points);
  if (n_obs - (int64_t)len0 * n_points <= n_points && cam.size() != (size_t)std::min<int64_t>(n_obs, (int64_t)n_points * n_poses))
    FAIL("reserve_window(%d, %d, %ld): %zu observations", n_poses, n_points, (long)n_obs, cam.size());
  if (cam.size() != want) FAIL("reserve_window(%d, %d, %ld): %zu observations, %zu pinned", n_poses, n_points, (long)n_obs, cam.size(), want);
  std::vector<float> uv(2 * cam.size(), 0.0f);
  BAPlan P;
  const std::string err = vo::build_plan(P, n_poses, n_points, (int)cam.size(), 1, ptr.data(), cam.data(), uv.data(), 1);
  if (!err.empty()) FAIL("reserve_window(%d, %d, %ld): plan: %s", n_poses, n_points, (long)n_obs, err.c_str());
  return true;
}

static bool check_lm_log() {
  for (int n : {0, 1, 7}) {
    const vo::LmLog g{n};
    const size_t m = (size_t)n, off[6] = {g.cost_off(), g.lambda_off(), g.trial_off(), g.accepted_off(), g.stop_off(), g.bytes()};
    const size_t len[5] = {8 * (m + 1), 8 * (m + 1), 8 * m, 4 * m, 8};  // what the run writes of each region
    for (int k = 0; k < 5; ++k)
      if (off[k] + len[k] > off[k + 1] || (k < 3 && off[k] % 8) || off[k] % 4) FAIL("LmLog{%d}: region %d", n, k);
    if (off[0] != 0 || g.bytes() != (3 * m + 2) * 8 + (std::max(1, n) + 2) * sizeof(int)) FAIL("LmLog{%d}: %zu bytes", n, g.bytes());
  }
  // a log of five iterations: ran all; stopped behind trial 2 (f = 2); failed at iteration 3 (f = 3)
  const int N = 5;
  double raw[3 * N + 2];
  for (int k = 0; k <= N; ++k) raw[k] = 100.0 - k, raw[N + 1 + k] = 10.0 + k;
  for (int k = 0; k < N; ++k) raw[2 * N + 2 + k] = 50.0 + k;
  const int acc[N] = {1, 0, 1, 1, 0};
  struct Case {
    int n, f;
    bool stopped;
  } cases[] = {{5, 5, false}, {5, 2, true}, {5, 3, false}, {3, 2, true}};
  for (const Case& q : cases) {
    double cost[N + 1], lam[N + 1], trial[N];
    uint8_t a[N];
    vo::LmLog{N}.decode(raw, acc, q.n, q.f, q.stopped, cost, lam, trial, a);
    for (int k = 0; k <= q.n; ++k) {
      const bool live = k <= q.f;
      if (live || q.stopped ? cost[k] != 100.0 - std::min(k, q.f) || lam[k] != 10.0 + std::min(k, q.f)
                            : !(std::isnan(cost[k]) && std::isnan(lam[k])))
        FAIL("LmLog::decode(n %d, f %d, stopped %d): cost / lambda %d", q.n, q.f, q.stopped, k);
    }
    for (int k = 0; k < q.n; ++k)
      if (k < q.f ? trial[k] != 50.0 + k || a[k] != acc[k] : !std::isnan(trial[k]) || a[k] != 0)
        FAIL("LmLog::decode(n %d, f %d, stopped %d): trial / decision %d", q.n, q.f, q.stopped, k);
  }
  vo::LmLog{N}.decode(raw, acc, N, N, false, nullptr, nullptr, nullptr, nullptr);  // every output may be null
  vo_ba_lm_options o;
  if (!vo::lm_options(nullptr, 0.0, o).empty() || o.lambda0 != 1e-4 || o.up != 10.0 || o.down != 0.1 || o.lambda_min != 1e-6 ||
      o.lambda_max != 1e6)
    FAIL("lm_options: defaults");
  vo_ba_lm_options in{};
  in.up = 0.5;
  if (vo::lm_options(&in, 2.0, o) != "vo_ba_run_lm: up must be > 1") FAIL("lm_options: up = 0.5 accepted");
  in.up = 0.0;
  in.lambda_max = 1.0;
  if (!vo::lm_options(&in, 2.0, o).empty() || o.lambda0 != 1.0) FAIL("lm_options: lambda0 not clamped to lambda_max");
  return true;
}

static vo_ba_pose_factor make_factor(int i, int j) {
  vo_ba_pose_factor f{};
  f.cam_i = i;
  f.cam_j = j;
  for (int k = 0; k < 3; ++k) f.meas[4 * k] = 1.0;
  for (int k = 0; k < 6; ++k) f.info[7 * k] = 1.0;
  return f;
}

static int bandwidth(const std::vector<int32_t>& first) {
  int w = 0;
  for (size_t i = 0; i < first.size(); ++i) w = std::max(w, (int)i - first[i]);
  return w;
}

// every factor row inside its range, behind K1's sources, ahead of the prior's, none twice
static bool check_factor_rows(const BAPlan& P, const vo::FactorRows& R, int prior_k) {
  const int F = P.n_free;
  std::vector<int> slots(P.n_prof_blocks(), 0), ents(F, 0);
  for (size_t s = 0; s < P.slot_i.size(); ++s) ++slots[P.prof_off[P.slot_i[s]] + P.slot_j[s] - P.prof_first[P.slot_i[s]]];
  for (size_t e = 0; e < P.segcam_f.size(); ++e) ++ents[P.segcam_f[e]];
  std::vector<char> used(P.prof_src_ptr.back(), 0), usedb(P.camb_ptr.back(), 0);
  if (R.rows.size() != 5 * R.fi.size()) FAIL("factor rows: %zu entries for %zu factors", R.rows.size(), R.fi.size());
  for (size_t k = 0; k < R.fi.size(); ++k) {
    const int fi = R.fi[k], fj = R.fj[k], hi = std::max(fi, fj), lo = std::min(fi, fj);
    const int32_t* r = &R.rows[5 * k];
    const int want_blk[3][2] = {{fi, fi}, {fj, fj}, {lo >= 0 ? hi : -1, lo}};
    for (int q = 0; q < 3; ++q) {
      const int i = want_blk[q][0], j = want_blk[q][1];
      if ((i < 0 || j < 0) != (r[q] < 0)) FAIL("factor %zu: slab row %d is %d", k, q, r[q]);
      if (r[q] < 0) continue;
      if (j < P.prof_first[i]) FAIL("factor %zu: block (%d, %d) outside the profile", k, i, j);
      const int b = P.prof_off[i] + j - P.prof_first[i];
      const int last = P.prof_src_ptr[b + 1] - (i < prior_k ? 1 : 0);  // (the prior's row is the block's last)
      if (r[q] < P.prof_src_ptr[b] + slots[b] || r[q] >= last || used[r[q]]) FAIL("factor %zu: slab row %d at %d", k, q, r[q]);
      if (P.prof_src[r[q]] != -1) FAIL("factor %zu: slab row %d has a K1 source", k, q);
      used[r[q]] = 1;
    }
    const int cams[2] = {fi, fj};
    for (int q = 0; q < 2; ++q) {
      const int f = cams[q], row = r[3 + q];
      if ((f < 0) != (row < 0)) FAIL("factor %zu: rhs row %d is %d", k, q, row);
      if (row < 0) continue;
      const int last = P.camb_ptr[f + 1] - (f < prior_k ? 1 : 0);
      if (row < P.camb_ptr[f] + ents[f] || row >= last || usedb[row] || P.camb_src[row] != -1) FAIL("factor %zu: rhs row %d at %d", k, q, row);
      usedb[row] = 1;
    }
    // factor order within a block: a later factor on the same pair sits behind an earlier one
    for (size_t k2 = 0; k2 < k; ++k2)
      if (R.fi[k2] == fi && R.fj[k2] == fj)
        for (int q = 0; q < 5; ++q)
          if (r[q] >= 0 && R.rows[5 * k2 + q] >= r[q]) FAIL("factors %zu and %zu on one pair: rows out of factor order", k2, k);
  }
  return true;
}

static bool check_factor_errors(int N) {
  vo_ba_problem prob{};
  prob.n_poses = N;
  prob.n_fixed = 2;
  std::vector<vo_ba_pose_factor> fs{make_factor(1, 0), make_factor(2, -1), make_factor(1, N - 1)};
  auto err = [&](const std::vector<vo_ba_pose_factor>& v, int n) { return vo::pose_factor_error(&prob, v.data(), n); };
  if (!err(fs, 3).empty() || !err(fs, 0).empty()) FAIL("pose_factor_error: a good list refused: %s", err(fs, 3).c_str());
  if (err(fs, -1).empty() || vo::pose_factor_error(&prob, nullptr, 2).empty() || vo::pose_factor_error(nullptr, fs.data(), 3).empty())
    FAIL("pose_factor_error: n < 0, null factors or a null problem accepted");
  auto bad = [&](auto change) {
    std::vector<vo_ba_pose_factor> v = fs;
    change(v);
    const std::string e = err(v, 3);
    return !e.empty() && e.find("vo_ba_setup_factors") != std::string::npos;
  };
  if (!bad([&](auto& v) { v[0].cam_i = N; }) || !bad([&](auto& v) { v[0].cam_i = -1; }) || !bad([&](auto& v) { v[2].cam_j = N; }) ||
      !bad([&](auto& v) { v[1].cam_j = -2; }) || !bad([&](auto& v) { v[0].cam_j = 1; }) || !bad([&](auto& v) { v[1].meas[11] = NAN; }) ||
      !bad([&](auto& v) { v[2].info[6 * 5 + 2] = INFINITY; }))
    FAIL("pose_factor_error: a bad field accepted");
  std::vector<vo_ba_pose_factor> v = fs;
  v[0].info[6 * 2 + 5] = NAN;  // above the diagonal: not read
  if (!err(v, 3).empty()) FAIL("pose_factor_error: reads the upper triangle");
  std::vector<vo_ba_pose_factor> many(VO_BA_MAX_POSE_FACTORS + 1, fs[0]);
  if (!err(many, VO_BA_MAX_POSE_FACTORS).empty() || err(many, VO_BA_MAX_POSE_FACTORS + 1).empty()) FAIL("pose_factor_error: the cap");
  // the mask rule: an endpoint among cameras 0 .. n_drop - 1
  if (!vo::factor_marginalised(0, 5, 1) || !vo::factor_marginalised(5, 0, 1) || vo::factor_marginalised(1, 5, 1) ||
      vo::factor_marginalised(3, -1, 3) || !vo::factor_marginalised(2, -1, 3) || !vo::factor_marginalised(7, 2, 3))
    FAIL("factor_marginalised");
  return true;
}

// The pose factors' host tables over plan P (profile built without factors).
static bool check_factors(BAPlan& P, int N, int nf) {
  const int F = P.n_free;
  const std::vector<int32_t> first0 = vo::local_profile_first(P);
  const uint64_t digest0 = vo::plan_digest(P);
  const std::vector<int32_t> src_ptr = P.prof_src_ptr, src = P.prof_src, slab_pos = P.slab_pos, cptr = P.camb_ptr, csrc = P.camb_src,
                             cpos = P.cam_pos, off = P.prof_off, last = P.prof_last, tab = P.solve_tab;
  auto same = [&] {
    return P.prof_src_ptr == src_ptr && P.prof_src == src && P.slab_pos == slab_pos && P.camb_ptr == cptr && P.camb_src == csrc &&
           P.cam_pos == cpos && P.prof_off == off && P.prof_last == last && P.solve_tab == tab && P.prof_first == first0 &&
           vo::plan_digest(P) == digest0;
  };
  // no factors: nothing moves
  vo::FactorRows none;
  vo::factor_free_cams(nf, nullptr, 0, none);
  std::vector<int32_t> first = first0;
  vo::factor_lower_first(none, first);
  vo::build_profile(P, first, true, 0, &none);
  if (first != first0 || !same() || !none.rows.empty()) FAIL("an empty factor list changes the profile");
  // the chain over all cameras (fixed-fixed and fixed-free pairs included), a duplicate pair, a unary factor
  std::vector<vo_ba_pose_factor> fs;
  for (int c = 0; c + 1 < N; ++c) fs.push_back(make_factor(c + 1, c));
  if (N >= 2) fs.push_back(make_factor(N - 2, N - 1));  // the last pair again, the other way round
  fs.push_back(make_factor(N - 1, -1));
  vo::FactorRows chain;
  vo::factor_free_cams(nf, fs.data(), (int)fs.size(), chain);
  for (size_t k = 0; k < fs.size(); ++k)
    if (chain.fi[k] != (fs[k].cam_i >= nf ? fs[k].cam_i - nf : -1) || chain.fj[k] != (fs[k].cam_j >= nf ? fs[k].cam_j - nf : -1))
      FAIL("factor_free_cams at factor %zu", k);
  first = first0;
  vo::factor_lower_first(chain, first);
  const int w0 = bandwidth(first0), w_chain = bandwidth(first);
  for (int i = 1; i < F; ++i)
    if (first[i] > i - 1) FAIL("the chain leaves first[%d] = %d", i, first[i]);
  vo::build_profile(P, first, true, 0, &chain);
  if (!check_factor_rows(P, chain, 0)) return false;
  {  // K1's sources keep their order (K2's summation order over them), the factors' rows lie between
    std::vector<int32_t> k1, k1b;
    for (int32_t v : P.prof_src)
      if (v >= 0) k1.push_back(v);
    for (int32_t v : P.camb_src)
      if (v >= 0) k1b.push_back(v);
    if (k1 != src || k1b != csrc) FAIL("factors reorder K1's sources");
    for (size_t s = 0; s < P.slot_i.size(); ++s)
      if (P.prof_src[P.slab_pos[s]] != (int32_t)s) FAIL("slab_pos of slot %zu", s);
    for (size_t e = 0; e < P.segcam_f.size(); ++e)
      if (P.camb_src[P.cam_pos[e]] != (int32_t)e) FAIL("cam_pos of entry %zu", e);
  }
  size_t rows = 0, brows = 0;
  for (size_t e = 0; e < chain.rows.size(); ++e) (e % 5 < 3 ? rows : brows) += chain.rows[e] >= 0;
  if ((size_t)P.prof_src_ptr.back() != P.slot_i.size() + rows || (size_t)P.camb_ptr.back() != P.segcam_f.size() + brows)
    FAIL("%d slab rows for %zu slots and %zu factor rows, %d rhs rows for %zu entries and %zu", P.prof_src_ptr.back(),
         P.slot_i.size(), rows, P.camb_ptr.back(), P.segcam_f.size(), brows);
  // with a prior over the leading poses as well: its rows stay the last of their ranges
  const int pk = std::min(3, F);
  std::vector<int32_t> firstp = first;
  for (int i = 0; i < pk; ++i) firstp[i] = 0;
  vo::build_profile(P, firstp, true, pk, &chain);
  if (!check_factor_rows(P, chain, pk)) return false;
  // one more factor between the first and the last free pose: the profile's span is F - 1
  int w_far = w_chain;
  if (F >= 2) {
    fs.push_back(make_factor(nf, N - 1));
    vo::FactorRows far;
    vo::factor_free_cams(nf, fs.data(), (int)fs.size(), far);
    first = first0;
    vo::factor_lower_first(far, first);
    w_far = bandwidth(first);
    if (first[F - 1] != 0) FAIL("the far factor leaves first[%d] = %d", F - 1, first[F - 1]);
    vo::build_profile(P, first, true, 0, &far);
    if (!check_factor_rows(P, far, 0)) return false;
    if (!check_layout(P, false, w_far, F, "profile layout with the far factor")) return false;
  }
  // and back: the profile without factors again
  vo::build_profile(P, first0);
  if (!same()) FAIL("the profile without factors differs after one with factors");
  if (!check_factor_errors(N)) return false;
  std::printf("factors ok %d %d %d %d %zu\n", F, w0, w_chain, w_far, rows);
  return true;
}

// group_by_point against a counting loop: with order, the CSR and the stable grouping; without,
// the CSR of grouped input and the verdict alone (point_ptr untouched) of ungrouped input.
static bool check_group(int n_points, const std::vector<int32_t>& pt, const char* what) {
  const int M = (int)pt.size();
  bool sorted = true;
  for (int o = 1; o < M; ++o) sorted = sorted && pt[o] >= pt[o - 1];
  std::vector<int32_t> want_ptr(n_points + 1, 0), want_order;
  for (int p = 0; p < n_points; ++p) {
    for (int o = 0; o < M; ++o)
      if (pt[o] == p) want_order.push_back(o);
    want_ptr[p + 1] = (int32_t)want_order.size();
  }
  const int32_t* in = M ? pt.data() : nullptr;
  std::vector<int32_t> ptr(n_points + 1, -7), order(std::max(M, 1), -7);
  bool grouped = false;
  std::string err = vo::group_by_point(n_points, M, in, order.data(), ptr.data(), grouped);
  order.resize(M);
  if (!err.empty() || !grouped || ptr != want_ptr || order != want_order) FAIL("group_by_point, %s, with order: %s", what, err.c_str());
  ptr.assign(n_points + 1, -7);
  err = vo::group_by_point(n_points, M, in, nullptr, ptr.data(), grouped);
  if (!err.empty() || grouped != sorted || ptr != (sorted ? want_ptr : std::vector<int32_t>(n_points + 1, -7)))
    FAIL("group_by_point, %s, without order: %s", what, err.c_str());
  return true;
}

// a bad entry: both paths name the first offender and report nothing else
static bool check_group_error(int n_points, const std::vector<int32_t>& pt, int at) {
  const std::string want = "vo_ba_group_by_point: obs_pt[" + std::to_string(at) + "]=" + std::to_string(pt[at]) + " out of range";
  std::vector<int32_t> ptr(n_points + 1), order(pt.size());
  for (int32_t* ord : {order.data(), (int32_t*)nullptr}) {
    bool grouped = false;
    const std::string err = vo::group_by_point(n_points, (int)pt.size(), pt.data(), ord, ptr.data(), grouped);
    if (err != want || !grouped) FAIL("group_by_point %s order: \"%s\", not \"%s\"", ord ? "with" : "without", err.c_str(), want.c_str());
  }
  return true;
}

static bool check_group_by_point() {
  if (!check_group(7, {1, 1, 2, 4, 4, 4, 5}, "grouped, landmarks 0, 3 and 6 empty") ||
      !check_group(7, {3, 0, 3, 1, 0, 5, 3}, "ungrouped") || !check_group(2, {1, 0}, "ungrouped, two observations") ||
      !check_group(1, {0, 0, 0}, "one landmark") || !check_group(3, {}, "n_obs = 0") || !check_group(0, {}, "n_points = 0"))
    return false;
  // out of range at the first, the last and a middle position, in grouped and ungrouped input
  if (!check_group_error(3, {9, 1, 2}, 0) || !check_group_error(3, {0, 1, 3}, 2) || !check_group_error(3, {0, -1, 2}, 1) ||
      !check_group_error(3, {-1, 0, 2}, 0) || !check_group_error(3, {2, 0, 3}, 2) || !check_group_error(3, {2, 7, 0}, 1) ||
      !check_group_error(4, {0, 7, -2, 1, 9}, 1) || !check_group_error(0, {0}, 0))
    return false;
  bool grouped = false;
  int32_t one[1] = {0}, ptr[2];
  if (vo::group_by_point(-1, 0, one, nullptr, ptr, grouped) != "vo_ba_group_by_point: bad sizes" ||
      vo::group_by_point(1, -1, one, nullptr, ptr, grouped) != "vo_ba_group_by_point: bad sizes" ||
      vo::group_by_point(1, 1, one, nullptr, nullptr, grouped) != "vo_ba_group_by_point: null argument" ||
      vo::group_by_point(1, 1, nullptr, one, ptr, grouped) != "vo_ba_group_by_point: null argument")
    FAIL("group_by_point: bad sizes or a null argument accepted");
  std::printf("group ok\n");
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (std::string(argv[1]) == "group") return check_group_by_point() ? 0 : 1;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hd[5];
  if (std::fread(hd, 4, 5, f) != 5) return 2;
  const int N = hd[0], L = hd[1], M = hd[2], nf = hd[3], so = hd[4];
  std::vector<int32_t> ptr(L + 1), cam(M);
  std::vector<float> uv(2 * (size_t)M);
  if (std::fread(ptr.data(), 4, L + 1, f) != (size_t)L + 1 || std::fread(cam.data(), 4, M, f) != (size_t)M ||
      std::fread(uv.data(), 4, 2 * (size_t)M, f) != 2 * (size_t)M)
    return 2;
  std::fclose(f);
  const int sc = argc > 2 ? std::atoi(argv[2]) : 1;
  auto plan = [&](BAPlan& P, const BAPlan* prev) {
    const std::string err = vo::build_plan(P, N, L, M, nf, ptr.data(), cam.data(), uv.data(), so, prev, sc);
    if (!err.empty()) FAIL("plan: %s", err.c_str());
    vo::build_profile(P, vo::local_profile_first(P));
    return true;
  };
  BAPlan P, P2;
  if (!plan(P, nullptr) || !check_obs(P, ptr, cam, uv)) return 1;
  if (argc > 3 && std::string(argv[3]) == "factors") return check_factors(P, N, nf) ? 0 : 1;
  const int F = P.n_free;
  int w = 0, layouts = 2;
  for (int i = 0; i < F; ++i) w = std::max(w, i - P.prof_first[i]);
  if (!check_layout(P, false, w, F, "profile layout") || !check_layout(P, true, w, F, "banded layout, one-sided")) return 1;
  if (F >= 2 * w + 2) {  // band_split's two-sided split: s = w, nb = (F - w) / 2, m = F - w - nb
    const int nb = (F - w) / 2, m = F - w - nb;
    if (!check_layout(P, true, w, m + w, "banded layout, two-sided")) return 1;
    ++layouts;
  }
  int none = 0, taken = 0;
  if (!check_runs(P, nullptr, &none)) return 1;
  // the same window again, on top of its own plan: the chunks it takes over
  if (!plan(P2, &P) || !check_obs(P2, ptr, cam, uv) || !check_runs(P2, &P, &taken)) return 1;
  if (!check_reserve(8, 200, 661, 661) || !check_reserve(2, 1, 2, 2) || !check_reserve(50, 1000, 5000, 5000) ||
      !check_reserve(2, 10, 100, 20))
    return 1;
  if (!check_lm_log()) return 1;
  std::printf("ok %d %d %d %d %d\n", F, w, layouts, P.n_chunks(), taken);
  return 0;
}
