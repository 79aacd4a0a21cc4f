// Entry points of the BA engine (ba_engine.hip) used by api.hip; the engine is created in the
// context on first use.
#pragma once

#include <cstdint>

#include "vo_common.h"

struct vo_ctx;

namespace vo {

uint64_t ba_setup(vo_ctx* ctx, const vo_ba_problem* p, const vo_ba_pose_prior* prior = nullptr,
                  const vo_ba_pose_factor* factors = nullptr, int n_factors = 0);
void ba_reserve(vo_ctx* ctx, int n_poses, int n_points, int64_t n_obs, int n_fixed);
void ba_check_session(vo_ctx* ctx, uint64_t session);
void ba_set_state(vo_ctx* ctx, const double* poses, const double* pts);
void ba_get_state(vo_ctx* ctx, double* poses, double* pts);
int ba_run(vo_ctx* ctx, int iters, double* cost, bool sync);
int ba_gn_step(vo_ctx* ctx, double* S, double* b, double* dc, double* cost);
int ba_run_lm(vo_ctx* ctx, int iters, const vo_ba_lm_options* opt, double* cost, double* lambda, double* trial,
              uint8_t* accepted, bool sync);
int ba_lm_log(vo_ctx* ctx, int n, double* cost, double* lambda, double* trial, uint8_t* accepted);
void ba_set_lm_stop(vo_ctx* ctx, const vo_ba_lm_stop* stop);
void ba_lm_stop_info(vo_ctx* ctx, int32_t* trials, int32_t* reason);
void ba_set_robust(vo_ctx* ctx, double huber_delta);
void ba_residuals(vo_ctx* ctx, double* err2, double* depth);
int ba_covariance(vo_ctx* ctx, double lambda, double* pose_cov, double* pose_dense, double* point_cov);
int ba_marginalize(vo_ctx* ctx, int n_drop, double lambda, int32_t* n_prior, double* info, double* rhs, double* poses0,
                   double* cost0, uint8_t* mask);
void ba_set_obs_weights(vo_ctx* ctx, const double* w);
void ba_get_obs_weights(vo_ctx* ctx, double* w_out);
void ba_cull(vo_ctx* ctx, const vo_ba_cull_options* opt, int32_t* n_culled, int32_t* n_active, bool sync);
int ba_stats(vo_ctx* ctx, int64_t* out, int n);
int ba_stamps(vo_ctx* ctx, uint64_t* out, int n);
int ba_chain_stamps(vo_ctx* ctx, uint64_t* out, int n);
void ba_last_run(vo_ctx* ctx, int* chained, int* launches);

}  // namespace vo
