"""GPU covariance read-out (``vo_ba_covariance``) against its CPU restatement (tests/ba_cov_ref.py).

Metric: max_ij |A_ij - B_ij| / sqrt(B_ii B_jj), over the dense 6F x 6F pose matrix and per 3x3
landmark block.  The GPU is compared with route A at ``max(1e-8, 100 eps_ref)``: 1e-8 is the
project's per-step tolerance and eps_ref the disagreement of routes A and B on the same input,
computed here on the CPU and required to be <= 1e-9 (so the tolerance never exceeds 1e-7).
Inputs whose eps_ref misses that are not used: ``(20, 500, 9, max_track=4)`` at lambda = 0
(4.2e-8), and the narrow input at lambda = 0 after five iterations (1.6e-9).  Constructions with a
frozen landmark have no route B (it freezes nothing) and are held to 1e-8.
"""

import ctypes as C
import functools
import threading

import numpy as np
import pytest

from oracle import ba_ref
from tests import ba_cov_ref as cr
from tests import ba_robust_ref as rr
from visualodometry_amd import _lib
from visualodometry_amd._lib import VoError, ptr
from visualodometry_amd.ba import BASession, BAWindow, SlidingWindowBA, rt_to_poses, poses_to_rt
from visualodometry_amd.shard import shard
from visualodometry_amd.synthetic import make_ba_problem

pytestmark = pytest.mark.gpu

STEP_TOL = 1e-8
EPS_REF_MAX = 1e-9
RUN_LAM = 1.0  # the problem's damping in every session here (the covariance call has its own)


@functools.lru_cache(maxsize=None)
def _problem(name):
    n, l, seed, kw = cr.INPUTS[name]
    return make_ba_problem(n, l, seed, **kw)


def _session(p, ctx, uv=None, huber=0.0, ptr_cam=None):
    pp, cam = (p.point_ptr, p.obs_cam) if ptr_cam is None else ptr_cam
    s = BASession(p.K, pp, cam, p.obs_uv if uv is None else uv, p.n_poses, p.n_fixed, RUN_LAM, ctx, huber=huber)
    s.set_state(p.poses_cw, p.points)
    return s


def _structure(p, uv=None, ptr_cam=None):
    pp, cam = (p.point_ptr, p.obs_cam) if ptr_cam is None else ptr_cam
    return ba_ref.BAStructure(p.K, pp, cam, p.obs_uv if uv is None else uv, p.n_fixed, p.n_poses)


def _check(got, st, s, lam, delta=0.0, what=""):
    """got = (pose_cov, point_cov, dense) of the GPU at state st."""
    pose, pts, dense = got
    eps, (cc, pp) = cr.routes_disagreement(st, s, lam, delta)
    assert eps <= EPS_REF_MAX, f"{what}: eps_ref {eps:.3g} makes this input unusable"
    tol = max(STEP_TOL, 100.0 * eps)
    e_pose, e_pts = cr.rel_err(dense, cc), cr.rel_err(pts, pp)
    print(f"{what} lam={lam}: eps_ref {eps:.3g} tol {tol:.3g} pose err {e_pose:.3g} landmark err {e_pts:.3g}")
    assert e_pose <= tol and e_pts <= tol
    _consistent(pose, pts, dense)
    return cc, pp


def _consistent(pose, pts, dense):
    F = pose.shape[0]
    np.testing.assert_array_equal(dense, dense.T)
    np.testing.assert_array_equal(pts, pts.transpose(0, 2, 1))
    for f in range(F):
        np.testing.assert_array_equal(pose[f], dense[6 * f : 6 * f + 6, 6 * f : 6 * f + 6])


@pytest.mark.parametrize("name", list(cr.INPUTS))
def test_parity_at_the_initial_guess_and_after_a_run(ctx, name):
    p = _problem(name)
    s, struct = _session(p, ctx), _structure(p)
    st0 = ba_ref.BAState.from_poses(p.poses_cw, p.points)
    for lam in (0.0, 1.0):
        cc, _ = _check(s.covariance(lam, dense=True), st0, struct, lam, what=f"{name} initial")
        if name == "narrow" and lam == 0.0:
            # an inverse of S's band alone cannot pass: the reference is dense outside it
            F = struct.n_free
            d = np.sqrt(np.diag(cc))
            corr = np.abs(cc / d[:, None] / d[None, :]).reshape(F, 6, F, 6).max(axis=(1, 3))
            assert corr[np.abs(np.subtract.outer(np.arange(F), np.arange(F))) > 3].max() > 0.9
    rc, _ = s.run(5)
    assert rc == _lib.VO_OK
    P, X = s.get_state()
    st5 = ba_ref.BAState.from_poses(P, X)
    for lam in (1.0,) if name == "narrow" else (0.0, 1.0):  # (narrow at 0: eps_ref 1.6e-9, see above)
        _check(s.covariance(lam, dense=True), st5, struct, lam, what=f"{name} after run(5)")


def test_parity_on_a_wide_profile(ctx):
    """F = 48 with a block row span of 46: the factor kernel's panel has more than 256 rows (its
    lanes take a second pass and every wave owns panel rows), and S is in the profile solver's
    layout.  lambda = 1 only: at 0 this input's eps_ref is 9e-8 (tests/ba_cov_ref.py)."""
    p, cam, uv = cr.wide_problem()
    s = _session(p, ctx, uv=uv, ptr_cam=(p.point_ptr, cam))
    assert s.plan_stats()["band_solver"] == 0
    struct = _structure(p, uv=uv, ptr_cam=(p.point_ptr, cam))
    st0 = ba_ref.BAState.from_poses(p.poses_cw, p.points)
    _check(s.covariance(1.0, dense=True), st0, struct, 1.0, what="wide initial")
    rc, _ = s.run(3)
    assert rc == _lib.VO_OK
    P, X = s.get_state()
    _check(s.covariance(1.0, dense=True), ba_ref.BAState.from_poses(P, X), struct, 1.0, what="wide after run(3)")


def test_repeatable_and_null_outputs(ctx):
    p = _problem("small")
    s = _session(p, ctx)
    a = s.covariance(0.0, dense=True)
    b = s.covariance(0.0, dense=True)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    pose, pts = s.covariance(0.0)
    np.testing.assert_array_equal(pose, a[0])
    np.testing.assert_array_equal(pts, a[1])
    assert ctx.lib.vo_ba_covariance(ctx.handle, s.session, 0.0, None, None, None) == _lib.VO_OK
    only = np.empty_like(a[1])
    assert ctx.lib.vo_ba_covariance(ctx.handle, s.session, 0.0, None, None, ptr(only, C.c_double)) == _lib.VO_OK
    np.testing.assert_array_equal(only, a[1])


def _run_pair(p, ctx, prepare, between):
    """State and costs of prepare(s); between(s); run(3) on a fresh session."""
    s = _session(p, ctx)
    prepare(s)
    between(s)
    rc, costs = s.run(3)
    assert rc == _lib.VO_OK
    return (costs,) + tuple(s.get_state())


@pytest.mark.parametrize("prepare", ["run", "gn_step", "run_lm"])
def test_state_and_later_runs_untouched(ctx, prepare):
    p = _problem("small")
    prep = {"run": lambda s: s.run(3), "gn_step": lambda s: s.gn_step(), "run_lm": lambda s: s.run_lm(3)}[prepare]

    def cov(s):
        s.covariance(0.0)
        s.covariance(0.5, dense=True)

    with_cov = _run_pair(p, ctx, prep, cov)
    without = _run_pair(p, ctx, prep, lambda s: None)
    for x, y in zip(with_cov, without):
        np.testing.assert_array_equal(x, y)
    # the call itself leaves poses and points as they were
    s = _session(p, ctx)
    prep(s)
    P0, X0 = s.get_state()
    cov(s)
    P1, X1 = s.get_state()
    np.testing.assert_array_equal(P0, P1)
    np.testing.assert_array_equal(X0, X1)


def test_frozen_fixed_only_and_duplicate(ctx):
    p = make_ba_problem(6, 120, 31)
    ptr2, cam2, uv2 = cr.degenerate_problem(p, duplicate=True)
    s = _session(p, ctx, uv=uv2, ptr_cam=(ptr2, cam2))
    struct = _structure(p, uv=uv2, ptr_cam=(ptr2, cam2))
    st = ba_ref.BAState.from_poses(p.poses_cw, p.points)
    # lambda = 0: landmark 0 (one observation) is frozen
    pose, pts, dense = s.covariance(0.0, dense=True)
    cc, pp = cr.route_a(st, struct, 0.0)
    assert np.isnan(pts[0]).all() and np.isnan(pp[0]).all() and np.isfinite(pts[1:]).all()
    e_pose, e_pts = cr.rel_err(dense, cc), cr.rel_err(pts, pp)
    print(f"degenerate lam=0: pose err {e_pose:.3g} landmark err {e_pts:.3g}")
    assert e_pose <= STEP_TOL and e_pts <= STEP_TOL
    _consistent(pose, pts, dense)
    vinv = ba_ref.build_system(st, struct, 0.0).Vinv[2]  # fixed cameras only: no pose term
    assert cr.rel_err(pts[2:3], vinv[None]) <= STEP_TOL
    # lambda = 1: nothing is frozen, and both routes exist
    got = s.covariance(1.0, dense=True)
    assert np.isfinite(got[1]).all()
    _check(got, st, struct, 1.0, what="degenerate")


@pytest.mark.parametrize("lam", [0.0, 1.0])
def test_huber(ctx, lam):
    p = _problem("small")
    uv = rr.with_outliers(p, 21)
    s = _session(p, ctx, uv=uv, huber=2.0)
    st = ba_ref.BAState.from_poses(p.poses_cw, p.points)
    _check(s.covariance(lam, dense=True), st, _structure(p, uv=uv), lam, delta=2.0, what="huber")


def test_not_spd_is_a_status(ctx):
    """``test_not_spd_reported``'s construction: a free camera without observations makes S
    singular without damping; the call says so and the session goes on."""
    p = make_ba_problem(6, 100, 41)
    cam = p.obs_cam.copy()
    cam[cam == 5] = 4
    s = BASession(p.K, p.point_ptr, cam, p.obs_uv, p.n_poses, 2, 0.0, ctx)
    s.set_state(p.poses_cw, p.points)
    F = p.n_poses - 2
    pose, dense, pts = np.zeros((F, 6, 6)), np.zeros((6 * F, 6 * F)), np.zeros((p.n_points, 3, 3))
    rc = ctx.lib.vo_ba_covariance(ctx.handle, s.session, 0.0, ptr(pose, C.c_double), ptr(dense, C.c_double),
                                  ptr(pts, C.c_double))
    assert rc == _lib.VO_ERR_NOT_SPD
    assert np.isnan(pose).all() and np.isnan(dense).all() and np.isnan(pts).all()
    with pytest.raises(VoError) as e:
        s.covariance(0.0)
    assert e.value.code == _lib.VO_ERR_NOT_SPD
    got = s.covariance(1.0, dense=True)
    st = ba_ref.BAState.from_poses(p.poses_cw, p.points)
    struct = ba_ref.BAStructure(p.K, p.point_ptr, cam, p.obs_uv, 2, p.n_poses)
    _check(got, st, struct, 1.0, what="after not-SPD")
    P, X = s.get_state()
    np.testing.assert_array_equal(P, rt_to_poses(poses_to_rt(p.poses_cw)))
    np.testing.assert_array_equal(X, p.points)


def test_bad_arguments_and_stale_session(ctx):
    p = _problem("tiny")
    s = _session(p, ctx)
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(VoError) as e:
            s.covariance(bad)
        assert e.value.code == _lib.VO_ERR_ARG
    fresh = BASession(p.K, p.point_ptr, p.obs_cam, p.obs_uv, p.n_poses, p.n_fixed, RUN_LAM, ctx)
    for sess in (s, fresh):  # replaced by the later setup; set up but without a state
        with pytest.raises(VoError) as e:
            sess.covariance(0.0)
        assert e.value.code == _lib.VO_ERR_STATE


def test_all_poses_fixed(ctx):
    """F = 0 (``test_all_fixed_and_empty``'s problem): empty pose outputs, every landmark V^-1."""
    p = make_ba_problem(4, 50, 51)
    s = BASession(p.K, p.point_ptr, p.obs_cam, p.obs_uv, 4, 4, RUN_LAM, ctx)
    s.set_state(p.poses_cw, p.points)
    struct = ba_ref.BAStructure(p.K, p.point_ptr, p.obs_cam, p.obs_uv, 4, 4)
    st = ba_ref.BAState.from_poses(p.poses_cw, p.points)
    for lam in (0.0, 1.0):
        pose, pts, dense = s.covariance(lam, dense=True)
        assert pose.shape == (0, 6, 6) and dense.shape == (0, 0)
        eps, (_, pp) = cr.routes_disagreement(st, struct, lam)
        assert eps <= EPS_REF_MAX
        assert cr.rel_err(pts, pp) <= max(STEP_TOL, 100.0 * eps)
        vinv = ba_ref.build_system(st, struct, lam).Vinv
        assert cr.rel_err(pts, 0.5 * (vinv + vinv.transpose(0, 2, 1))) <= STEP_TOL


def test_two_ranks_are_refused():
    """Sharded covariance is not built: with a two-rank (loopback) communicator every rank gets
    VO_ERR_STATE (the pattern of test_gpu_ba_lm.py::test_two_ranks_are_refused)."""
    p = _problem("small")
    nranks, codes, errors = 2, [None, None], []

    def worker(r):
        try:
            c = _lib.Context(0)
            _lib.comm_init_loopback(c, nranks, r, b"vo-loopback-cov")
            _, pp, cam, suv, pts = shard(p.point_ptr, p.obs_cam, p.obs_uv, p.points, nranks, r)
            s = BASession(p.K, pp, cam, suv, p.n_poses, p.n_fixed, RUN_LAM, c)
            s.set_state(p.poses_cw, pts)
            try:
                s.covariance(0.0)
            except VoError as e:
                codes[r] = e.code
        except Exception as e:  # surfaced below
            errors.append(e)

    th = [threading.Thread(target=worker, args=(r,)) for r in range(nranks)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in th), "loopback group deadlocked"
    if errors:
        raise errors[0]
    assert codes == [_lib.VO_ERR_STATE] * nranks


def test_sliding_window_ba_returns_covariance(ctx):
    """Observations not grouped by landmark: point_cov still comes back by the window's landmark
    index, and cov_sigma2 follows its formula."""
    p = _problem("small")
    obs_pt = np.repeat(np.arange(p.n_points), np.diff(p.point_ptr))
    perm = np.random.default_rng(5).permutation(obs_pt.size)
    w = BAWindow(p.poses_cw, p.points, p.obs_uv[perm], p.obs_cam[perm], obs_pt[perm], p.n_fixed)
    ba = SlidingWindowBA(p.K, None, iters=5, lam=RUN_LAM)
    res = ba.optimize(w, return_covariance=True)
    assert res.status == "ok"
    F, L, M = p.n_poses - p.n_fixed, p.n_points, obs_pt.size
    assert res.pose_cov.shape == (F, 6, 6) and res.point_cov.shape == (L, 3, 3)
    live = int(np.isfinite(res.point_cov[:, 0, 0]).sum())
    assert res.cov_sigma2 == res.cost_per_iter[-1] / max(1, 2 * M - 6 * F - 3 * live)
    st = ba_ref.BAState.from_poses(res.poses_cw, res.points)
    eps, (cc, pp) = cr.routes_disagreement(st, _structure(p), 0.0)
    assert eps <= EPS_REF_MAX
    tol = max(STEP_TOL, 100.0 * eps)
    assert cr.rel_err(res.point_cov, pp) <= tol
    blocks = np.stack([cc[6 * f : 6 * f + 6, 6 * f : 6 * f + 6] for f in range(F)])
    assert cr.rel_err(res.pose_cov, blocks) <= tol
    off = ba.optimize(w)
    assert off.pose_cov is None and off.point_cov is None and off.cov_sigma2 is None
    on = SlidingWindowBA(p.K, type("Cfg", (), {"ba_covariance": True, "ba_iters": 5, "ba_lambda": RUN_LAM})()).optimize(w)
    np.testing.assert_array_equal(on.point_cov, res.point_cov)
