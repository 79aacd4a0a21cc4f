"""The pose prior on the MI355X (``vo_ba_setup_prior``), against the CPU restatement
(tests/ba_prior_ref.py).

Inputs: ``make_ba_problem(8, 300, 21)`` (SMALL) and ``make_ba_problem(16, 400, 5, max_track=4)``
(NARROW): the smallest windows here that cross chunks and segments and have observations in the
fixed cameras.  lambda = 1, Huber delta = 2 px and ``test_gpu_ba_weights``' weights where a test uses
them.  Synthetic priors (``_prior``): Lambda = A^T A + I from a seeded generator, A scaled so that
Lambda's diagonal is of the order of the reduced system's own (a prior that vanishes beside S would
pass every parity check without being applied: ``test_the_prior_moves_the_step`` holds that it does
not), eta of the order of Lambda * 0.01, poses0 the initial poses moved by twists of about 1e-2.
K = 3 keeps both windows on the banded solver, K = 12 on NARROW forces the profile solver.

Bounds.  A step (S, b, dc, cost against the restatement) is held to the project's per-step bound,
1e-8 of the largest entry; a whole solve of 10 iterations to 1e-5.  Where two runs launch the same
kernels on the same plan the comparison is bit for bit.
"""

import ctypes as C
import functools

import numpy as np
import pytest
import scipy.linalg

from oracle import ba_ref
from tests import ba_cov_ref as cr
from tests import ba_prior_ref as pr
from visualodometry_amd import _lib
from visualodometry_amd._lib import VoError
from visualodometry_amd.ba import BASession, BAWindow, PosePrior, SlidingWindowBA, _prior_struct, _problem_struct
from visualodometry_amd.synthetic import make_ba_problem

pytestmark = pytest.mark.gpu

LAM, DELTA = 1.0, 2.0
STEP, SOLVE = 1e-8, 1e-5
SMALL, NARROW = (8, 300, 21, ()), (16, 400, 5, (("max_track", 4),))
# (window, K, banded solver expected)
CASES = [(SMALL, 3, True), (NARROW, 3, True), (NARROW, 12, False)]


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300)


@functools.lru_cache(maxsize=None)
def _case(case, n_fixed=None):
    n, L, seed, kw = case
    p = make_ba_problem(n, L, seed, **dict(kw))
    nf = p.n_fixed if n_fixed is None else n_fixed
    s = ba_ref.BAStructure(p.K, p.point_ptr, p.obs_cam, p.obs_uv, nf, p.n_poses)
    return p, s, ba_ref.BAState.from_poses(p.poses_cw, p.points)


@functools.lru_cache(maxsize=None)
def _weights(case):
    M = _case(case)[1].obs_cam.size
    rng = np.random.default_rng(1000 + case[2])
    w = rng.uniform(0.25, 4.0, M)
    w[rng.random(M) < 0.1] = 0.0
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _prior(case, k, n_fixed=None, zero=False):
    _, s, st0 = _case(case, n_fixed)
    rng = np.random.default_rng(7000 + 10 * case[2] + k)
    n = 6 * k
    d = np.diag(ba_ref.build_system(st0, s, 0.0).S)[:n].mean()  # the scale of S's own diagonal
    A = rng.normal(size=(n, n)) * np.sqrt(d / n)
    info = A.T @ A + np.eye(n)
    rhs = info @ (0.01 * rng.normal(size=n))
    Rd, td = ba_ref.se3_exp(1e-2 * rng.normal(size=(k, 6)))
    poses0 = np.tile(np.eye(4), (k, 1, 1))
    poses0[:, :3, :3] = Rd @ st0.R[s.n_fixed:s.n_fixed + k]
    poses0[:, :3, 3] = np.einsum("nij,nj->ni", Rd, st0.t[s.n_fixed:s.n_fixed + k]) + td
    if zero:
        info, rhs = np.zeros_like(info), np.zeros_like(rhs)
    # cost0: the quadratic's minimum is cost0 - eta^T Lambda^-1 eta; 3.5 above it keeps E_prior > 0
    return pr.Prior(info, rhs, poses0, 0.0 if zero else 3.5 + float(rhs @ np.linalg.solve(info, rhs)))


def _session(case, ctx, prior, huber=0.0, n_fixed=None, lam=LAM, w=None):
    p, s, st0 = _case(case, n_fixed)
    pp = None if prior is None else PosePrior(prior.info, prior.rhs, prior.poses0, prior.cost0)
    sess = BASession(p.K, s.point_ptr, s.obs_cam, s.obs_uv, p.n_poses, s.n_fixed, lam, ctx, huber=huber, prior=pp)
    sess.set_state(st0.poses_cw(), st0.X)
    if w is not None:
        sess.set_obs_weights(w)
    return sess


def _step_figures(got, ref):
    rc, S, b, dc, cost = got
    assert rc == _lib.VO_OK
    assert np.isfinite(S).all() and np.isfinite(b).all() and np.isfinite(dc).all() and np.isfinite(cost)
    return dict(S=_rel(S, ref.system.S), b=_rel(b, ref.system.b), dc=_rel(dc, ref.dc),
                cost=abs(cost - ref.system.cost) / abs(ref.system.cost))


def _assert_step(figs, what):
    print(f"{what}: step errors", {k: f"{v:.2e}" for k, v in figs.items()})
    for k, v in figs.items():
        assert v < STEP, (what, k, v)


# 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robust", [False, True], ids=["plain", "huber+weights"])
@pytest.mark.parametrize("case,k,banded", CASES)
def test_gn_step_parity(ctx, case, k, banded, robust):
    _, s, st0 = _case(case)
    prior = _prior(case, k)
    delta, w = (DELTA, _weights(case)) if robust else (0.0, None)
    sess = _session(case, ctx, prior, huber=delta, w=w)
    assert bool(sess.plan_stats()["band_solver"]) == banded
    ref = pr.gn_step(st0, s, LAM, prior, w, delta)
    figs = _step_figures(sess.gn_step(), ref)
    P, X = sess.get_state()
    figs.update(P=_rel(P, ref.state.poses_cw()), X=_rel(X, ref.state.X))
    _assert_step(figs, f"{case[:3]} K {k} {'huber+weights' if robust else 'plain'}")


@pytest.mark.parametrize("case,k,banded", CASES)
def test_the_prior_moves_the_step(ctx, case, k, banded):
    """The synthetic prior is no rounding matter: the restatement's step with it differs from the
    step without it by far more than any bound here, in S, b, dc and the cost."""
    _, s, st0 = _case(case)
    a, b = pr.gn_step(st0, s, LAM, _prior(case, k)), pr.gn_step(st0, s, LAM, None)
    for x, y in ((a.system.S, b.system.S), (a.system.b, b.system.b), (a.dc, b.dc)):
        assert _rel(x, y) > 1e-2
    assert abs(a.system.cost - b.system.cost) > 1.0


# 2 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,k,banded", CASES)
def test_run_parity_and_repeatable(ctx, case, k, banded):
    _, s, st0 = _case(case)
    prior = _prior(case, k)
    sess = _session(case, ctx, prior)
    rc, costs = sess.run(10)
    assert rc == _lib.VO_OK
    chained, launches = _lib.ba_testing_last_run(ctx)
    assert not chained and launches == 20, "a session with a prior: a K1 launch and a solve launch per iteration"
    P, X = sess.get_state()
    ref, ref_costs = pr.solve(st0, s, 10, LAM, prior)
    figs = (_rel(costs, ref_costs), _rel(P, ref.poses_cw()), _rel(X, ref.X))
    print("run(10) errors:", " ".join(f"{v:.2e}" for v in figs))
    assert max(figs) < SOLVE
    again = _session(case, ctx, prior)
    rc, costs2 = again.run(10)
    P2, X2 = again.get_state()
    np.testing.assert_array_equal(costs, costs2)
    np.testing.assert_array_equal(P, P2)
    np.testing.assert_array_equal(X, X2)


LM_LAM0 = 1e4  # every decision of the restatement's ten is then decisive on all three cases (asserted)


@pytest.mark.parametrize("case,k,banded", CASES)
def test_run_lm_parity(ctx, case, k, banded):
    """Ten LM trials from lambda0 = 1e4: with the default lambda0 = 1 the restatement's late decisions
    have margins of 5e-6 .. 1e-4, too close to call against a 1e-5 bound; from 1e4 the smallest margin
    of any decision is above 1e-3 on every case (two of the three runs reject a step on the way), so
    the whole log and the final state are held to the solve bound."""
    _, s, st0 = _case(case)
    prior = _prior(case, k)
    sess = _session(case, ctx, prior)
    rc, c, lam, trial, acc = sess.run_lm(10, lam0=LM_LAM0)
    assert rc == _lib.VO_OK
    P, X = sess.get_state()
    log = pr.solve_lm(st0, s, 10, prior, LM_LAM0)
    print("run_lm(10):", log.pattern(), "margins", " ".join(f"{m:.1e}" for m in log.margins()))
    assert log.margins().min() > 1e-4, "a decision of the restatement too close to call: unfit input"
    assert (np.diff(c) <= 0).all(), "the LM cost never increases"
    for i in range(10):
        if acc[i]:
            assert c[i + 1] == trial[i], "an accepted trial's cost is the next cost, bit for bit"
        else:
            assert c[i + 1] == c[i]
    np.testing.assert_array_equal(acc, log.accepted)
    np.testing.assert_array_equal(lam, log.lam)  # equal decisions: the same two multiplications and clamps
    figs = (_rel(c, log.cost), _rel(trial, log.trial), _rel(P, log.state.poses_cw()), _rel(X, log.state.X))
    print("run_lm(10) errors:", " ".join(f"{v:.2e}" for v in figs))
    assert max(figs) < SOLVE


# 3 ------------------------------------------------------------------------------------------------
def _perturbed(st0, rel=1e-13):
    rng = np.random.default_rng(1)
    return ba_ref.BAState(st0.R.copy(), st0.t * (1 + rel * rng.normal(size=st0.t.shape)),
                          st0.X * (1 + rel * rng.normal(size=st0.X.shape)))


@pytest.mark.parametrize("case,k,fit", [(SMALL, 3, True), (NARROW, 12, False)])
def test_no_fixed_pose_with_a_prior_at_lambda_zero(ctx, case, k, fit):
    """n_fixed = 0, lambda = 0: the gauge is held by the prior alone.  The step is held to the step
    bound on both windows.  Ten undamped iterations are held to the solve bound where the
    restatement itself is fit for it: on NARROW with K = 12 its own result moves by about 1e-4 when
    its start state is perturbed by 1e-13 (the undamped cost first rises, 9.9e5 -> 1.6e6), ten times
    the bound, so there the run must solve and agree over its first step only; that the input is
    unfit is asserted, not assumed."""
    _, s, st0 = _case(case, 0)
    prior = _prior(case, k, 0)
    sess = _session(case, ctx, prior, n_fixed=0, lam=0.0)
    ref = pr.gn_step(st0, s, 0.0, prior)
    _assert_step(_step_figures(sess.gn_step(), ref), f"{case[:3]} n_fixed 0 K {k}")
    sess = _session(case, ctx, prior, n_fixed=0, lam=0.0)
    rc, costs = sess.run(10)
    assert rc == _lib.VO_OK and np.isfinite(costs).all()
    P, X = sess.get_state()
    st, ref_costs = pr.solve(st0, s, 10, 0.0, prior)
    st_p, costs_p = pr.solve(_perturbed(st0), s, 10, 0.0, prior)
    own = max(_rel(costs_p, ref_costs), _rel(st_p.poses_cw(), st.poses_cw()), _rel(st_p.X, st.X))
    figs = (_rel(costs, ref_costs), _rel(P, st.poses_cw()), _rel(X, st.X))
    print(f"n_fixed 0 run(10) errors: {' '.join(f'{v:.2e}' for v in figs)}; the restatement against itself: {own:.2e}")
    if fit:
        assert own < SOLVE / 100 and max(figs) < SOLVE
    else:
        assert own > SOLVE, "the restatement is fit for this input after all: hold the whole run to the bound"
        assert _rel(costs[:2], ref_costs[:2]) < STEP and costs[-1] < costs[0]


# 4 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,k,banded", CASES)
def test_a_zero_prior_is_no_prior(ctx, case, k, banded):
    zero = _prior(case, k, None, True)
    rc, S, b, dc, cost = _session(case, ctx, zero).gn_step()
    rc0, S0, b0, dc0, cost0 = _session(case, ctx, None).gn_step()
    assert rc == rc0 == _lib.VO_OK
    figs = dict(S=_rel(S, S0), b=_rel(b, b0), dc=_rel(dc, dc0), cost=abs(cost - cost0) / cost0)
    _assert_step(figs, f"{case[:3]} zero prior K {k}")


# 5 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [SMALL, NARROW])
def test_a_null_prior_is_vo_ba_setup(ctx, case):
    p, s, st0 = _case(case)

    def run(setup_prior):
        if setup_prior:
            sess = BASession.__new__(BASession)
            sess.ctx, sess.point_ptr, sess.obs_cam, sess.obs_uv = ctx, s.point_ptr, s.obs_cam, s.obs_uv
            sess.n_poses, sess.n_points, sess.n_fixed = p.n_poses, s.n_points, s.n_fixed
            sess._prob = _problem_struct(p.K, sess.point_ptr, sess.obs_cam, sess.obs_uv, p.n_poses, s.n_fixed, LAM)
            sid = C.c_uint64(0)
            _lib.check(ctx.lib.vo_ba_setup_prior(ctx.handle, C.byref(sess._prob), None, C.byref(sid)))
            sess.session = int(sid.value)
            sess.set_state(st0.poses_cw(), st0.X)
        else:
            sess = _session(case, ctx, None)
        stats = sess.plan_stats()
        rc, costs = sess.run(6)
        return rc, costs, sess.get_state(), _lib.ba_testing_last_run(ctx), \
            {k: stats[k] for k in stats if k not in ("setup_us", "reused_groups", "reused_chunks")}  # (not the plan: how it was built)

    a, b = run(True), run(False)
    assert a[0] == b[0] == _lib.VO_OK
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2][0], b[2][0])
    np.testing.assert_array_equal(a[2][1], b[2][1])
    assert a[3] == b[3] and a[4] == b[4]


# 6 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,k,banded", CASES)
def test_covariance_includes_the_prior(ctx, case, k, banded):
    _, s, st0 = _case(case)
    prior = _prior(case, k)
    sess = _session(case, ctx, prior)
    for lam in (0.0, 1.0):
        pose, pts, dense = sess.covariance(lam, dense=True)
        eps, _ = cr.routes_disagreement(st0, s, lam)
        assert eps <= 1e-9
        tol = max(STEP, 100.0 * eps)
        S = cr._system(st0, s, lam, 0.0).S + pr.prior_terms(st0, s, prior)[0]
        cc = scipy.linalg.cho_solve(scipy.linalg.cho_factor(S, lower=True), np.eye(S.shape[0]))
        err = cr.rel_err(dense, 0.5 * (cc + cc.T))
        print(f"{case[:3]} K {k} lam {lam}: eps_ref {eps:.3g} tol {tol:.3g} pose covariance err {err:.3g}")
        assert err <= tol
        np.testing.assert_array_equal(dense, dense.T)
    # nothing but the read-out happened: the run that follows is the run without it
    rc, costs = sess.run(3)
    rc2, costs2 = _session(case, ctx, prior).run(3)
    np.testing.assert_array_equal(costs, costs2)


# 7 ------------------------------------------------------------------------------------------------
def test_sliding_window_ba_honours_the_window_prior(ctx):
    p, s, st0 = _case(SMALL)
    prior = _prior(SMALL, 3)
    obs_pt = np.repeat(np.arange(p.n_points), np.diff(p.point_ptr))
    win = BAWindow(p.poses_cw, p.points, p.obs_uv, p.obs_cam, obs_pt, n_fixed=p.n_fixed,
                   prior=PosePrior(prior.info, prior.rhs, prior.poses0, prior.cost0))
    res = SlidingWindowBA(p.K, iters=5, lam=LAM).optimize(win)
    assert res.status == "ok"
    ref, ref_costs = pr.solve(st0, s, 5, LAM, prior)
    assert max(_rel(res.cost_per_iter, ref_costs), _rel(res.poses_cw, ref.poses_cw()), _rel(res.points, ref.X)) < SOLVE


# 8 ------------------------------------------------------------------------------------------------
def test_bad_priors_and_a_stale_session(ctx):
    p, s, st0 = _case(SMALL)
    good = _prior(SMALL, 3)
    F = p.n_poses - p.n_fixed
    too_many = pr.Prior(np.eye(6 * (F + 1)), np.zeros(6 * (F + 1)), np.tile(np.eye(4), (F + 1, 1, 1)))
    nan_info = pr.Prior(good.info.copy(), good.rhs, good.poses0)
    nan_info.info[4, 2] = np.nan
    inf_rhs = pr.Prior(good.info, np.where(np.arange(18) == 5, np.inf, good.rhs), good.poses0)
    for bad in (too_many, nan_info, inf_rhs, pr.Prior(good.info, good.rhs, good.poses0, float("nan"))):
        with pytest.raises(VoError) as e:
            _session(SMALL, ctx, bad)
        assert e.value.code == _lib.VO_ERR_ARG
    # the upper triangle is not read: a NaN there changes nothing
    upper = pr.Prior(good.info.copy(), good.rhs, good.poses0, good.cost0)
    upper.info[2, 4] = np.nan
    a = _session(SMALL, ctx, upper).gn_step()
    b = _session(SMALL, ctx, good).gn_step()
    for x, y in zip(a[1:4], b[1:4]):
        np.testing.assert_array_equal(x, y)
    stale = _session(SMALL, ctx, good)
    _session(SMALL, ctx, good)
    with pytest.raises(VoError) as e:
        stale.gn_step()
    assert e.value.code == _lib.VO_ERR_STATE
    pc, keep = _prior_struct(PosePrior(good.info, good.rhs, good.poses0, good.cost0))
    pc.reserved = 1
    prob = _problem_struct(p.K, s.point_ptr, s.obs_cam, s.obs_uv, p.n_poses, s.n_fixed, LAM)
    sid = C.c_uint64(0)
    assert ctx.lib.vo_ba_setup_prior(ctx.handle, C.byref(prob), C.byref(pc), C.byref(sid)) == _lib.VO_ERR_ARG


# 9 ---- vo_ba_marginalize -------------------------------------------------------------------------
def _struct_session(s, st, ctx, lam, prior=None, huber=0.0, w=None):
    pp = None if prior is None else PosePrior(prior.info, prior.rhs, prior.poses0, prior.cost0)
    sess = BASession(s.K, s.point_ptr, s.obs_cam, s.obs_uv, s.n_poses, s.n_fixed, lam, ctx, huber=huber, prior=pp)
    sess.set_state(st.poses_cw(), st.X)
    if w is not None:
        sess.set_obs_weights(w)
    return sess


@pytest.mark.parametrize("robust", [False, True], ids=["plain", "huber+weights+prior"])
@pytest.mark.parametrize("n_drop", [1, 3])
@pytest.mark.parametrize("case", [SMALL, NARROW])
def test_marginalize_parity_and_nothing_else_written(ctx, case, n_drop, robust):
    """info, rhs and cost0 against the restatement, the mask exactly; n_drop = 1 eliminates no pose
    (m = 0), n_drop = n_fixed + 1 one.  The robust variant also folds a session prior in."""
    _, s, st0 = _case(case)
    assert n_drop in (1, s.n_fixed + 1)
    delta, w, prior = (DELTA, _weights(case), _prior(case, 3)) if robust else (0.0, None, None)
    lam_m = 0.5
    sess = _struct_session(s, st0, ctx, LAM, prior, delta, w)
    new, mask = sess.marginalize(n_drop, lam_m)
    ref, k, ref_mask, ref_info, ref_rhs = pr.marginalize(st0, s, n_drop, prior, w, delta, lam_m)
    np.testing.assert_array_equal(mask, ref_mask)
    assert new is not None and new.n_poses == k
    figs = dict(info=_rel(new.info, ref.info), rhs=_rel(new.rhs, ref.rhs), cost0=abs(new.cost0 - ref.cost0) / ref.cost0)
    print(f"{case[:3]} n_drop {n_drop} K {k} {int(mask.sum())} landmarks: errors", {a: f"{v:.2e}" for a, v in figs.items()})
    assert max(figs.values()) < STEP
    np.testing.assert_array_equal(new.info, new.info.T)
    m = max(0, n_drop - s.n_fixed)
    np.testing.assert_array_equal(new.poses0, st0.poses_cw()[s.n_fixed + m:s.n_fixed + m + k])
    # the call wrote nothing: state, weights and the run that follows are those of a session without it
    P, X = sess.get_state()
    np.testing.assert_array_equal(P, st0.poses_cw())
    np.testing.assert_array_equal(X, st0.X)
    if w is not None:
        np.testing.assert_array_equal(sess.obs_weights(), w)
    rc, costs = sess.run(3)
    after = sess.get_state()
    other = _struct_session(s, st0, ctx, LAM, prior, delta, w)  # (replaces sess on the context)
    rc2, costs2 = other.run(3)
    assert rc == rc2 == _lib.VO_OK
    np.testing.assert_array_equal(costs, costs2)
    for a, b in zip(after, other.get_state()):
        np.testing.assert_array_equal(a, b)
    # two calls at one state agree bit for bit
    again, mask2 = other.marginalize(n_drop, lam_m)
    third, _ = other.marginalize(n_drop, lam_m)
    np.testing.assert_array_equal(again.info, third.info)
    np.testing.assert_array_equal(again.rhs, third.rhs)


@pytest.mark.parametrize("n_drop", [1, 3])
@pytest.mark.parametrize("case", [SMALL, NARROW])
def test_marginalisation_identity_on_the_device(ctx, case, n_drop):
    """One GN step of the full window against one of the reduced window under the device's own
    prior, both at lambda = 0 from the same state: the remaining poses get the same update, within
    max(1e-8, 100 x the CPU routes' own disagreement) of max |dc|."""
    _, s, st0 = _case(case)
    st = pr.gn_step(st0, s, 1.0, None).state
    eps, full, _, k, ref_mask, _, s2, st2 = pr.slide_identity(st, s, n_drop)
    tol = max(STEP, 100.0 * eps)
    sess = _struct_session(s, st, ctx, 0.0)
    new, mask = sess.marginalize(n_drop, 0.0)
    np.testing.assert_array_equal(mask, ref_mask)
    rc, _, _, dc_full, _ = sess.gn_step()
    assert rc == _lib.VO_OK
    red = _struct_session(s2, st2, ctx, 0.0, pr.Prior(new.info, new.rhs, new.poses0, new.cost0))
    rc, _, _, dc_red, _ = red.gn_step()
    assert rc == _lib.VO_OK
    m = 6 * max(0, n_drop - s.n_fixed)
    err = np.abs(dc_full[m:] - dc_red).max() / np.abs(dc_full).max()
    print(f"{case[:3]} n_drop {n_drop}: CPU routes {eps:.2e}, tol {tol:.2e}, device full against reduced {err:.2e}, "
          f"device against CPU dc {_rel(dc_full, full.dc):.2e}")
    assert err < tol


def test_three_chained_slides(ctx):
    """A drive of 11 cameras, windows of 8 sliding by one: each window is solved under the prior the
    last one left, then marginalises its oldest camera; n_fixed goes 2 -> 1 -> 0 -> 0.  The device
    chain and the restatement's chain (each on its own priors and states) agree within the solve
    bound at every slide."""
    d = make_ba_problem(11, 420, 33)
    obs_pt = np.repeat(np.arange(d.points.shape[0]), np.diff(d.point_ptr))

    def chain(gpu):
        gone = np.zeros(d.points.shape[0], bool)
        poses, points = d.poses_cw.copy(), d.points.copy()
        prior, nf, out = None, d.n_fixed, []
        for j in range(4):
            inw = (d.obs_cam >= j) & (d.obs_cam < j + 8) & ~gone[obs_pt]
            cnt = np.bincount(obs_pt[inw], minlength=gone.size)
            idx = np.flatnonzero(cnt >= 2)
            sel = inw & (cnt >= 2)[obs_pt]
            ptr_ = np.zeros(idx.size + 1, np.int32)
            ptr_[1:] = np.cumsum(cnt[idx])
            s = ba_ref.BAStructure(d.K, ptr_, (d.obs_cam[sel] - j).astype(np.int32), d.obs_uv[sel].copy(), nf, 8)
            st = ba_ref.BAState.from_poses(poses[j:j + 8], points[idx])
            if gpu:
                sess = _struct_session(s, st, ctx, LAM, prior)
                rc, costs = sess.run(5)
                assert rc == _lib.VO_OK
                P, X = sess.get_state()
                new, mask = sess.marginalize(1, LAM)
                prior = None if new is None else pr.Prior(new.info, new.rhs, new.poses0, new.cost0)
            else:
                st5, costs = pr.solve(st, s, 5, LAM, prior)
                P, X = st5.poses_cw(), st5.X
                prior, _, mask, _, _ = pr.marginalize(st5, s, 1, prior, None, 0.0, LAM)
            poses[j:j + 8], points[idx] = P, X
            gone[idx[mask]] = True
            out.append((costs, P, X, prior, nf, int(mask.sum())))
            nf = max(0, nf - 1)
        return out

    for j, (g, r) in enumerate(zip(chain(True), chain(False))):
        figs = [_rel(g[0], r[0]), _rel(g[1], r[1]), _rel(g[2], r[2]), _rel(g[3].info, r[3].info), _rel(g[3].rhs, r[3].rhs),
                abs(g[3].cost0 - r[3].cost0) / r[3].cost0]
        print(f"slide {j}: n_fixed {g[4]}, {g[5]} landmarks marginalised, K {g[3].k}, errors", " ".join(f"{v:.2e}" for v in figs))
        assert g[4:] == r[4:] and g[3].k == r[3].k and max(figs) < SOLVE
    assert [g[4] for g in chain(False)[:3]] == [2, 1, 0]


def test_marginalize_errors(ctx):
    _, s, st0 = _case(SMALL)
    sess = _struct_session(s, st0, ctx, LAM)
    for n_drop, lam in ((0, 0.0), (s.n_poses, 0.0), (-1, 0.0), (1, -1.0), (1, float("nan"))):
        with pytest.raises(VoError) as e:
            sess.marginalize(n_drop, lam)
        assert e.value.code == _lib.VO_ERR_ARG
    # not positive definite: the eliminated pose sees nothing but fixed-camera-free noise -- every
    # weight zero leaves its block exactly zero at lambda = 0
    sess.set_obs_weights(np.zeros(s.obs_cam.size))
    k, cost0 = C.c_int32(5), C.c_double(0.0)
    r = s.n_free - 1
    info, rhs, poses0 = np.zeros((6 * r, 6 * r)), np.zeros(6 * r), np.zeros((r, 12))
    mask = np.ones(s.n_points, np.uint8)
    rc = ctx.lib.vo_ba_marginalize(ctx.handle, sess.session, 3, 0.0, C.byref(k), _lib.ptr(info, C.c_double),
                                   _lib.ptr(rhs, C.c_double), _lib.ptr(poses0, C.c_double), C.byref(cost0),
                                   _lib.ptr(mask, C.c_uint8))
    assert rc == _lib.VO_ERR_NOT_SPD
    assert np.isnan(info).all() and np.isnan(rhs).all() and np.isnan(poses0).all() and np.isnan(cost0.value)
    assert k.value == 0 and not mask.any(), "no active observation in a dropped camera: nothing is marked"
    # the session stays usable
    sess.set_obs_weights(None)
    new, mask = sess.marginalize(3, 0.0)
    assert new is not None and np.isfinite(new.info).all() and mask.any()
    rc, costs = sess.run(2)
    assert rc == _lib.VO_OK and np.isfinite(costs).all()
    stale = sess
    _struct_session(s, st0, ctx, LAM)
    with pytest.raises(VoError) as e:
        stale.marginalize(1)
    assert e.value.code == _lib.VO_ERR_STATE


# 10 ---- the keyframe hook on the real engine ------------------------------------------------------
def test_keyframe_hook_slides_on_the_real_engine(ctx):
    """``cfg.ba_marginalize`` through ``run_window_ba`` with the real ``SlidingWindowBA``: a drive of
    12 keyframes over windows of 8.  Every window is adjusted (none skipped or rejected: the prior's K
    fits the next window's free poses, the absorbed ids map back through ``lm_ids``), each full window
    hands its prior to the next, n_fixed goes 2 -> 1 -> 0, and the absorbed landmarks stay out."""
    from tests.test_dropin_marginalize_host import FakeVO
    from visualodometry_amd.dropin.config.config import VOConfig
    from visualodometry_amd.dropin.hooks import KeyframeWindow, run_window_ba

    d = make_ba_problem(12, 450, 41)
    obs_pt = np.repeat(np.arange(d.points.shape[0]), np.diff(d.point_ptr))
    cfg = VOConfig()
    cfg.ba_enabled, cfg.ba_window, cfg.ba_fixed, cfg.ba_iters, cfg.ba_lambda, cfg.ba_marginalize = True, 8, 2, 5, LAM, True
    seen = []

    class Spy(SlidingWindowBA):
        def optimize(self, window, **kw):
            res = super().optimize(window, **kw)
            seen.append((window, kw, res))
            return res

    vo = FakeVO(cfg, Spy(d.K, cfg))
    vo.map_points = {int(i): d.points[i].copy() for i in range(d.points.shape[0])}
    win = KeyframeWindow(cfg.ba_window, cfg.ba_fixed)
    for k in range(d.poses_cw.shape[0]):
        o = d.obs_cam == k
        win.add(np.linalg.inv(d.poses_cw[k]), d.obs_uv[o], obs_pt[o])
        res = run_window_ba(vo, win)
        if k >= cfg.ba_fixed:
            assert res is not None and res.status == "ok", (k, res and res.message)
            assert np.isfinite(res.cost_per_iter).all() and res.cost_per_iter[-1] <= res.cost_per_iter[0]
    full = [i for i, (w, kw, r) in enumerate(seen) if kw.get("marginalize")]
    assert len(full) == 5 and full == list(range(full[0], len(seen))), "every full window marginalises"
    assert [seen[i][0].n_fixed for i in full] == [2, 1, 0, 0, 0]
    absorbed = set()
    for i in full:
        w, kw, r = seen[i]
        assert w.poses_cw.shape[0] == 8 and (w.prior is None) == (i == full[0])
        assert r.prior is not None and r.point_marginalised.any()
        if i + 1 < len(seen):
            nxt = seen[i + 1][0]
            assert nxt.prior is r.prior and nxt.prior.n_poses <= nxt.poses_cw.shape[0] - nxt.n_fixed
            # the prior's linearisation poses are the adjusted poses of the cameras it covers, one slot down
            first = nxt.n_fixed
            np.testing.assert_array_equal(r.prior.poses0, r.poses_cw[first + 1:first + 1 + r.prior.n_poses])
    kf, uv, pid = win.observations(vo.map_points)
    assert win.marginalised and not set(pid.tolist()) & win.marginalised
    held = set(np.concatenate([fr.ids for fr in win.frames]).tolist())
    assert win.marginalised <= held, "ids no frame of the window sees any more are pruned"


def test_optimize_keeps_its_solve_when_the_marginalisation_is_refused(ctx, monkeypatch):
    p, s, st0 = _case(SMALL)
    obs_pt = np.repeat(np.arange(p.n_points), np.diff(p.point_ptr))
    win = BAWindow(p.poses_cw, p.points, p.obs_uv, p.obs_cam, obs_pt, n_fixed=p.n_fixed)
    ba = SlidingWindowBA(p.K, iters=3, lam=LAM)
    good = ba.optimize(win, marginalize=1)
    assert good.status == "ok" and good.prior is not None
    for code in (_lib.VO_ERR_ARG, _lib.VO_ERR_STATE, _lib.VO_ERR_NOT_SPD):
        def refuse(self, n_drop, lam=0.0, code=code):
            raise VoError(code, "refused")
        monkeypatch.setattr(BASession, "marginalize", refuse)
        res = ba.optimize(win, marginalize=1)
        assert res.status == "ok" and res.prior is None and res.point_marginalised is None
        np.testing.assert_array_equal(res.cost_per_iter, good.cost_per_iter)
        np.testing.assert_array_equal(res.poses_cw, good.poses_cw)
