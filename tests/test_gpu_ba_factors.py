"""Pose factors on the MI355X (``vo_ba_setup_factors``), against the CPU restatement
(tests/ba_factor_ref.py).

Inputs: the prior tests' smallest windows, SMALL = ``make_ba_problem(8, 300, 21)`` (6 free poses)
and NARROW = ``make_ba_problem(16, 400, 5, max_track=4)`` (14 free poses).  Factor sets: *chain* --
every consecutive pair of cameras (so a fixed-fixed and a fixed-free pair are in it), the last pair
once more the other way round, and one unary factor --, and *far* -- chain plus a factor between
free poses 0 and 13 of NARROW, which takes the window off the banded solver.  The measurements are
the true relative poses moved by twists of about 1e-2; Lambda = s (M^T M + I) from a seeded
generator, s chosen so that Lambda is of the order of the reduced system's own diagonal (factors
that vanish beside S would pass every parity check without being applied:
``test_the_factors_move_the_step`` holds that they do not).

Bounds: the project's -- 1e-8 of the largest entry per step (``test_gpu_ba_prior.py``'s
``_step_figures`` scaling), 1e-5 over a solve, the covariance by ``test_gpu_ba_cov.py``'s rule
max(1e-8, 100 x the CPU routes' own disagreement).  Where two runs launch the same kernels on the same
plan the comparison is bit for bit.
"""

import ctypes as C
import functools
import threading

import numpy as np
import pytest
import scipy.linalg

from oracle import ba_ref
from tests import ba_cov_ref as cr
from tests import ba_factor_ref as fr
from tests import ba_prior_ref as pr
from tests.test_gpu_ba_prior import _assert_step, _prior, _rel, _step_figures, _weights
from visualodometry_amd import _lib
from visualodometry_amd._lib import VoError
from visualodometry_amd.ba import BASession, BAWindow, PoseFactor, PosePrior, SlidingWindowBA, _problem_struct
from visualodometry_amd.synthetic import make_ba_problem

pytestmark = pytest.mark.gpu

LAM, DELTA = 1.0, 2.0
STEP, SOLVE = 1e-8, 1e-5
SMALL, NARROW = (8, 300, 21, ()), (16, 400, 5, (("max_track", 4),))
# (window, factor set, banded solver expected)
CASES = [(SMALL, "chain", True), (NARROW, "chain", True), (NARROW, "far", False)]


@functools.lru_cache(maxsize=None)
def _case(case, n_fixed=None):
    n, L, seed, kw = case
    p = make_ba_problem(n, L, seed, **dict(kw))
    nf = p.n_fixed if n_fixed is None else n_fixed
    s = ba_ref.BAStructure(p.K, p.point_ptr, p.obs_cam, p.obs_uv, nf, p.n_poses)
    return p, s, ba_ref.BAState.from_poses(p.poses_cw, p.points)


def _scale(case, n_fixed=None):
    """Lambda's scale: the mean of the reduced system's diagonal over the 6 of M^T M + I's."""
    _, s, st0 = _case(case, n_fixed)
    return float(np.diag(ba_ref.build_system(st0, s, 1.0).S).mean()) / 6.0


@functools.lru_cache(maxsize=None)
def _factors(case, which, zero=False):
    p, s, _ = _case(case)
    N, nf = p.n_poses, p.n_fixed
    pairs = [(i + 1, i) for i in range(N - 1)] + [(N - 2, N - 1), (nf + 2, -1)]
    if which == "far":
        assert s.n_free == 14
        pairs.append((nf + 13, nf))
    out = fr.make_factors(p.poses_cw, pairs, 11 + case[2], 1e-2, _scale(case))
    if zero:
        out = [fr.Factor(f.cam_i, f.cam_j, f.meas, np.zeros((6, 6))) for f in out]
    return tuple(out)


def _pf(factors):
    return [PoseFactor(f.cam_i, f.cam_j, f.meas, f.info) for f in factors]


def _pp(prior):
    return None if prior is None else PosePrior(prior.info, prior.rhs, prior.poses0, prior.cost0)


def _struct_session(s, st, ctx, lam, factors, prior=None, huber=0.0, w=None):
    sess = BASession(s.K, s.point_ptr, s.obs_cam, s.obs_uv, s.n_poses, s.n_fixed, lam, ctx, huber=huber, prior=_pp(prior),
                     factors=None if factors is None else _pf(factors))
    sess.set_state(st.poses_cw(), st.X)
    if w is not None:
        sess.set_obs_weights(w)
    return sess


def _session(case, ctx, factors, prior=None, huber=0.0, n_fixed=None, lam=LAM, w=None):
    _, s, st0 = _case(case, n_fixed)
    return _struct_session(s, st0, ctx, lam, factors, prior, huber, w)


# 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robust", [False, True], ids=["plain", "huber+weights+prior"])
@pytest.mark.parametrize("case,which,banded", CASES)
def test_gn_step_parity(ctx, case, which, banded, robust):
    _, s, st0 = _case(case)
    factors = _factors(case, which)
    delta, w, prior = (DELTA, _weights(case), _prior(case, 3)) if robust else (0.0, None, None)
    sess = _session(case, ctx, factors, prior, huber=delta, w=w)
    assert sess.plan_stats()["band_solver"] == (1 if banded else 0)
    ref = fr.gn_step(st0, s, LAM, factors, prior, w, delta)
    figs = _step_figures(sess.gn_step(), ref)
    P, X = sess.get_state()
    figs.update(P=_rel(P, ref.state.poses_cw()), X=_rel(X, ref.state.X))
    _assert_step(figs, f"{case[:3]} {which} {'huber+weights+prior' if robust else 'plain'}")


# 2 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,which,banded", CASES)
def test_the_factors_move_the_step(ctx, case, which, banded):
    """The factors are no rounding matter: on the device the step with them differs from the step
    without them by orders of magnitude more than any bound here, in S, b, dc and the cost."""
    a = _session(case, ctx, _factors(case, which)).gn_step()
    b = _session(case, ctx, None).gn_step()
    assert a[0] == b[0] == _lib.VO_OK
    for x, y in zip(a[1:4], b[1:4]):
        assert _rel(x, y) > 1e-2
    assert abs(a[4] - b[4]) > 1.0


# 3 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,which,banded", CASES)
def test_run_parity_and_repeatable(ctx, case, which, banded):
    _, s, st0 = _case(case)
    factors = _factors(case, which)
    sess = _session(case, ctx, factors)
    rc, costs = sess.run(5)
    assert rc == _lib.VO_OK
    chained, launches = _lib.ba_testing_last_run(ctx)
    assert not chained and launches == 10, "a session with factors: a K1 launch and a solve launch per iteration"
    P, X = sess.get_state()
    ref, ref_costs = fr.solve(st0, s, 5, LAM, factors)
    figs = (_rel(costs, ref_costs), _rel(P, ref.poses_cw()), _rel(X, ref.X))
    print("run(5) errors:", " ".join(f"{v:.2e}" for v in figs))
    assert max(figs) < SOLVE
    again = _session(case, ctx, factors)
    rc, costs2 = again.run(5)
    P2, X2 = again.get_state()
    np.testing.assert_array_equal(costs, costs2)
    np.testing.assert_array_equal(P, P2)
    np.testing.assert_array_equal(X, X2)


# 4 ------------------------------------------------------------------------------------------------
LM_LAM0, LM_ITERS = 1e-4, 8  # the restatement rejects its first steps from there, every decision decisive (asserted)


@pytest.mark.parametrize("case,which,banded", CASES)
def test_run_lm_parity_with_a_rejection(ctx, case, which, banded):
    _, s, st0 = _case(case)
    factors = _factors(case, which)
    sess = _session(case, ctx, factors)
    rc, c, lam, trial, acc = sess.run_lm(LM_ITERS, lam0=LM_LAM0)
    assert rc == _lib.VO_OK
    P, X = sess.get_state()
    log = fr.solve_lm(st0, s, LM_ITERS, factors, LM_LAM0)
    print(f"run_lm({LM_ITERS}):", log.pattern(), "margins", " ".join(f"{m:.1e}" for m in log.margins()))
    assert log.margins().min() > 1e-4, "a decision of the restatement too close to call: unfit input"
    assert 0 in log.accepted and 1 in log.accepted, "the input must reject a step and accept one"
    assert (np.diff(c) <= 0).all(), "the LM cost never increases"
    for i in range(LM_ITERS):
        assert c[i + 1] == (trial[i] if acc[i] else c[i])
    np.testing.assert_array_equal(acc, log.accepted)
    np.testing.assert_array_equal(lam, log.lam)
    figs = (_rel(c, log.cost), _rel(trial, log.trial), _rel(P, log.state.poses_cw()), _rel(X, log.state.X))
    print("run_lm errors:", " ".join(f"{v:.2e}" for v in figs))
    assert max(figs) < SOLVE
    # a rejected step restores poses and points bit for bit: the state behind trial r (rejected) is
    # the state behind trial r - 1
    r = int(np.flatnonzero(log.accepted == 0)[-1])
    states = []
    for n in (r, r + 1):
        one = _session(case, ctx, factors)
        rc, _, _, _, a = one.run_lm(n, lam0=LM_LAM0)
        assert rc == _lib.VO_OK
        states.append(one.get_state())
    assert a[-1] == 0
    np.testing.assert_array_equal(states[0][0], states[1][0])
    np.testing.assert_array_equal(states[0][1], states[1][1])


# 5 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [SMALL, NARROW])
def test_unary_factors_are_a_block_diagonal_prior_on_the_device(ctx, case):
    _, s, st0 = _case(case)
    k, nf = 3, s.n_fixed
    rng = np.random.default_rng(5)
    info = np.zeros((6 * k, 6 * k))
    poses0 = _prior(case, k).poses0  # the initial poses moved by twists of about 1e-2
    factors = []
    for f in range(k):
        M = rng.normal(size=(6, 6))
        L = _scale(case) * (M.T @ M + np.eye(6))
        info[6 * f:6 * f + 6, 6 * f:6 * f + 6] = L
        factors.append(fr.Factor(nf + f, -1, poses0[f], L))
    prior = pr.Prior(info, np.zeros(6 * k), poses0, 0.0)
    rc, S, b, dc, cost = _session(case, ctx, factors).gn_step()
    rc0, S0, b0, dc0, cost0 = _session(case, ctx, None, prior).gn_step()
    plain = _session(case, ctx, None).gn_step()
    assert rc == rc0 == _lib.VO_OK
    figs = dict(S=_rel(S, S0), b=_rel(b, b0), dc=_rel(dc, dc0), cost=abs(cost - cost0) / cost0)
    _assert_step(figs, f"{case[:3]} unary factors against the prior")
    assert _rel(dc, plain[3]) > 1e-2 and abs(cost - plain[4]) > 1.0, "neither is applied"


# 6 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,which,banded", CASES)
def test_zero_information_factors_are_no_factors(ctx, case, which, banded):
    rc, S, b, dc, cost = _session(case, ctx, _factors(case, which, True)).gn_step()
    rc0, S0, b0, dc0, cost0 = _session(case, ctx, None).gn_step()
    assert rc == rc0 == _lib.VO_OK
    figs = dict(S=_rel(S, S0), b=_rel(b, b0), dc=_rel(dc, dc0), cost=abs(cost - cost0) / cost0)
    _assert_step(figs, f"{case[:3]} zero-information {which}")


# 7 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [SMALL, NARROW])
def test_no_factors_and_a_null_prior_is_vo_ba_setup(ctx, case):
    p, s, st0 = _case(case)

    def run(setup_factors):
        if setup_factors:
            sess = BASession.__new__(BASession)
            sess.ctx, sess.point_ptr, sess.obs_cam, sess.obs_uv = ctx, s.point_ptr, s.obs_cam, s.obs_uv
            sess.n_poses, sess.n_points, sess.n_fixed = p.n_poses, s.n_points, s.n_fixed
            sess._prob = _problem_struct(p.K, sess.point_ptr, sess.obs_cam, sess.obs_uv, p.n_poses, s.n_fixed, LAM)
            sid = C.c_uint64(0)
            _lib.check(ctx.lib.vo_ba_setup_factors(ctx.handle, C.byref(sess._prob), None, None, 0, C.byref(sid)))
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


# 8 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,which,banded", CASES)
def test_covariance_includes_the_factors(ctx, case, which, banded):
    _, s, st0 = _case(case)
    factors = _factors(case, which)
    sess = _session(case, ctx, factors)
    plain = _session(case, ctx, None).covariance(0.0, dense=True)[2]
    sess = _session(case, ctx, factors)
    for lam in (0.0, 1.0):
        pose, pts, dense = sess.covariance(lam, dense=True)
        eps, _ = cr.routes_disagreement(st0, s, lam)
        assert eps <= 1e-9
        tol = max(STEP, 100.0 * eps)
        S = cr._system(st0, s, lam, 0.0).S + fr.factor_terms(st0, s, factors)[0]
        cc = scipy.linalg.cho_solve(scipy.linalg.cho_factor(S, lower=True), np.eye(S.shape[0]))
        err = cr.rel_err(dense, 0.5 * (cc + cc.T))
        print(f"{case[:3]} {which} lam {lam}: eps_ref {eps:.3g} tol {tol:.3g} pose covariance err {err:.3g}")
        assert err <= tol
        np.testing.assert_array_equal(dense, dense.T)
        if lam == 0.0:
            assert cr.rel_err(dense, plain) > 1e-2, "the factors do not show in the covariance"
    # nothing but the read-out happened: the run that follows is the run without it
    rc, costs = sess.run(3)
    rc2, costs2 = _session(case, ctx, factors).run(3)
    np.testing.assert_array_equal(costs, costs2)


# 9 ---- vo_ba_marginalize -------------------------------------------------------------------------
@pytest.mark.parametrize("robust", [False, True], ids=["plain", "huber+weights+prior"])
@pytest.mark.parametrize("n_drop", [1, 3])
@pytest.mark.parametrize("case", [SMALL, NARROW])
def test_marginalize_parity_and_nothing_else_written(ctx, case, n_drop, robust):
    _, s, st0 = _case(case)
    factors = _factors(case, "chain")
    delta, w, prior = (DELTA, _weights(case), _prior(case, 3)) if robust else (0.0, None, None)
    lam_m = 0.5
    sess = _struct_session(s, st0, ctx, LAM, factors, prior, delta, w)
    new, mask = sess.marginalize(n_drop, lam_m)
    ref, k, ref_mask, ref_info, ref_rhs = fr.marginalize(st0, s, n_drop, factors, prior, w, delta, lam_m)
    bare = pr.marginalize(st0, s, n_drop, prior, w, delta, lam_m)[0]
    np.testing.assert_array_equal(mask, ref_mask)
    assert new is not None and new.n_poses == k
    figs = dict(info=_rel(new.info, ref.info), rhs=_rel(new.rhs, ref.rhs), cost0=abs(new.cost0 - ref.cost0) / ref.cost0)
    print(f"{case[:3]} n_drop {n_drop} K {k}: errors", {a: f"{v:.2e}" for a, v in figs.items()})
    assert max(figs.values()) < STEP
    assert abs(ref.cost0 - bare.cost0) > 1.0, "the marginalised factors do not show in cost0"
    np.testing.assert_array_equal(new.info, new.info.T)
    # the call wrote nothing: state, weights and the run that follows are those of a session without it
    P, X = sess.get_state()
    np.testing.assert_array_equal(P, st0.poses_cw())
    np.testing.assert_array_equal(X, st0.X)
    if w is not None:
        np.testing.assert_array_equal(sess.obs_weights(), w)
    rc, costs = sess.run(3)
    after = sess.get_state()
    other = _struct_session(s, st0, ctx, LAM, factors, prior, delta, w)
    rc2, costs2 = other.run(3)
    assert rc == rc2 == _lib.VO_OK
    np.testing.assert_array_equal(costs, costs2)
    for a, b in zip(after, other.get_state()):
        np.testing.assert_array_equal(a, b)
    again, _ = other.marginalize(n_drop, lam_m)
    third, _ = other.marginalize(n_drop, lam_m)
    np.testing.assert_array_equal(again.info, third.info)
    np.testing.assert_array_equal(again.rhs, third.rhs)


@pytest.mark.parametrize("n_drop", [1, 3])
@pytest.mark.parametrize("case", [SMALL, NARROW])
def test_marginalisation_identity_on_the_device(ctx, case, n_drop):
    """One GN step of the full window with its factors against one of the reduced window under the
    device's own prior and the remaining factors, both at lambda = 0 from the same state: within
    max(1e-8, 100 x the CPU routes' own disagreement) of max |dc|, the existing identity test's bound."""
    _, s, st0 = _case(case)
    factors = _factors(case, "chain")
    st = fr.gn_step(st0, s, 1.0, factors).state
    eps, full, _, k, ref_mask, _, s2, st2, f2 = fr.slide_identity(st, s, n_drop, factors)
    tol = max(STEP, 100.0 * eps)
    sess = _struct_session(s, st, ctx, 0.0, factors)
    new, mask = sess.marginalize(n_drop, 0.0)
    np.testing.assert_array_equal(mask, ref_mask)
    rc, _, _, dc_full, _ = sess.gn_step()
    assert rc == _lib.VO_OK
    red = _struct_session(s2, st2, ctx, 0.0, f2, pr.Prior(new.info, new.rhs, new.poses0, new.cost0))
    rc, _, _, dc_red, _ = red.gn_step()
    assert rc == _lib.VO_OK
    m = 6 * max(0, n_drop - s.n_fixed)
    err = np.abs(dc_full[m:] - dc_red).max() / np.abs(dc_full).max()
    print(f"{case[:3]} n_drop {n_drop}: CPU routes {eps:.2e}, tol {tol:.2e}, device full against reduced {err:.2e}, "
          f"{len(factors) - len(f2)} factors marginalised")
    assert err < tol


# 10 -----------------------------------------------------------------------------------------------
def test_unary_factors_hold_the_gauge(ctx):
    """n_fixed = 0, lambda = 0, unary factors on two poses: the solve succeeds and matches the
    restatement (whose own result moves by 1.5e-9 under a 1e-13 perturbation of its start: fit for the
    solve bound); without the factors the system is singular."""
    p, s, st0 = _case(SMALL, 0)
    factors = fr.make_factors(p.poses_cw, [(0, -1), (1, -1)], 5, 1e-2, _scale(SMALL, 0))
    sess = _session(SMALL, ctx, factors, n_fixed=0, lam=0.0)
    _assert_step(_step_figures(sess.gn_step(), fr.gn_step(st0, s, 0.0, factors)), "n_fixed 0, unary gauge")
    sess = _session(SMALL, ctx, factors, n_fixed=0, lam=0.0)
    rc, costs = sess.run(5)
    assert rc == _lib.VO_OK and np.isfinite(costs).all()
    P, X = sess.get_state()
    st, ref_costs = fr.solve(st0, s, 5, 0.0, factors)
    figs = (_rel(costs, ref_costs), _rel(P, st.poses_cw()), _rel(X, st.X))
    print("n_fixed 0 run(5) errors:", " ".join(f"{v:.2e}" for v in figs))
    assert max(figs) < SOLVE
    bare = _session(SMALL, ctx, None, n_fixed=0, lam=0.0)
    rc, S, b, dc, cost = bare.gn_step()
    with pytest.raises(np.linalg.LinAlgError):
        ba_ref.gn_step(st0, s, 0.0)
    assert rc == _lib.VO_ERR_NOT_SPD or not (_rel(dc, fr.gn_step(st0, s, 0.0, factors).dc) <= SOLVE)


# 11 -----------------------------------------------------------------------------------------------
def test_session_errors(ctx):
    p, s, st0 = _case(SMALL)
    factors = _factors(SMALL, "chain")
    stale = _session(SMALL, ctx, factors)
    _session(SMALL, ctx, factors)
    with pytest.raises(VoError) as e:
        stale.gn_step()
    assert e.value.code == _lib.VO_ERR_STATE
    # an indefinite Lambda large enough to break S: VO_ERR_NOT_SPD, and the session stays usable
    bad = list(factors) + [fr.Factor(s.n_fixed + 1, -1, p.poses_cw[s.n_fixed + 1], -1e3 * _scale(SMALL) * np.eye(6))]
    sess = _session(SMALL, ctx, bad)
    rc, S, b, dc, cost = sess.gn_step()
    assert rc == _lib.VO_ERR_NOT_SPD
    P, X = sess.get_state()
    np.testing.assert_array_equal(P, st0.poses_cw())
    err2, depth = sess.residuals()
    assert np.isfinite(err2).all()
    sess.set_state(st0.poses_cw(), st0.X)
    rc, costs = sess.run(2)
    assert rc == _lib.VO_ERR_NOT_SPD
    with pytest.raises(VoError) as e:
        sess.covariance(0.0)
    assert e.value.code == _lib.VO_ERR_NOT_SPD
    # and the context: the next session on it solves
    rc, costs = _session(SMALL, ctx, factors).run(2)
    assert rc == _lib.VO_OK and np.isfinite(costs).all()


def test_two_ranks_are_refused():
    """Factors over landmark shards are not built: with a two-rank (loopback) communicator every
    rank's setup gets VO_ERR_STATE, ahead of any collective."""
    p, s, st0 = _case(SMALL)
    factors = _pf(_factors(SMALL, "chain"))
    nranks, codes, errors = 2, [None, None], []

    def worker(r):
        try:
            c = _lib.Context(0)
            _lib.comm_init_loopback(c, nranks, r, b"vo-loopback-factors")
            try:
                BASession(p.K, s.point_ptr, s.obs_cam, s.obs_uv, p.n_poses, s.n_fixed, LAM, c, factors=factors)
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


# 12 -----------------------------------------------------------------------------------------------
def test_sliding_window_ba_honours_the_window_factors(ctx):
    p, s, st0 = _case(SMALL)
    factors = _factors(SMALL, "chain")
    obs_pt = np.repeat(np.arange(p.n_points), np.diff(p.point_ptr))
    win = BAWindow(p.poses_cw, p.points, p.obs_uv, p.obs_cam, obs_pt, n_fixed=p.n_fixed, factors=_pf(factors))
    res = SlidingWindowBA(p.K, iters=5, lam=LAM).optimize(win)
    assert res.status == "ok"
    ref, ref_costs = fr.solve(st0, s, 5, LAM, factors)
    assert max(_rel(res.cost_per_iter, ref_costs), _rel(res.poses_cw, ref.poses_cw()), _rel(res.points, ref.X)) < SOLVE
    plain = SlidingWindowBA(p.K, iters=5, lam=LAM).optimize(BAWindow(p.poses_cw, p.points, p.obs_uv, p.obs_cam, obs_pt,
                                                                     n_fixed=p.n_fixed))
    assert _rel(res.cost_per_iter, plain.cost_per_iter) > 1e-3


def test_keyframe_hook_with_motion_factors_slides_on_the_real_engine(ctx):
    """``cfg.ba_motion_factors`` and ``cfg.ba_marginalize`` through ``run_window_ba`` with the real
    ``SlidingWindowBA``: a drive of 11 keyframes over windows of 8, three slides behind the first full
    window.  Every window is adjusted, every window carries the chain over its own consecutive pairs,
    and no recorded pair is counted twice: the one pair a slide marginalises (cameras 0 and 1) is in no
    later window."""
    from tests.test_dropin_marginalize_host import FakeVO
    from visualodometry_amd.dropin.config.config import VOConfig
    from visualodometry_amd.dropin.hooks import KeyframeWindow, run_window_ba

    d = make_ba_problem(11, 420, 33)
    obs_pt = np.repeat(np.arange(d.points.shape[0]), np.diff(d.point_ptr))
    cfg = VOConfig()
    cfg.ba_enabled, cfg.ba_window, cfg.ba_fixed, cfg.ba_iters, cfg.ba_lambda, cfg.ba_marginalize = True, 8, 2, 5, LAM, True
    cfg.ba_motion_factors, cfg.ba_motion_sigma_t, cfg.ba_motion_sigma_r = True, 0.05, 0.01
    seen = []

    class Spy(SlidingWindowBA):
        def optimize(self, window, **kw):
            res = super().optimize(window, **kw)
            seen.append((window, kw, res))
            return res

    vo = FakeVO(cfg, Spy(d.K, cfg))
    vo.map_points = {int(i): d.points[i].copy() for i in range(d.points.shape[0])}
    win = KeyframeWindow(cfg.ba_window, cfg.ba_fixed, motion_factors=True, motion_sigma_t=cfg.ba_motion_sigma_t,
                         motion_sigma_r=cfg.ba_motion_sigma_r)
    for k in range(d.poses_cw.shape[0]):
        o = d.obs_cam == k
        win.add(np.linalg.inv(d.poses_cw[k]), d.obs_uv[o], obs_pt[o])
        res = run_window_ba(vo, win)
        if k >= cfg.ba_fixed:
            assert res is not None and res.status == "ok", (k, res and res.message)
            assert np.isfinite(res.cost_per_iter).all() and res.cost_per_iter[-1] <= res.cost_per_iter[0]
    full = [i for i, (w, kw, r) in enumerate(seen) if kw.get("marginalize")]
    assert len(full) == 4 and [seen[i][0].n_fixed for i in full] == [2, 1, 0, 0]
    gone = []  # the recorded motions a slide marginalised (by identity: each keyframe holds its own array)
    for i, (w, kw, r) in enumerate(seen):
        n = w.poses_cw.shape[0]
        assert [(f.cam_i, f.cam_j) for f in w.factors] == [(q, q + 1) for q in range(n - 1)]
        assert not any(f.meas is g for f in w.factors for g in gone), "a marginalised pair is counted again"
        if kw.get("marginalize"):
            assert r.prior is not None
            gone.append(w.factors[0].meas)
    assert len(gone) == 4 and len({id(g) for g in gone}) == 4
    # the factors are in the cost the solver reports: at the poses the front end gave, every factor's
    # residual is 0 only for the pair whose two poses BA has not moved since
    w, kw, r = seen[-1]
    st = ba_ref.BAState.from_poses(w.poses_cw, w.points)
    fs = [fr.Factor(f.cam_i, f.cam_j, f.meas, f.info) for f in w.factors]
    assert np.abs(fr.residual(st, fs[-1])).max() < 1e-12 and fr.factors_cost(st, fs) > 0
