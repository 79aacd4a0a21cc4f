"""Per-observation weights and device-side culling on the MI355X (``vo_ba_set_obs_weights``,
``vo_ba_cull``), against the CPU restatement (tests/ba_weight_ref.py).

Inputs: ``make_ba_problem(8, 300, 21)`` (SMALL) and ``make_ba_problem(16, 400, 5, max_track=4)``
(NARROW): the smallest windows here that cross chunks and segments and have observations in the
fixed cameras.  lambda = 1, Huber delta = 2 px where a test uses one.  Weights: uniform in
[0.25, 4] with about a tenth of them zero (``_weights``).

Bounds.  A step (S, b, dc, cost against the restatement, or two GPU sessions whose plans differ)
is held to the project's per-step bound, 1e-8 of the largest entry (``_rel``, as
tests/test_gpu_ba_robust.py scales it); a whole solve to 1e-5.  Where two runs launch the same
kernels on the same plan the comparison is bit for bit.
"""

import functools

import numpy as np
import pytest

from oracle import ba_ref
from tests import ba_cov_ref as cr
from tests import ba_robust_ref as rr
from tests import ba_weight_ref as wr
from tests.ba_weight_ref import CULL_MARGIN, SCHEDULE
from visualodometry_amd import _lib
from visualodometry_amd._lib import VoError
from visualodometry_amd.ba import BASession, BAWindow, SlidingWindowBA
from visualodometry_amd.synthetic import make_ba_problem

pytestmark = pytest.mark.gpu

LAM, DELTA = 1.0, 2.0
STEP, SOLVE = 1e-8, 1e-5
SMALL, NARROW = (8, 300, 21, ()), (16, 400, 5, (("max_track", 4),))
CASES = [SMALL, NARROW]


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300)


@functools.lru_cache(maxsize=None)
def _case(case, outliers=False):
    n, L, seed, kw = case
    p = make_ba_problem(n, L, seed, **dict(kw))
    uv = rr.with_outliers(p, seed) if outliers else p.obs_uv
    return p, uv, rr.structure(p, uv), ba_ref.BAState.from_poses(p.poses_cw, p.points)


@functools.lru_cache(maxsize=None)
def _weights(case):
    """Uniform in [0.25, 4], about 10 % zeros (never modified: callers copy before they write)."""
    M = _case(case)[2].obs_cam.size
    rng = np.random.default_rng(1000 + case[2])
    w = rng.uniform(0.25, 4.0, M)
    w[rng.random(M) < 0.1] = 0.0
    w.setflags(write=False)
    return w


def _session(case, ctx, huber=0.0, state=None, outliers=False, structure=None):
    p, uv, s, st0 = _case(case, outliers)
    s = structure or s
    sess = BASession(p.K, s.point_ptr, s.obs_cam, s.obs_uv, p.n_poses, p.n_fixed, LAM, ctx, huber=huber)
    st = state or st0
    sess.set_state(st.poses_cw(), st.X)
    return sess


def _step_figures(got, ref_S, ref_b, ref_dc, ref_cost):
    rc, S, b, dc, cost = got
    assert rc == _lib.VO_OK
    assert np.isfinite(S).all() and np.isfinite(b).all() and np.isfinite(dc).all() and np.isfinite(cost)
    return dict(S=_rel(S, ref_S), b=_rel(b, ref_b), dc=_rel(dc, ref_dc), cost=abs(cost - ref_cost) / abs(ref_cost))


def _assert_step(figs, what):
    print(f"{what}: step errors", {k: f"{v:.2e}" for k, v in figs.items()})
    for k, v in figs.items():
        assert v < STEP, (what, k, v)


# 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [0.0, DELTA])
@pytest.mark.parametrize("case", CASES)
def test_gn_step_parity(ctx, case, delta):
    _, _, struct, st0 = _case(case)
    w = _weights(case)
    assert 0.05 < (w == 0).mean() < 0.15
    s = _session(case, ctx, huber=delta)
    s.set_obs_weights(w)
    ref = wr.gn_step(st0, struct, LAM, w, delta)
    figs = _step_figures(s.gn_step(), ref.system.S, ref.system.b, ref.dc, ref.system.cost)
    P, X = s.get_state()
    figs.update(P=_rel(P, ref.state.poses_cw()), X=_rel(X, ref.state.X))
    _assert_step(figs, f"{case[:3]} delta {delta}")


# 2 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [0.0, DELTA])
@pytest.mark.parametrize("case", CASES)
def test_solve_parity(ctx, case, delta):
    _, _, struct, st0 = _case(case)
    w = _weights(case)
    s = _session(case, ctx, huber=delta)
    s.set_obs_weights(w)
    rc, costs = s.run(5)
    assert rc == _lib.VO_OK
    P, X = s.get_state()
    ref, ref_costs = wr.solve(st0, struct, 5, LAM, w, delta)
    figs = (_rel(costs, ref_costs), _rel(P, ref.poses_cw()), _rel(X, ref.X))
    print("run(5) errors:", " ".join(f"{v:.2e}" for v in figs))
    assert max(figs) < SOLVE
    chained, launches = _lib.ba_testing_last_run(ctx)
    assert not chained and launches == 10, "a session with weights: a K1 launch and a solve launch per iteration"

    s = _session(case, ctx, huber=delta)
    s.set_obs_weights(w)
    rc, c, lam, trial, acc = s.run_lm(5, lam0=LAM)
    assert rc == _lib.VO_OK
    P, X = s.get_state()
    log = wr.solve_lm(st0, struct, 5, w, delta, LAM)
    print("run_lm(5):", log.pattern(), "margins", " ".join(f"{m:.1e}" for m in log.margins()))
    assert log.margins().min() > 1e-4, "a decision of the restatement too close to call: unfit input"
    np.testing.assert_array_equal(acc, log.accepted)
    np.testing.assert_array_equal(lam, log.lam)  # equal decisions: the same two multiplications and clamps
    figs = (_rel(c, log.cost), _rel(trial, log.trial), _rel(P, log.state.poses_cw()), _rel(X, log.state.X))
    print("run_lm(5) errors:", " ".join(f"{v:.2e}" for v in figs))
    assert max(figs) < SOLVE


# 3 ------------------------------------------------------------------------------------------------
def _zero_depth_state(case):
    """Camera 0 (fixed) at the origin and a landmark it sees moved there: R 0 + 0 is an exact zero
    in any arithmetic, so that observation's depth is 0 and its raw residual 0 * inf = NaN.  The
    landmark is behind its later cameras (finite residuals)."""
    p, _, struct, st0 = _case(case)
    q = next(q for q in range(p.n_points) if p.obs_cam[p.point_ptr[q]] == 0 and p.point_ptr[q + 1] - p.point_ptr[q] >= 3)
    st = st0.copy()
    st.t[0] = 0.0
    st.X[q] = 0.0
    return st, int(p.point_ptr[q])


@pytest.mark.parametrize("delta", [0.0, DELTA])
def test_zero_weight_is_a_select(ctx, delta):
    p, uv, struct, _ = _case(SMALL)
    st, o = _zero_depth_state(SMALL)
    err2, z = wr.raw_err2_depth(st, struct)
    assert not np.isfinite(err2[o]) and z[o] == 0.0 and np.isfinite(np.delete(err2, o)).all()
    w = np.ones(struct.obs_cam.size)
    w[o] = 0.0
    # the same window without that observation: another plan, the per-step bound
    dropped, _ = wr.repeated_structure(p, w.astype(np.int64), uv)
    t = _session(SMALL, ctx, huber=delta, state=st, structure=dropped)
    rc, S, b, dc, cost = t.gn_step()
    assert rc == _lib.VO_OK
    P2, X2 = t.get_state()
    s = _session(SMALL, ctx, huber=delta, state=st)
    e2, zz = s.residuals()
    assert not np.isfinite(e2[o]) and zz[o] == 0.0  # the device sees the same non-finite value
    s.set_obs_weights(w)
    got = s.gn_step()
    P, X = s.get_state()
    assert np.isfinite(P).all() and np.isfinite(X).all()
    figs = _step_figures(got, S, b, dc, cost)
    figs.update(P=_rel(P, P2), X=_rel(X, X2))
    _assert_step(figs, f"zero weight vs dropped, delta {delta}")
    ref = wr.gn_step(st, struct, LAM, w, delta)
    _assert_step(_step_figures(got, ref.system.S, ref.system.b, ref.dc, ref.system.cost), "zero weight vs restatement")
    # a whole solve and the cost-only kernel stay finite too
    rc, costs = s.run(3)
    assert rc == _lib.VO_OK and np.isfinite(costs).all()


# 4 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_integer_weights_are_repeated_observations(ctx, case):
    """w in {0, 1, 2, 3} against an unweighted session on the window with observation o repeated
    w_o times.  Every landmark keeps its first observation (an empty track is not a window the
    planner is asked to take here)."""
    p, uv, struct, st0 = _case(case)
    w = np.random.default_rng(11 + case[2]).integers(0, 4, struct.obs_cam.size)
    w[p.point_ptr[:-1]] = np.maximum(w[p.point_ptr[:-1]], 1)
    assert set(np.unique(w)) == {0, 1, 2, 3}
    rep, _ = wr.repeated_structure(p, w, uv)
    t = _session(case, ctx, structure=rep)
    rc, S, b, dc, cost = t.gn_step()
    assert rc == _lib.VO_OK
    s = _session(case, ctx)
    s.set_obs_weights(w.astype(np.float64))
    _assert_step(_step_figures(s.gn_step(), S, b, dc, cost), f"{case[:3]} integer weights vs repeats")


# 5 ------------------------------------------------------------------------------------------------
def test_clearing_setup_and_bad_arguments(ctx):
    _, _, struct, st0 = _case(SMALL)
    w = _weights(SMALL)
    M = w.size

    def plain():
        s = _session(SMALL, ctx)
        rc, costs = s.run(4)
        assert rc == _lib.VO_OK
        return (costs,) + s.get_state()

    base = plain()
    s = _session(SMALL, ctx)
    np.testing.assert_array_equal(s.obs_weights(), np.ones(M))  # a new setup starts at all ones
    s.set_obs_weights(w)
    np.testing.assert_array_equal(s.obs_weights(), w)
    s.set_obs_weights(None)
    np.testing.assert_array_equal(s.obs_weights(), np.ones(M))
    rc, costs = s.run(4)
    assert rc == _lib.VO_OK
    for x, y in zip((costs,) + s.get_state(), base):  # the same kernels: bit for bit
        np.testing.assert_array_equal(x, y)
    # a cull that culls nothing leaves a session without weights without them
    s = _session(SMALL, ctx)
    assert s.cull(max_chi2=0.0, min_depth=-1e30, min_track=0) == (0, M)
    rc, costs = s.run(4)
    for x, y in zip((costs,) + s.get_state(), base):
        np.testing.assert_array_equal(x, y)
    # bad weights: VO_ERR_ARG, and the old weights stay in force
    s = _session(SMALL, ctx)
    s.set_obs_weights(w)
    for bad in (-1.0, float("nan"), float("inf")):
        wb = np.array(w)
        wb[M // 2] = bad
        with pytest.raises(VoError) as e:
            s.set_obs_weights(wb)
        assert e.value.code == _lib.VO_ERR_ARG
    np.testing.assert_array_equal(s.obs_weights(), w)
    ref = wr.gn_step(st0, struct, LAM, w)
    _assert_step(_step_figures(s.gn_step(), ref.system.S, ref.system.b, ref.dc, ref.system.cost), "after bad weights")
    # bad cull options
    for kw in (dict(max_chi2=-1.0), dict(max_chi2=float("nan")), dict(min_depth=float("inf"))):
        with pytest.raises(VoError) as e:
            s.cull(**kw)
        assert e.value.code == _lib.VO_ERR_ARG
    opt = _lib.BACullOptionsC(0.0, 0.0, 2, 1)  # reserved != 0
    assert ctx.lib.vo_ba_cull_async(ctx.handle, s.session, _lib.C.byref(opt)) == _lib.VO_ERR_ARG
    # a new setup on the context starts at all ones and makes the old session stale
    t = _session(SMALL, ctx)
    np.testing.assert_array_equal(t.obs_weights(), np.ones(M))
    for call in (lambda: s.set_obs_weights(w), s.obs_weights, s.cull, s.cull_async):
        with pytest.raises(VoError) as e:
            call()
        assert e.value.code == _lib.VO_ERR_STATE
    # no state set
    u = BASession(struct.K, struct.point_ptr, struct.obs_cam, struct.obs_uv, struct.n_poses, struct.n_fixed, LAM, ctx)
    with pytest.raises(VoError) as e:
        u.cull()
    assert e.value.code == _lib.VO_ERR_STATE


def test_pending_step_lands_under_the_weights_it_was_solved_with(ctx):
    """gn_step under weights w leaves the landmark update pending; new weights must not change it."""
    _, _, struct, st0 = _case(SMALL)
    w = _weights(SMALL)
    ref = wr.gn_step(st0, struct, LAM, w)
    s = _session(SMALL, ctx)
    s.set_obs_weights(w)
    assert s.gn_step()[0] == _lib.VO_OK
    s.set_obs_weights(None)
    P, X = s.get_state()
    assert _rel(P, ref.state.poses_cw()) < STEP and _rel(X, ref.state.X) < STEP


def test_layouts_covered_and_refused(ctx):
    """Every one-wave K1 layout has a weighted form (1, 2, 3 and 6 chunks per segment agree to the
    per-step bound: only the summation order differs); the four-wave K1 of the testing switch has
    none, and refuses the run instead of dropping the weights."""
    _, _, struct, st0 = _case(SMALL)
    w = _weights(SMALL)
    ref = wr.gn_step(st0, struct, LAM, w, DELTA)
    try:
        for v in (1, 2, 3, 6):
            _lib.ba_testing_k1(ctx, v)
            s = _session(SMALL, ctx, huber=DELTA)
            s.set_obs_weights(w)
            _assert_step(_step_figures(s.gn_step(), ref.system.S, ref.system.b, ref.dc, ref.system.cost), f"K1 variant {v}")
        _lib.ba_testing_k1(ctx, -1)
        s = _session(SMALL, ctx)
        rc, costs = s.run(1)  # without weights the four-wave K1 runs as ever
        assert rc == _lib.VO_OK
        s = _session(SMALL, ctx)
        s.set_obs_weights(w)
        for call in (s.gn_step, lambda: s.run(2), lambda: s.run_lm(2), lambda: s.covariance(1.0)):
            with pytest.raises(VoError) as e:
                call()
            assert e.value.code == _lib.VO_ERR_STATE
    finally:
        _lib.ba_testing_k1(ctx, 0)


# 6 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_cull_rule_exactly(ctx, case):
    p, uv, struct, _ = _case(case, outliers=True)
    w = _weights(case)
    s = _session(case, ctx, huber=DELTA, outliers=True)
    s.set_obs_weights(w)
    s.run_async(3)  # leaves a pending landmark update: the cull applies it first
    err2, z = s.residuals()
    P0, X0 = s.get_state()
    # options that make every rule bite: chi2 at the median of the active w err2, a depth bound
    # that takes a few percent, the track rule
    chi2 = float(np.median((w * err2)[w > 0]))
    depth = float(np.quantile(z, 0.03))
    want = wr.cull_weights(err2, z, w, struct.point_ptr, chi2, depth, 2)
    by_rule = wr.cull_weights(err2, z, w, struct.point_ptr, chi2, depth, 0)
    assert ((by_rule == 0) & (w > 0)).sum() > 100 and ((want == 0) & (by_rule > 0)).sum() > 0, "every rule must bite"
    n_culled, n_active = s.cull(chi2, depth, 2)
    got = s.obs_weights()
    np.testing.assert_array_equal(got == 0, want == 0)
    np.testing.assert_array_equal(got, want)  # survivors keep their weight
    assert n_culled == int(((want == 0) & (w > 0)).sum()) and n_active == int((want > 0).sum())
    P1, X1 = s.get_state()
    np.testing.assert_array_equal(P1, P0)
    np.testing.assert_array_equal(X1, X0)
    assert s.cull(chi2, depth, 2) == (0, n_active)  # the same state, the same options: nothing more
    np.testing.assert_array_equal(s.obs_weights(), want)
    # the solve goes on under the culled weights
    st = ba_ref.BAState.from_poses(P1, X1)
    ref = wr.gn_step(st, struct, LAM, want, DELTA)
    _assert_step(_step_figures(s.gn_step(), ref.system.S, ref.system.b, ref.dc, ref.system.cost), "after the cull")


def test_cull_of_non_finite_and_unweighted(ctx):
    """A session that never had weights: the cull starts from all ones; the zero-depth observation
    (NaN residual) goes by the finiteness rule even with every other rule off."""
    _, _, struct, _ = _case(SMALL)
    st, o = _zero_depth_state(SMALL)
    s = _session(SMALL, ctx, state=st)
    M = struct.obs_cam.size
    assert s.cull(max_chi2=0.0, min_depth=-1e30, min_track=0) == (1, M - 1)
    w = s.obs_weights()
    assert w[o] == 0 and (np.delete(w, o) == 1).all()
    rc, S, b, dc, cost = s.gn_step()
    assert rc == _lib.VO_OK and np.isfinite(S).all() and np.isfinite(dc).all() and np.isfinite(cost)


# 7 ------------------------------------------------------------------------------------------------
def test_schedule_without_a_host_round_trip(ctx):
    chi2 = SCHEDULE["max_chi2"]

    def run(asynchronous):
        s = _session(SMALL, ctx, huber=DELTA, outliers=True)
        if asynchronous:
            s.run_lm_async(4, lam0=LAM)
            s.cull_async(chi2, 0.0, 2)
            s.run_lm_async(4, lam0=LAM)
            rc, c, lam, trial, acc = s.lm_log(4)
        else:
            assert s.run_lm(4, lam0=LAM)[0] == _lib.VO_OK
            n_culled, _ = s.cull(chi2, 0.0, 2)
            assert n_culled > 0
            rc, c, lam, trial, acc = s.run_lm(4, lam0=LAM)
        assert rc == _lib.VO_OK
        return (c, lam, trial, acc, s.obs_weights()) + s.get_state()

    a, b = run(True), run(False)
    assert (a[4] == 0).sum() > 0
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


# 8 ------------------------------------------------------------------------------------------------
def test_outlier_schedule(ctx):
    """Optimise, cull by chi^2, optimise again (tests/ba_weight_ref.py SCHEDULE, whose margins
    tests/test_ba_weight_ref.py re-establishes on the CPU): the GPU's final active set is the restatement's, apart
    from observations within CULL_MARGIN of the bound at a cull (at most 0.1 % of them; none here),
    and the final translation error is no worse than the restatement's Huber-only run of the same
    length."""
    assert SCHEDULE["win"] == SMALL[:3]
    delta, chi2, R, iters = (SCHEDULE[k] for k in ("delta", "max_chi2", "rounds", "iters"))
    p, uv, struct, st0 = _case(SMALL, outliers=True)
    ref, w_ref, ref_parts, margin, near = wr.cull_schedule(st0, struct, R, iters, LAM, delta, chi2, near_rel=CULL_MARGIN)
    assert near.sum() <= 1e-3 * near.size
    s = _session(SMALL, ctx, huber=delta, outliers=True)
    parts = []
    for k in range(R + 1):
        rc, costs = s.run(iters)
        assert rc == _lib.VO_OK
        parts.append(costs)
        if k < R:
            s.cull(chi2, 0.0, 2)
    w = s.obs_weights()
    differ = ((w == 0) != (w_ref == 0)) & ~near
    assert not differ.any(), f"{int(differ.sum())} observations differ from the restatement's active set"
    P, X = s.get_state()
    huber, _ = rr.solve(st0, struct, (R + 1) * iters, LAM, delta)
    e_gpu, e_ref = rr.max_translation_error(P, p), rr.max_translation_error(ref.poses_cw(), p)
    e_huber = rr.max_translation_error(huber.poses_cw(), p)
    print(f"outlier schedule: {int((w == 0).sum())} of {w.size} culled; translation error GPU {e_gpu:.4f} m, "
          f"restatement {e_ref:.4f} m, Huber alone {e_huber:.4f} m")
    assert e_gpu <= e_huber
    if not near.any():  # the same active sets throughout: the solve itself agrees
        assert _rel(np.concatenate(parts), np.concatenate(ref_parts)) < SOLVE
        assert _rel(P, ref.poses_cw()) < SOLVE and _rel(X, ref.X) < SOLVE


def test_sliding_window_cull_rounds(ctx):
    """``SlidingWindowBA(cull_rounds=2)`` on a window whose observations are shuffled: obs_active and
    the weights are in the window's own order, cost_per_iter concatenates the parts."""
    delta, chi2, R, iters = (SCHEDULE[k] for k in ("delta", "max_chi2", "rounds", "iters"))
    p, uv, struct, st0 = _case(SMALL, outliers=True)
    w0 = np.ones(struct.obs_cam.size)
    w0[::17] = 0.0
    w0[1::17] = 2.0
    ref, w_ref, ref_parts, _, near = wr.cull_schedule(st0, struct, R, iters, LAM, delta, chi2, w=w0)
    assert not near.any()
    perm = np.random.default_rng(7).permutation(struct.obs_cam.size)
    win = BAWindow(p.poses_cw, p.points, uv[perm], p.obs_cam[perm], struct.obs_pt[perm], p.n_fixed, obs_weight=w0[perm])
    ba = SlidingWindowBA(p.K, None, iters=iters, lam=LAM, huber=delta, cull_rounds=R, cull_chi2=chi2)
    res = ba.optimize(win)
    assert res.status == "ok" and res.obs_active.dtype == bool
    np.testing.assert_array_equal(res.obs_active, (w_ref > 0)[perm])
    assert res.cost_per_iter.shape == ((R + 1) * (iters + 1),)
    assert _rel(res.cost_per_iter, np.concatenate(ref_parts)) < SOLVE
    assert _rel(res.poses_cw, ref.poses_cw()) < SOLVE
    assert SlidingWindowBA(p.K, None, iters=2, lam=LAM).optimize(win).obs_active is None


# 9 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [0.0, DELTA])
@pytest.mark.parametrize("case", CASES)
def test_covariance_honours_the_weights(ctx, case, delta):
    """Against the dense inverse of J^T W J + lambda I over the whitened Jacobians
    (``ba_weight_ref.cov_dense``), tests/ba_cov_ref.py's metric and bound: max(1e-8, 100 eps_ref),
    eps_ref the disagreement of that route with the Schur route on the same input, required to be
    <= 1e-9.  lambda = 1: with zero weights a landmark may keep a single observation, which only
    damping holds."""
    _, _, struct, st0 = _case(case)
    w = _weights(case)
    lam = 1.0
    cc, pp = wr.cov_dense(st0, struct, lam, w, delta)
    cc_a, pp_a = wr.cov_schur(st0, struct, lam, w, delta)
    assert not np.isnan(pp_a).any()
    eps = max(cr.rel_err(cc_a, cc), cr.rel_err(pp_a, pp))
    assert eps <= 1e-9, f"eps_ref {eps:.3g} makes this input unusable"
    tol = max(1e-8, 100.0 * eps)
    s = _session(case, ctx, huber=delta)
    s.set_obs_weights(w)
    pose, pts, dense = s.covariance(lam, dense=True)
    e_pose, e_pts = cr.rel_err(dense, cc), cr.rel_err(pts, pp)
    print(f"{case[:3]} delta {delta}: eps_ref {eps:.3g} tol {tol:.3g} pose err {e_pose:.3g} landmark err {e_pts:.3g}")
    assert e_pose <= tol and e_pts <= tol
    # the weights matter: the unweighted covariance is far from this one
    s.set_obs_weights(None)
    _, _, dense1 = s.covariance(lam, dense=True)
    assert cr.rel_err(dense1, cc) > 1e-3
