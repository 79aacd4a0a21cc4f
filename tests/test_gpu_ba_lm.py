"""The BA's Levenberg-Marquardt step control on the MI355X (vo_ba_run_lm) against the CPU
restatement (tests/ba_lm_ref.py).

Inputs: the cases of ``ba_lm_ref.CASES`` -- ``make_ba_problem(n, L, seed)`` with
``ba_robust_ref.with_outliers``, twelve iterations of the default schedule.  tests/test_ba_lm_ref.py
establishes on the CPU that every decision of every case has a relative margin |t - c| / c of at
least 1e-4; the device meets 1e-8 per step, so it takes the same decisions, and with equal
decisions the damping log is the same sequence of double multiplications and clamps: bitwise.
"""

import functools
import threading

import numpy as np
import pytest

from oracle import ba_ref
from tests import ba_lm_ref as lr
from tests import ba_robust_ref as rr
from visualodometry_amd import _lib
from visualodometry_amd._lib import VoError
from visualodometry_amd.ba import BASession, BAWindow, SlidingWindowBA
from visualodometry_amd.shard import shard

pytestmark = pytest.mark.gpu

REL = 1e-5  # the project's tolerance for a whole solve
PROBLEM_LAM = 1.0  # the sessions' fixed damping (vo_ba_run's), as the bench and the drop-in set it


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300)


def _session(name, ctx, state=None, huber=None):
    win, delta, _, _, _ = lr.CASES[name]
    p, uv, _, st0 = lr.window(win)
    s = BASession(p.K, p.point_ptr, p.obs_cam, uv, p.n_poses, p.n_fixed, PROBLEM_LAM, ctx,
                  huber=delta if huber is None else huber)
    st = state or st0
    s.set_state(st.poses_cw(), st.X)
    return s


def _lm(name, ctx, iters=lr.ITERS, **kw):
    """One device LM run of a case from its initial guess -> (log tuple, poses, points)."""
    _, _, lam0, lam_max, _ = lr.CASES[name]
    s = _session(name, ctx)
    out = s.run_lm(iters, lam0=lam0, lam_max=lam_max if lam_max != lr.LAM_MAX else 0.0, **kw)
    assert out[0] == _lib.VO_OK
    return out[1:], *s.get_state()


def _check_log_invariants(costs, lambdas, trials, accepted):
    assert np.isfinite(costs).all() and np.isfinite(trials).all()
    assert (np.diff(costs) <= 0).all()
    for k, a in enumerate(accepted):
        assert (trials[k] < costs[k]) == bool(a), k
        # one kernel path and one reduction order: the accepted trial's cost is the next cost, bitwise
        assert costs[k + 1] == (trials[k] if a else costs[k]), k


def _check_parity(log, P, X, ref):
    costs, lambdas, trials, accepted = log
    print("accepted", "".join(map(str, accepted)), "errors:", f"cost {_rel(costs, ref.cost):.2e}",
          f"trial {_rel(trials, ref.trial):.2e}", f"P {_rel(P, ref.state.poses_cw()):.2e} X {_rel(X, ref.state.X):.2e}")
    np.testing.assert_array_equal(accepted, ref.accepted)
    np.testing.assert_array_equal(lambdas, ref.lam)  # bitwise
    assert _rel(costs, ref.cost) < REL
    assert _rel(P, ref.state.poses_cw()) < REL
    assert _rel(X, ref.state.X) < REL
    _check_log_invariants(costs, lambdas, trials, accepted)


@pytest.mark.parametrize("name", ["A", "B", "C", "T", "T2"])
def test_parity(ctx, name):
    _check_parity(*_lm(name, ctx), lr.case_log(name))


def test_first_trial_rejected_restores_the_state(ctx):
    """B's first trial is rejected: after one iteration poses and points are set_state's, bitwise."""
    p = lr.window(lr.CASES["B"][0])[0]
    (costs, lambdas, trials, accepted), P, X = _lm("B", ctx, iters=1)
    assert list(accepted) == [0] and costs[1] == costs[0] and not trials[0] < costs[0]
    np.testing.assert_array_equal(P, p.poses_cw)
    np.testing.assert_array_equal(X, p.points)


def test_twelve_rejections_restore_the_state(ctx):
    p = lr.window(lr.CASES["Bclamp"][0])[0]
    log, P, X = _lm("Bclamp", ctx)
    ref = lr.case_log("Bclamp")
    assert not log[3].any() and log[1][-1] == 1e-2
    np.testing.assert_array_equal(log[1], ref.lam)
    assert (log[0] == log[0][0]).all()
    np.testing.assert_array_equal(P, p.poses_cw)
    np.testing.assert_array_equal(X, p.points)


def test_descends_where_the_fixed_damping_rises(ctx):
    """Case E: vo_ba_run(12) under the fixed lambda = 1 ends above its start; LM on the same window
    ends below its start and below the fixed-damping run."""
    (costs, _, _, accepted), _, _ = _lm("E", ctx)
    s = _session("E", ctx)
    rc, fixed = s.run(lr.ITERS)
    assert rc == _lib.VO_OK
    print(f"fixed lambda = 1: {fixed[0]:.4g} -> {fixed[-1]:.4g}; LM: {costs[0]:.4g} -> {costs[-1]:.4g}")
    np.testing.assert_array_equal(accepted, lr.case_log("E").accepted)
    assert fixed[-1] > fixed[0]
    assert costs[-1] < costs[0] and costs[-1] < fixed[-1]


def test_zero_iterations(ctx):
    """iters = 0: cost_out[0] is vo_ba_run(0)'s cost bitwise -- both are the cost-only K1's segment
    partials summed in K2's cost order (ba_lm_decide restates that partition and tree) -- and the
    state is untouched."""
    p = lr.window(lr.CASES["A"][0])[0]
    s = _session("A", ctx)
    rc, costs, lambdas, trials, accepted = s.run_lm(0, lam0=0.5)
    assert rc == _lib.VO_OK and costs.shape == (1,) and trials.shape == (0,) and lambdas[0] == 0.5
    P, X = s.get_state()
    np.testing.assert_array_equal(P, p.poses_cw)
    np.testing.assert_array_equal(X, p.points)
    rc, c0 = _session("A", ctx).run(0)
    assert rc == _lib.VO_OK and costs[0] == c0[0]


def test_every_k1_variant(ctx):
    """A under the four-wave K1 (-1) and the one-wave K1 of 1, 2 and 6 chunks per segment: the same
    decisions and damping log, states within 1e-5 of each other, each bitwise against itself."""
    ref = lr.case_log("A")
    runs = {}
    try:
        for v in (-1, 1, 2, 6):
            _lib.ba_testing_k1(ctx, v)
            a, b = _lm("A", ctx), _lm("A", ctx)
            for x, y in zip(a[0] + a[1:], b[0] + b[1:]):
                np.testing.assert_array_equal(x, y)
            runs[v] = a
    finally:
        _lib.ba_testing_k1(ctx, 0)
    for v, (log, P, X) in runs.items():
        _check_parity(log, P, X, ref)
        for w, (log2, P2, X2) in runs.items():
            assert _rel(log[0], log2[0]) < REL and _rel(P, P2) < REL and _rel(X, X2) < REL, (v, w)


def test_reduction_launched_on_its_own_and_no_split_layout(ctx):
    """A with K2 as a launch of its own (its LM kernel restates the fused reducers' sums: the
    same bits), and with the banded solver's split layout switched off."""
    ref = lr.case_log("A")
    fused = _lm("A", ctx)
    try:
        _lib.ba_split_reduce(ctx, True)
        split = _lm("A", ctx)
    finally:
        _lib.ba_split_reduce(ctx, False)
    _check_parity(*split, ref)
    for x, y in zip(fused[0] + fused[1:], split[0] + split[1:]):
        np.testing.assert_array_equal(x, y)
    try:
        _lib.ba_testing_no_split(ctx, True)
        _check_parity(*_lm("A", ctx), ref)
    finally:
        _lib.ba_testing_no_split(ctx, False)


def test_after_a_pending_gn_step(ctx):
    """run_async(3) leaves a pose step whose landmark update is pending; run_lm applies it first
    (under the problem's lambda): bitwise the run that starts from the synchronised state."""
    s = _session("A", ctx)
    s.run_async(3)
    out1 = s.run_lm(6, lam0=1.0)
    st1 = s.get_state()
    s = _session("A", ctx)
    assert s.run(3)[0] == _lib.VO_OK
    P, X = s.get_state()
    s = _session("A", ctx, state=ba_ref.BAState.from_poses(P, X))
    out2 = s.run_lm(6, lam0=1.0)
    st2 = s.get_state()
    assert out1[0] == out2[0] == _lib.VO_OK
    for x, y in zip(out1[1:] + st1, out2[1:] + st2):
        np.testing.assert_array_equal(x, y)
    _check_log_invariants(*out1[1:])


def test_gn_and_residuals_after_lm(ctx):
    """run_lm(6), run(2), residuals(): nothing is pending after LM, and the GN kernels go on from
    its state as from any other."""
    win, delta, lam0, _, _ = lr.CASES["A"]
    _, _, struct, _ = lr.window(win)
    ref = lr.case_log("A", 6)
    ref2, (ref_costs,) = rr.solve_schedule(ref.state, struct, [(2, delta)], PROBLEM_LAM)
    s = _session("A", ctx)
    rc, costs, lambdas, trials, accepted = s.run_lm(6, lam0=lam0)
    assert rc == _lib.VO_OK
    np.testing.assert_array_equal(accepted, ref.accepted)
    rc, c2 = s.run(2)
    assert rc == _lib.VO_OK and _rel(c2, ref_costs) < REL
    err2, depth = s.residuals()
    r, pc = ba_ref.residuals(ref2, struct)
    assert _rel(err2, (r * r).sum(-1)) < REL and _rel(depth, pc[:, 2]) < REL
    P, X = s.get_state()
    assert _rel(P, ref2.poses_cw()) < REL and _rel(X, ref2.X) < REL


def test_set_robust_between_two_lm_runs(ctx):
    ra, rb = lr.robust_switch_logs()
    s = _session("E", ctx)
    rc, costs, lambdas, _, accepted = s.run_lm(3, lam0=1e-4)
    assert rc == _lib.VO_OK
    np.testing.assert_array_equal(accepted, ra.accepted)
    s.set_robust(2.0)
    rc, costs, lambdas, trials, accepted = s.run_lm(3, lam0=1e-4)
    assert rc == _lib.VO_OK
    _check_parity((costs, lambdas, trials, accepted), *s.get_state(), rb)


def test_async_and_log(ctx):
    sync, P, X = _lm("A", ctx)
    s = _session("A", ctx)
    s.run_lm_async(lr.ITERS, lam0=lr.CASES["A"][2])
    rc, *log = s.lm_log(lr.ITERS)
    assert rc == _lib.VO_OK
    for x, y in zip(log + list(s.get_state()), list(sync) + [P, X]):
        np.testing.assert_array_equal(x, y)
    rc, c5, l5, t5, a5 = s.lm_log(5)  # a prefix, and readable more than once
    assert rc == _lib.VO_OK
    np.testing.assert_array_equal(c5, sync[0][:6])
    np.testing.assert_array_equal(a5, sync[3][:5])
    with pytest.raises(VoError) as e:
        s.lm_log(lr.ITERS + 1)
    assert e.value.code == _lib.VO_ERR_ARG


def test_gn_is_untouched_by_an_earlier_lm_run(ctx):
    """vo_ba_run(8) on a context that has run LM (this one, by now) is bitwise the run on a fresh one."""
    _lm("A", ctx, iters=3)
    res = []
    for c in (ctx, _lib.Context(0)):
        s = _session("A", c)
        rc, costs = s.run(8)
        assert rc == _lib.VO_OK
        res.append((costs, *s.get_state()))
    for x, y in zip(*res):
        np.testing.assert_array_equal(x, y)


BAD_OPTIONS = [dict(lam0=float("nan")), dict(up=float("inf")), dict(lam_min=float("nan")), dict(lam0=-1.0),
               dict(up=1.0), dict(up=0.5), dict(up=-10.0), dict(down=1.0), dict(down=1.5), dict(down=-0.1),
               dict(lam_min=-1e-6), dict(lam_min=1.0, lam_max=0.5), dict(lam_max=1e-9)]


def test_bad_options_and_stale_session(ctx):
    s = _session("T", ctx)
    for bad in BAD_OPTIONS:
        with pytest.raises(VoError) as e:
            s.run_lm(2, **bad)
        assert e.value.code == _lib.VO_ERR_ARG, bad
        with pytest.raises(VoError) as e:
            s.run_lm_async(2, **bad)
        assert e.value.code == _lib.VO_ERR_ARG, bad
    with pytest.raises(VoError) as e:
        s.run_lm(-1)
    assert e.value.code == _lib.VO_ERR_ARG
    with pytest.raises(VoError) as e:
        s.lm_log(0)  # no LM run on this session yet
    assert e.value.code == _lib.VO_ERR_STATE
    rc, costs, lambdas, _, _ = s.run_lm(2, lam0=1e9)  # still usable; lambda0 clamped into the range
    assert rc == _lib.VO_OK and lambdas[0] == 1e6
    assert s.run_lm(1)[2][0] == PROBLEM_LAM  # lambda0 = 0: the problem's damping
    _session("T", ctx)  # another vo_ba_setup on the context replaces the problem
    for call in (lambda: s.run_lm(2), lambda: s.run_lm_async(2), lambda: s.lm_log(1)):
        with pytest.raises(VoError) as e:
            call()
        assert e.value.code == _lib.VO_ERR_STATE


def test_two_ranks_are_refused():
    """Sharded LM is not built: with a two-rank (loopback) communicator every rank gets VO_ERR_STATE."""
    p, uv, _, _ = lr.window(lr.CASES["C"][0])
    nranks, codes, errors = 2, [None, None], []

    def worker(r):
        try:
            c = _lib.Context(0)
            _lib.comm_init_loopback(c, nranks, r, b"vo-loopback-lm")
            _, ptr, cam, suv, pts = shard(p.point_ptr, p.obs_cam, uv, p.points, nranks, r)
            s = BASession(p.K, ptr, cam, suv, p.n_poses, p.n_fixed, PROBLEM_LAM, c)
            s.set_state(p.poses_cw, pts)
            try:
                s.run_lm(2)
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


def test_sliding_window_ba_with_lm(ctx):
    win, delta, _, _, _ = lr.CASES["C"]
    p, uv, _, _ = lr.window(win)
    obs_pt = np.repeat(np.arange(p.n_points), np.diff(p.point_ptr))
    w = BAWindow(p.poses_cw, p.points, uv, p.obs_cam, obs_pt, p.n_fixed)
    cfg = type("Cfg", (), {"ba_lm": True, "ba_iters": 8, "ba_lambda": 1e-4, "ba_huber": delta})()
    res = SlidingWindowBA(p.K, cfg).optimize(w)
    assert res.status == "ok" and res.cost_per_iter.shape == (9,)
    assert (np.diff(res.cost_per_iter) <= 0).all() and res.cost_per_iter[-1] < res.cost_per_iter[0]
    assert res.lambdas.shape == (9,) and res.lambdas[0] == 1e-4 and res.accepted.shape == (8,)
    np.testing.assert_array_equal(res.accepted, lr.case_log("C").accepted[:8])
    off = SlidingWindowBA(p.K, None, iters=2, lam=1.0).optimize(w)
    assert off.lambdas is None and off.accepted is None
