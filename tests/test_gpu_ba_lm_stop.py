"""Termination of the BA's LM loop on the MI355X (vo_ba_set_lm_stop, vo_ba_lm_stop_info) against
the CPU restatement (tests/ba_lm_stop_ref.py).

Inputs: the rows of ``ba_lm_stop_ref.ROWS`` on the windows of ``ba_lm_ref.CASES``, twelve iterations
of the default schedule.  tests/test_ba_lm_stop_ref.py establishes on the CPU that every tested
quantity of an accepted step lies at least 10 % away from its tolerance (and tests/test_ba_lm_ref.py
that every accept / reject decision has a margin of 1e-4); the device meets 1e-8 per step, so it
stops where the restatement stops, and the damping log is the same sequence of doubles: bitwise.
"""

import numpy as np
import pytest

from oracle import ba_ref
from tests import ba_lm_ref as lr
from tests import ba_lm_stop_ref as sr
from visualodometry_amd import _lib
from visualodometry_amd._lib import VoError
from visualodometry_amd.ba import BASession, BAWindow, SlidingWindowBA

pytestmark = pytest.mark.gpu

REL = 1e-5  # the project's tolerance for a whole solve
PROBLEM_LAM = 1.0  # the sessions' fixed damping (vo_ba_run's), as the bench and the drop-in set it


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300)


def _session(name, ctx, state=None):
    win, delta, _, _, _ = lr.CASES[name]
    p, uv, _, st0 = lr.window(win)
    s = BASession(p.K, p.point_ptr, p.obs_cam, uv, p.n_poses, p.n_fixed, PROBLEM_LAM, ctx, huber=delta)
    st = state or st0
    s.set_state(st.poses_cw(), st.X)
    return s


def _options(name):
    _, _, lam0, lam_max, _ = lr.CASES[name]
    return dict(lam0=lam0, lam_max=lam_max if lam_max != lr.LAM_MAX else 0.0)


def _run(name, ctx, iters=lr.ITERS, stop=None, state=None):
    """One device LM run of a case (from its initial guess unless ``state`` is given) with the
    criteria ``stop`` = (ftol, xtol, max_rejects) or none set -> ((trials, reason), log tuple, poses,
    points)."""
    s = _session(name, ctx, state)
    if stop is not None:
        s.set_lm_stop(*stop)
    out = s.run_lm(iters, **_options(name))
    assert out[0] == _lib.VO_OK
    return s.lm_stop_info(), out[1:], *s.get_state()


def _row(row, ctx):
    name, ftol, xtol, max_rejects, _, _ = sr.ROWS[row]
    return _run(name, ctx, stop=(ftol, xtol, max_rejects))


def _assert_same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)  # (NaN equals NaN here)


@pytest.mark.parametrize("row", list(sr.ROWS))
def test_row(ctx, row):
    ref = sr.row_log(row)
    info, (costs, lambdas, trials, accepted), P, X = _row(row, ctx)
    k = ref.trials
    print(row, info, "accepted", "".join(map(str, accepted)), f"cost {_rel(costs, ref.cost):.2e}",
          f"P {_rel(P, ref.state.poses_cw()):.2e} X {_rel(X, ref.state.X):.2e}")
    assert info == (ref.trials, ref.reason)
    np.testing.assert_array_equal(accepted[:k], ref.accepted[:k])
    np.testing.assert_array_equal(lambdas, ref.lam)  # bitwise, the repeated tail included
    assert _rel(costs, ref.cost) < REL and _rel(trials[:k], ref.trial[:k]) < REL
    assert _rel(P, ref.state.poses_cw()) < REL and _rel(X, ref.state.X) < REL
    # the tail behind the stop
    assert np.isnan(trials[k:]).all() and not accepted[k:].any()
    assert (costs[k:] == costs[k]).all() and (lambdas[k:] == lambdas[k]).all()
    assert np.isfinite(costs).all() and (np.diff(costs) <= 0).all()
    for j in range(k):
        assert (trials[j] < costs[j]) == bool(accepted[j]) and costs[j + 1] == (trials[j] if accepted[j] else costs[j])


@pytest.mark.parametrize("row", ["A-ftol", "A-xtol", "C-rej3"])
def test_a_stop_changes_nothing_before_it(ctx, row):
    """The stopped run's log prefix, poses and points are bitwise an unconfigured run_lm(iters = trials)."""
    name = sr.ROWS[row][0]
    (k, reason), log, P, X = _row(row, ctx)
    assert 0 < k < lr.ITERS and reason == sr.ROWS[row][5]
    info, short, Ps, Xs = _run(name, ctx, iters=k)
    assert info == (k, sr.RAN_ALL)
    costs, lambdas, trials, accepted = log
    _assert_same_bits([costs[:k + 1], lambdas[:k + 1], trials[:k], accepted[:k], P, X], list(short) + [Ps, Xs])


def test_no_criterion_and_criteria_that_never_trip(ctx):
    plain = _run("A", ctx)
    assert plain[0] == (lr.ITERS, sr.RAN_ALL)
    zero = _run("A", ctx, stop=(0.0, 0.0, 0))
    never = _row("A-never", ctx)
    for other in (zero, never):
        assert other[0] == (lr.ITERS, sr.RAN_ALL)
        _assert_same_bits(list(other[1]) + list(other[2:]), list(plain[1]) + list(plain[2:]))
    np.testing.assert_array_equal(plain[1][3], lr.case_log("A").accepted)


def test_runs_after_an_unread_stop(ctx):
    """A stopped run_lm_async leaves a zero status word without a host read: the next run_async /
    run_lm on the session is bitwise the same call made from the stopped state on a fresh context,
    and vo_ba_run on this context stays what it is on a fresh one."""
    name, ftol, xtol, max_rejects, k, reason = sr.ROWS["A-ftol"]
    (k_dev, reason_dev), _, P, X = _row("A-ftol", ctx)
    assert (k_dev, reason_dev) == (k, reason) and k < lr.ITERS
    stopped = ba_ref.BAState.from_poses(P, X)

    s = _session(name, ctx)
    s.set_lm_stop(ftol, xtol, max_rejects)
    s.run_lm_async(lr.ITERS, **_options(name))
    s.run_async(2)
    got = s.get_state()
    fresh = _session(name, _lib.Context(0), state=stopped)
    fresh.run_async(2)
    _assert_same_bits(got, fresh.get_state())

    s = _session(name, ctx)
    s.set_lm_stop(ftol, xtol, max_rejects)
    s.run_lm_async(lr.ITERS, **_options(name))
    out = s.run_lm(3, lam0=1e-3)
    info, got = s.lm_stop_info(), s.get_state()
    fresh = _session(name, _lib.Context(0), state=stopped)
    fresh.set_lm_stop(ftol, xtol, max_rejects)
    want = fresh.run_lm(3, lam0=1e-3)
    assert out[0] == want[0] == _lib.VO_OK and info == fresh.lm_stop_info()
    _assert_same_bits(list(out[1:]) + list(got), list(want[1:]) + list(fresh.get_state()))

    res = []
    for c in (ctx, _lib.Context(0)):
        s = _session(name, c)
        rc, costs = s.run(8)
        assert rc == _lib.VO_OK
        res.append((costs, *s.get_state()))
    _assert_same_bits(*res)


def test_every_k1_variant_and_reduction_layout(ctx):
    """A with ftol 1e-2 under the four-wave K1 (-1), the one-wave K1 of 1, 2 and 6 chunks per segment,
    K2 as a launch of its own, and the banded solver's split layout switched off: the same stop and
    damping log, each bitwise against itself, states within 1e-5 of each other."""
    ref = sr.row_log("A-ftol")
    runs = {}

    def twice(tag):
        a, b = _row("A-ftol", ctx), _row("A-ftol", ctx)
        assert a[0] == b[0]
        _assert_same_bits(list(a[1]) + list(a[2:]), list(b[1]) + list(b[2:]))
        runs[tag] = a

    try:
        for v in (-1, 1, 2, 6):
            _lib.ba_testing_k1(ctx, v)
            twice(v)
    finally:
        _lib.ba_testing_k1(ctx, 0)
    try:
        _lib.ba_split_reduce(ctx, True)
        twice("split_reduce")
    finally:
        _lib.ba_split_reduce(ctx, False)
    try:
        _lib.ba_testing_no_split(ctx, True)
        twice("no_split")
    finally:
        _lib.ba_testing_no_split(ctx, False)
    for v, (info, log, P, X) in runs.items():
        assert info == (ref.trials, ref.reason), v
        np.testing.assert_array_equal(log[1], ref.lam)
        for w, (_, log2, P2, X2) in runs.items():
            assert _rel(log[0], log2[0]) < REL and _rel(P, P2) < REL and _rel(X, X2) < REL, (v, w)


BAD_STOPS = [(float("nan"), 0.0, 0), (0.0, float("nan"), 0), (float("inf"), 0.0, 0), (0.0, float("inf"), 0),
             (-1e-3, 0.0, 0), (0.0, -1e-3, 0), (0.0, 0.0, -1), (1.0, 0.0, 0), (1.5, 0.0, 0)]


def test_settings(ctx):
    name, ftol, xtol, max_rejects, k, reason = sr.ROWS["T-rej1"]
    s = _session(name, ctx)
    with pytest.raises(VoError) as e:
        s.lm_stop_info()  # no LM run on this session yet
    assert e.value.code == _lib.VO_ERR_STATE
    for bad in BAD_STOPS:
        with pytest.raises(VoError) as e:
            s.set_lm_stop(*bad)
        assert e.value.code == _lib.VO_ERR_ARG, bad
    stop = _lib.BALmStopC(0.0, 0.0, 1, 7)  # a nonzero reserved word
    assert ctx.lib.vo_ba_set_lm_stop(ctx.handle, s.session, _lib.C.byref(stop)) == _lib.VO_ERR_ARG
    # the refused settings changed nothing; iters = 0 stops nowhere
    assert s.run_lm(0)[0] == _lib.VO_OK and s.lm_stop_info() == (0, sr.RAN_ALL)
    assert s.run_lm(lr.ITERS, **_options(name))[0] == _lib.VO_OK and s.lm_stop_info() == (lr.ITERS, sr.RAN_ALL)
    # the setting holds over two runs; NULL clears it
    p, _, _, st0 = lr.window(lr.CASES[name][0])
    s.set_lm_stop(ftol, xtol, max_rejects)
    s.set_state(st0.poses_cw(), st0.X)
    assert s.run_lm(0)[0] == _lib.VO_OK and s.lm_stop_info() == (0, sr.RAN_ALL)  # with a criterion set, too
    for _ in range(2):
        s.set_state(st0.poses_cw(), st0.X)
        assert s.run_lm(lr.ITERS, **_options(name))[0] == _lib.VO_OK and s.lm_stop_info() == (k, reason)
    assert ctx.lib.vo_ba_set_lm_stop(ctx.handle, s.session, None) == _lib.VO_OK
    s.set_state(st0.poses_cw(), st0.X)
    assert s.run_lm(lr.ITERS, **_options(name))[0] == _lib.VO_OK and s.lm_stop_info() == (lr.ITERS, sr.RAN_ALL)
    # a second vo_ba_setup resets it, and makes the first session stale
    s.set_lm_stop(ftol, xtol, max_rejects)
    s2 = _session(name, ctx)
    assert s2.run_lm(lr.ITERS, **_options(name))[0] == _lib.VO_OK and s2.lm_stop_info() == (lr.ITERS, sr.RAN_ALL)
    for call in (lambda: s.set_lm_stop(ftol, xtol, max_rejects), s.lm_stop_info):
        with pytest.raises(VoError) as e:
            call()
        assert e.value.code == _lib.VO_ERR_STATE


def test_sliding_window_ba_stops(ctx):
    win, delta, _, _, _ = lr.CASES["C"]
    p, uv, _, _ = lr.window(win)
    ref = sr.row_log("C-rej3")
    obs_pt = np.repeat(np.arange(p.n_points), np.diff(p.point_ptr))
    w = BAWindow(p.poses_cw, p.points, uv, p.obs_cam, obs_pt, p.n_fixed)
    cfg = type("Cfg", (), {"ba_lm": True, "ba_lm_max_rejects": 3, "ba_iters": lr.ITERS, "ba_lambda": 1e-4,
                           "ba_huber": delta})()
    res = SlidingWindowBA(p.K, cfg).optimize(w)
    assert res.status == "ok" and res.lm_trials == 8 and res.lm_stop == "rejects"
    assert res.cost_per_iter.shape == (lr.ITERS + 1,) and np.isfinite(res.cost_per_iter).all()
    assert (np.diff(res.cost_per_iter) <= 0).all()
    assert res.cost_per_iter[-1] == res.cost_per_iter[8] and _rel(res.cost_per_iter[-1], ref.cost[8]) < REL
    all_of_them = SlidingWindowBA(p.K, type("Cfg", (), {"ba_lm": True, "ba_iters": 4, "ba_huber": delta})()).optimize(w)
    assert all_of_them.lm_trials == 4 and all_of_them.lm_stop == "ran_all"
    off = SlidingWindowBA(p.K, None, iters=2, lam=1.0, lm_max_rejects=3).optimize(w)
    assert off.lm_trials is None and off.lm_stop is None
