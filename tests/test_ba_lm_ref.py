"""The CPU restatement of the BA's Levenberg-Marquardt loop (tests/ba_lm_ref.py) on the windows the
device tests use: the accept / reject pattern of every case, a non-increasing cost, a damping log
that obeys the schedule and its clamps -- and the fitness condition the device parity tests
depend on: every decision's relative margin |t - c| / c is at least 1e-4, so a device that meets
the project's 1e-8 per-step parity cannot flip one.  That is a condition on the inputs: a case
that stops meeting it is replaced, not loosened.
"""

import numpy as np
import pytest

from tests import ba_lm_ref as lr
from tests import ba_robust_ref as rr


@pytest.mark.parametrize("name", list(lr.CASES))
def test_case(name):
    win, delta, lam0, lam_max, pattern = lr.CASES[name]
    log = lr.case_log(name)  # a LinAlgError in the reference step would surface here: an unfit case
    print(name, log.pattern(), f"smallest margin {log.margins().min():.2e}", f"final lambda {log.lam[-1]:.3g}",
          f"cost {log.cost[0]:.6g} -> {log.cost[-1]:.6g}")
    assert log.pattern() == pattern
    assert np.isfinite(log.cost).all() and np.isfinite(log.trial).all()
    assert (np.diff(log.cost) <= 0).all()
    assert log.margins().min() >= lr.MARGIN
    # the schedule and its clamps, in the restatement's own arithmetic
    assert log.lam[0] == min(max(lam0, lr.LAM_MIN), lam_max)
    for k, a in enumerate(log.accepted):
        assert (log.trial[k] < log.cost[k]) == bool(a)
        assert log.cost[k + 1] == (log.trial[k] if a else log.cost[k])
        want = max(log.lam[k] * lr.DOWN, lr.LAM_MIN) if a else min(log.lam[k] * lr.UP, lam_max)
        assert log.lam[k + 1] == want
    assert lr.LAM_MIN <= log.lam.min() and log.lam.max() <= lam_max


def test_where_the_damping_ends():
    assert lr.case_log("A").lam[-1] == lr.LAM_MIN  # at the floor
    assert lr.case_log("E").lam[-1] == pytest.approx(1e-6, rel=1e-12)  # reached by six divisions, not clamped
    assert lr.case_log("C").lam[-1] == pytest.approx(10.0, rel=1e-12)
    assert lr.case_log("B").lam[-1] == pytest.approx(1.0, rel=1e-12)
    assert lr.case_log("Bclamp").lam[-1] == 1e-2  # pinned at lambda_max
    assert lr.window(lr.CASES["T"][0])[0].n_poses - lr.window(lr.CASES["T"][0])[0].n_fixed == 1  # one free pose


def test_fixed_damping_rises_where_lm_descends():
    """Case E's window under the default fixed damping (lambda = 1, every step accepted) ends worse
    than it began; the LM loop on the same window ends below its start."""
    win, delta, *_ = lr.CASES["E"]
    _, _, s, st0 = lr.window(win)
    _, costs = rr.solve(st0, s, lr.ITERS, 1.0, delta)
    log = lr.case_log("E")
    print(f"fixed lambda = 1: {costs[0]:.4g} -> {costs[-1]:.4g}; LM: {log.cost[0]:.4g} -> {log.cost[-1]:.4g}")
    assert costs[-1] > costs[0]
    assert log.cost[-1] < log.cost[0] and log.cost[-1] < costs[-1]


def test_robust_switch_sequence_is_fit():
    """The two-run sequence of the device test that switches the cost between LM runs: same margin."""
    a, b = lr.robust_switch_logs()
    print(a.pattern(), b.pattern(), f"{a.margins().min():.2e} {b.margins().min():.2e}")
    assert min(a.margins().min(), b.margins().min()) >= lr.MARGIN
    assert b.cost[0] != a.cost[-1]  # the second run's cost is the robust one


def test_nan_and_inf_trials_are_rejected():
    """``t < c`` is false for NaN and +inf: the comparison the kernel uses, stated on doubles."""
    c = np.float64(3.0)
    assert not (np.float64("nan") < c) and not (np.float64("inf") < c)
