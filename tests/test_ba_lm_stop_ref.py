"""The CPU restatement of the LM loop's termination tests (tests/ba_lm_stop_ref.py) on the windows
of tests/ba_lm_ref.py: every row of the table the device tests rely on, the tail of a stopped log,
that a stop leaves the trials before it as the unconfigured loop has them -- and the fitness
condition: every tested quantity of an accepted step lies at least 10 % away from its tolerance, so
a device that meets the project's 1e-8 per-step parity cannot decide differently.  That is a
condition on the inputs: a row that stops meeting it is replaced, not loosened.
"""

import numpy as np
import pytest

from tests import ba_lm_ref as lr
from tests import ba_lm_stop_ref as sr


@pytest.mark.parametrize("row", list(sr.ROWS))
def test_row(row):
    name, ftol, xtol, max_rejects, trials, reason = sr.ROWS[row]
    log = sr.row_log(row)
    print(row, log.trials, sr.REASONS[log.reason], f"smallest margin {log.margin:.3g}")
    assert (log.trials, log.reason) == (trials, reason)
    if ftol > 0 or xtol > 0:
        assert log.margin >= sr.MARGIN
    # the trials up to the stop are the unconfigured loop's
    full = lr.case_log(name)
    k = log.trials
    assert np.array_equal(log.accepted[:k], full.accepted[:k])
    assert np.array_equal(log.trial[:k], full.trial[:k])
    assert np.array_equal(log.cost[:k + 1], full.cost[:k + 1]) and np.array_equal(log.lam[:k + 1], full.lam[:k + 1])
    # the tail repeats the stopped cost and damping
    assert np.isnan(log.trial[k:]).all() and not log.accepted[k:].any()
    assert (log.cost[k:] == log.cost[k]).all() and (log.lam[k:] == log.lam[k]).all()
    assert np.isfinite(log.cost).all() and (np.diff(log.cost) <= 0).all()
    # the reason, restated on the log
    if reason == sr.REJECTS:
        assert not log.accepted[k - max_rejects:k].any() and k >= max_rejects
    elif reason in (sr.FTOL, sr.XTOL):
        assert log.accepted[k - 1]
    if reason == sr.FTOL:
        assert log.cost[k - 1] - log.trial[k - 1] <= ftol * log.cost[k - 1]


def test_the_stopped_state_is_the_shorter_runs():
    """A stop changes nothing before it: the state equals an unconfigured run of `trials` iterations."""
    for row in ("A-ftol", "C-rej3"):
        log = sr.row_log(row)
        short = lr.case_log(sr.ROWS[row][0], log.trials)
        assert np.array_equal(log.state.X, short.state.X) and np.array_equal(log.state.R, short.state.R)
        assert np.array_equal(log.state.t, short.state.t)
        assert np.array_equal(log.cost[:log.trials + 1], short.cost)


def test_ftol_goes_before_xtol_and_leading_rejections_do_not_trip():
    both, x = sr.row_log("A-ftol-xtol"), sr.row_log("A-xtol")
    assert both.trials == x.trials and both.reason == sr.FTOL and x.reason == sr.XTOL
    e = sr.row_log("E-ftol-rej5")
    assert not e.accepted[:4].any() and e.accepted[4]  # four leading rejections, fewer than max_rejects = 5
    assert sr.row_log("B-rej5").reason == sr.RAN_ALL  # B never rejects five times in a row


def test_no_criterion_is_the_plain_loop():
    for name in ("A", "C"):
        win, delta, lam0, lam_max, _ = lr.CASES[name]
        _, _, s, st0 = lr.window(win)
        log, full = sr.solve(st0, s, lr.ITERS, delta, lam0, lam_max=lam_max), lr.case_log(name)
        assert (log.trials, log.reason) == (lr.ITERS, sr.RAN_ALL) and log.margin == np.inf
        assert np.array_equal(log.cost, full.cost) and np.array_equal(log.lam, full.lam)
        assert np.array_equal(log.trial, full.trial) and np.array_equal(log.accepted, full.accepted)
