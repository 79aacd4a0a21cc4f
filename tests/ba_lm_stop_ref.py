"""CPU restatement of the LM loop's termination tests (DESIGN.md §Step control, ``vo_ba_set_lm_stop``
in include/vo_hip.h), on top of ``tests/ba_lm_ref.py``.

The loop is ``ba_lm_ref.solve``'s, with three tests after each decision; ``rej`` counts consecutive
rejections and starts at 0::

    for k in 0 .. iters-1:
        ... trial k as in ba_lm_ref.solve ...
        if accepted:
            rej = 0
            if ftol > 0 and (c - t) <= ftol * c:        stop, FTOL      (c = cost[k], t = trial[k])
            elif xtol > 0 and max|dc| <= xtol:          stop, XTOL      (dc: trial k's pose update)
        else:
            rej += 1
            if max_rejects > 0 and rej >= max_rejects:  stop, REJECTS
        on stop: trials = k + 1
    otherwise trials = iters, RAN_ALL

After a stop the log's tail repeats the stopped cost and damping, with ``trial = NaN`` and
``accepted = 0``.
"""

from __future__ import annotations

import dataclasses

import numpy as np

from oracle import ba_ref
from tests import ba_lm_ref as lr
from tests import ba_robust_ref as rr

RAN_ALL, FTOL, XTOL, REJECTS = 0, 1, 2, 3
FAILED = -1
REASONS = {RAN_ALL: "ran_all", FTOL: "ftol", XTOL: "xtol", REJECTS: "rejects"}


@dataclasses.dataclass
class StopLog:
    state: ba_ref.BAState
    cost: np.ndarray  # (iters + 1,)
    lam: np.ndarray  # (iters + 1,)
    trial: np.ndarray  # (iters,), NaN behind the stop
    accepted: np.ndarray  # (iters,) uint8, 0 behind the stop
    trials: int
    reason: int
    margin: float  # smallest relative distance of a tested quantity from its tolerance (inf: none tested)


def solve(st: ba_ref.BAState, s: ba_ref.BAStructure, iters: int, delta: float, lam0: float, ftol: float = 0.0,
          xtol: float = 0.0, max_rejects: int = 0, up: float = lr.UP, down: float = lr.DOWN,
          lam_min: float = lr.LAM_MIN, lam_max: float = lr.LAM_MAX) -> StopLog:
    lam = float(min(max(lam0 if lam0 > 0 else lr.LAM0_DEFAULT, lam_min), lam_max))
    c = rr.cost(st, s, delta)
    cost, lams = [c], [lam]
    trial = np.full(iters, np.nan)
    acc = np.zeros(iters, dtype=np.uint8)
    trials, reason, rej, margin = iters, RAN_ALL, 0, np.inf
    for k in range(iters):
        step = rr.gn_step(st, s, lam, delta)
        t = rr.cost(step.state, s, delta)
        trial[k] = t
        stop = None
        if t < c:
            acc[k] = 1
            rej = 0
            if ftol > 0:
                margin = min(margin, abs((c - t) / c - ftol) / ftol)
            if xtol > 0:
                margin = min(margin, abs(np.abs(step.dc).max() - xtol) / xtol)
            if ftol > 0 and (c - t) <= ftol * c:
                stop = FTOL
            elif xtol > 0 and np.abs(step.dc).max() <= xtol:
                stop = XTOL
            st, c = step.state, t
            lam = max(lam * down, lam_min)
        else:
            lam = min(lam * up, lam_max)
            rej += 1
            if max_rejects > 0 and rej >= max_rejects:
                stop = REJECTS
        cost.append(c)
        lams.append(lam)
        if stop is not None:
            trials, reason = k + 1, stop
            break
    cost += [c] * (iters + 1 - len(cost))
    lams += [lam] * (iters + 1 - len(lams))
    return StopLog(st, np.array(cost), np.array(lams), trial, acc, trials, reason, float(margin))


# The table of the device tests: (case of ba_lm_ref.CASES, ftol, xtol, max_rejects) -> (trials, reason),
# twelve iterations of the default schedule.  tests/test_ba_lm_stop_ref.py re-establishes every row and
# the fitness condition: each tested quantity of an accepted step lies at least MARGIN (relative)
# away from its tolerance, so a device within 1e-8 per step cannot decide differently.
MARGIN = 0.1
ROWS = {
    "A-ftol": ("A", 1e-2, 0.0, 0, 8, FTOL),
    "A-xtol": ("A", 0.0, 1e-2, 0, 8, XTOL),
    "A-ftol-xtol": ("A", 1e-2, 1e-2, 0, 8, FTOL),
    "A-rej1": ("A", 0.0, 0.0, 1, 3, REJECTS),
    "A-never": ("A", 1e-5, 1e-5, 2, 12, RAN_ALL),
    "T-ftol": ("T", 5e-3, 0.0, 0, 10, FTOL),
    "T-rej1": ("T", 0.0, 0.0, 1, 7, REJECTS),
    "T2-xtol": ("T2", 0.0, 2e-2, 0, 11, XTOL),
    "T2-ftol": ("T2", 1e-3, 0.0, 0, 11, FTOL),
    "C-ftol": ("C", 0.12, 0.0, 0, 4, FTOL),
    "C-rej3": ("C", 0.0, 0.0, 3, 8, REJECTS),
    "E-ftol-rej5": ("E", 6e-2, 0.0, 5, 9, FTOL),
    "B-rej4": ("B", 0.0, 0.0, 4, 4, REJECTS),
    "B-rej5": ("B", 0.0, 0.0, 5, 12, RAN_ALL),
    "Bclamp-rej4": ("Bclamp", 0.0, 0.0, 4, 4, REJECTS),
}
_logs: dict = {}


def row_log(row: str, iters: int = lr.ITERS) -> StopLog:
    """The restatement's run of a table row from the case's initial guess (computed once)."""
    if (row, iters) not in _logs:
        name, ftol, xtol, max_rejects, _, _ = ROWS[row]
        win, delta, lam0, lam_max, _ = lr.CASES[name]
        _, _, s, st0 = lr.window(win)
        _logs[row, iters] = solve(st0, s, iters, delta, lam0, ftol, xtol, max_rejects, lam_max=lam_max)
    return _logs[row, iters]
