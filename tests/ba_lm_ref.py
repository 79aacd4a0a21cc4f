"""CPU restatement of the BA's Levenberg-Marquardt step control (DESIGN.md §Step control,
``vo_ba_run_lm`` in include/vo_hip.h).

Test infrastructure on top of ``tests/ba_robust_ref.py`` (and through it ``oracle/ba_ref.py``): the
step is ``ba_robust_ref.gn_step`` with the damping of the moment, the cost ``ba_robust_ref.cost``.
Restated here is only the loop::

    for k in 0 .. iters-1:
        cost[k] = c ; lambda[k] = lam
        x' = x (+) step(x, lam) ;  t = cost(x') ;  trial[k] = t
        if t < c:   x = x' ; c = t ; lam = max(lam * down, lam_min) ; accepted[k] = 1
        else:       lam = min(lam * up, lam_max) ;                    accepted[k] = 0
    cost[iters] = c ; lambda[iters] = lam

``t < c`` is false for NaN and +inf.  The damping updates are those two double multiplications and
clamps and nothing else, so with equal decisions the device's lambda log equals this one bit for
bit.  A ``numpy.linalg.LinAlgError`` inside the reference step is not a rejection: it propagates,
and marks the case as unfit for a test.
"""

from __future__ import annotations

import dataclasses

import numpy as np

from oracle import ba_ref
from tests import ba_robust_ref as rr

UP, DOWN, LAM_MIN, LAM_MAX = 10.0, 0.1, 1e-6, 1e6
LAM0_DEFAULT = 1e-4  # when neither the options nor the problem give a positive damping


@dataclasses.dataclass
class LMLog:
    state: ba_ref.BAState
    cost: np.ndarray  # (iters + 1,) accepted-state cost before each trial and after the last
    lam: np.ndarray  # (iters + 1,) damping, likewise
    trial: np.ndarray  # (iters,) cost of each trial state
    accepted: np.ndarray  # (iters,) uint8

    def pattern(self) -> str:
        return "".join(str(int(a)) for a in self.accepted)

    def margins(self) -> np.ndarray:
        """|t - c| / c of every decision."""
        return np.abs(self.trial - self.cost[:-1]) / self.cost[:-1]


def solve(st: ba_ref.BAState, s: ba_ref.BAStructure, iters: int, delta: float, lam0: float, up: float = UP,
          down: float = DOWN, lam_min: float = LAM_MIN, lam_max: float = LAM_MAX) -> LMLog:
    lam = float(min(max(lam0 if lam0 > 0 else LAM0_DEFAULT, lam_min), lam_max))
    c = rr.cost(st, s, delta)
    cost, lams, trial, acc = [], [], [], []
    for _ in range(iters):
        cost.append(c)
        lams.append(lam)
        cand = rr.gn_step(st, s, lam, delta).state
        t = rr.cost(cand, s, delta)
        trial.append(t)
        if t < c:
            st, c = cand, t
            lam = max(lam * down, lam_min)
            acc.append(1)
        else:
            lam = min(lam * up, lam_max)
            acc.append(0)
    cost.append(c)
    lams.append(lam)
    return LMLog(st, np.array(cost), np.array(lams), np.array(trial), np.array(acc, dtype=np.uint8))


# The windows the device tests run (make_ba_problem(n, L, seed) with ba_robust_ref.with_outliers),
# twelve iterations of the default schedule each: (window, delta, lam0, lam_max, accepted pattern).
# tests/test_ba_lm_ref.py re-establishes every row, and that every decision's relative margin is
# at least MARGIN, before the device tests rely on it.
ITERS = 12
MARGIN = 1e-4
CASES = {
    "A": ((8, 300, 21), 2.0, 1.0, LAM_MAX, "110111011111"),
    "B": ((12, 600, 3), 0.0, 1e-4, LAM_MAX, "000010101001"),
    "C": ((6, 120, 5), 2.0, 1e-4, LAM_MAX, "111110000000"),
    "E": ((8, 300, 21), 0.0, 1e-4, LAM_MAX, "000011011111"),
    "T": ((3, 12, 1), 2.0, 1e-4, LAM_MAX, "111111011111"),
    "T2": ((4, 20, 2), 0.0, 1e-4, LAM_MAX, "000001011111"),
    "Bclamp": ((12, 600, 3), 0.0, 1e-4, 1e-2, "000000000000"),
}
_windows: dict = {}
_logs: dict = {}


def window(win):
    """(problem, measurements with outliers, structure, initial state) of a window, built once."""
    if win not in _windows:
        from visualodometry_amd.synthetic import make_ba_problem

        p = make_ba_problem(*win)
        uv = rr.with_outliers(p, win[2])
        _windows[win] = (p, uv, rr.structure(p, uv), ba_ref.BAState.from_poses(p.poses_cw, p.points))
    return _windows[win]


def case_log(name: str, iters: int = ITERS) -> LMLog:
    """The restatement's run of a case from its initial guess (computed once, never modified)."""
    if (name, iters) not in _logs:
        win, delta, lam0, lam_max, _ = CASES[name]
        _, _, s, st0 = window(win)
        _logs[name, iters] = solve(st0, s, iters, delta, lam0, lam_max=lam_max)
    return _logs[name, iters]


def robust_switch_logs():
    """Case E's window: three plain-cost LM iterations, then ``set_robust(2)`` and three more (each
    run starting at lambda 1e-4) -> (first log, second log)."""
    if "switch" not in _logs:
        _, _, s, st0 = window(CASES["E"][0])
        a = solve(st0, s, 3, 0.0, 1e-4)
        _logs["switch"] = (a, solve(a.state, s, 3, 2.0, 1e-4))
    return _logs["switch"]
