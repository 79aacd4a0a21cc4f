"""CPU restatement of the BA's Huber-robust cost (DESIGN.md §Bundle adjustment -> Model, §Robust cost).

Test infrastructure, built on ``oracle/ba_ref.py``: its ``residuals``, ``jacobians``, Schur
complement, solve, back substitution and update are used as they are.  Restated here is only
what the robust cost adds: the per-observation scale, ``sum(rho)`` and the stepping loop.

Model: for an observation with raw residual ``r`` and ``n2 = r.r``,

* ``n2 <= delta^2``: ``rho = n2``, ``s = 1``;
* otherwise ``n = sqrt(n2)``, ``rho = 2 delta n - delta^2``, ``s = sqrt(delta / n)``;

the linearised system is the oracle's over ``s r``, ``s J_pose``, ``s J_point`` (first-order IRLS),
and every reported cost is ``sum(rho)``.  ``delta = 0`` is the oracle itself.
"""

from __future__ import annotations

import contextlib
import dataclasses

import numpy as np

from oracle import ba_ref

OUTLIER_FRACTION = 0.05


def huber_scale(r: np.ndarray, delta: float):
    """(s (M,), rho (M,), beyond (M,) bool) of raw residuals r (M,2)."""
    n2 = (r * r).sum(-1)
    beyond = n2 > delta * delta
    n = np.sqrt(np.where(beyond, n2, 1.0))
    s = np.where(beyond, np.sqrt(delta / n), 1.0)
    rho = np.where(beyond, 2.0 * delta * n - delta * delta, n2)
    return s, rho, beyond


def cost(st: ba_ref.BAState, s: ba_ref.BAStructure, delta: float) -> float:
    r, _ = ba_ref.residuals(st, s)
    if delta <= 0:
        return float(np.sum(r * r))
    return float(huber_scale(r, delta)[1].sum())


@contextlib.contextmanager
def _scaled_linearisation(delta: float, out: dict):
    """Inside: the oracle's ``residuals`` / ``jacobians`` return the scaled quantities, so its
    ``build_system`` / ``back_substitute`` run unchanged on them.  out["rho"] = sum(rho).

    It swaps two globals of the oracle module for the duration of the call (``ba_ref.gn_step``
    resolves them at module scope): not thread-safe.  Call the restatement from the test's main
    thread only, never from the loopback worker threads, and not while they use the oracle."""
    res0, jac0 = ba_ref.residuals, ba_ref.jacobians

    def res(st, s):
        r, pc = res0(st, s)
        sc, rho, _ = huber_scale(r, delta)
        out["s"], out["rho"] = sc, float(rho.sum())
        return r * sc[:, None], pc

    def jac(st, s, pc):
        Jc, Jp = jac0(st, s, pc)
        return Jc * out["s"][:, None, None], Jp * out["s"][:, None, None]

    ba_ref.residuals, ba_ref.jacobians = res, jac
    try:
        yield
    finally:
        ba_ref.residuals, ba_ref.jacobians = res0, jac0


def gn_step(st: ba_ref.BAState, s: ba_ref.BAStructure, lam: float, delta: float) -> ba_ref.GNStep:
    """One GN step under the Huber cost; ``system.cost`` is ``sum(rho)`` at ``st``."""
    if delta <= 0:
        return ba_ref.gn_step(st, s, lam)
    out: dict = {}
    with _scaled_linearisation(delta, out):
        step = ba_ref.gn_step(st, s, lam)
    return dataclasses.replace(step, system=dataclasses.replace(step.system, cost=out["rho"]))


def solve_schedule(st: ba_ref.BAState, s: ba_ref.BAStructure, schedule, lam: float):
    """``schedule``: [(iters, delta), ...] run one after another, as ``run(iters)`` calls with
    ``set_robust(delta)`` between them: per part its costs[iters + 1] (the last one at the part's
    own delta).  Returns (state, [costs, ...])."""
    parts = []
    for iters, delta in schedule:
        costs = []
        for _ in range(iters):
            step = gn_step(st, s, lam, delta)
            costs.append(step.system.cost)
            st = step.state
        costs.append(cost(st, s, delta))
        parts.append(np.array(costs))
    return st, parts


def solve(st: ba_ref.BAState, s: ba_ref.BAStructure, iters: int, lam: float, delta: float):
    """``iters`` robust GN steps, all accepted -> (state, costs[iters + 1])."""
    st, parts = solve_schedule(st, s, [(iters, delta)], lam)
    return st, parts[0]


def irls_gradient(st: ba_ref.BAState, s: ba_ref.BAStructure, delta: float):
    """2 (sJ)^T (s r): (n_poses, 6) w.r.t. each pose's left twist and (L, 3) w.r.t. the points."""
    r, pc = ba_ref.residuals(st, s)
    sc = huber_scale(r, delta)[0]
    Jc, Jp = ba_ref.jacobians(st, s, pc)
    sr = r * sc[:, None]
    g_pose = np.zeros((s.n_poses, 6))
    np.add.at(g_pose, s.obs_cam, 2.0 * np.einsum("mki,mk->mi", Jc * sc[:, None, None], sr))
    g_pt = np.zeros_like(st.X)
    np.add.at(g_pt, s.obs_pt, 2.0 * np.einsum("mki,mk->mi", Jp * sc[:, None, None], sr))
    return g_pose, g_pt


def with_outliers(p, seed: int) -> np.ndarray:
    """The problem's measurements with 5 % of them moved 30-100 px in a random direction
    (``rng = default_rng(100 + seed)``), float32."""
    rng = np.random.default_rng(100 + seed)
    uv = p.obs_uv.copy()
    M = uv.shape[0]
    k = int(OUTLIER_FRACTION * M)
    idx = rng.permutation(M)[:k]
    ang = rng.uniform(0, 2 * np.pi, k)
    mag = rng.uniform(30, 100, k)
    uv[idx] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], -1).astype(np.float32)
    return uv


def structure(p, uv=None) -> ba_ref.BAStructure:
    return ba_ref.BAStructure(p.K, p.point_ptr, p.obs_cam, p.obs_uv if uv is None else uv, p.n_fixed, p.n_poses)


def max_translation_error(poses_cw: np.ndarray, p) -> float:
    """Largest translation error of any pose against the problem's truth (metres)."""
    return float(np.abs(np.asarray(poses_cw)[:, :3, 3] - p.poses_true[:, :3, 3]).max())
