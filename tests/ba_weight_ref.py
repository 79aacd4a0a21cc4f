"""CPU restatement of the BA's observation weights and culling (DESIGN.md §Observation weights and
culling, ``vo_ba_set_obs_weights`` / ``vo_ba_cull`` in include/vo_hip.h).

Test infrastructure on ``oracle/ba_ref.py`` in the style of ``tests/ba_robust_ref.py``: the oracle's
``residuals``, ``jacobians``, Schur complement, solve, back substitution and update are used as they
are.  Restated here is only what the weights add.

Model: observation ``o`` has an information weight ``w_o >= 0``; with ``r``, ``J_pose``, ``J_point``
the oracle's raw residual and Jacobians,

* ``w_o > 0``: the linearisation uses ``sqrt(w_o)`` times all three; the Huber rule (if any) is
  applied to the whitened residual, ``n2 = w_o r.r`` against ``delta^2``, its scale multiplying on
  top; the cost term is ``rho(w_o r.r)``, without Huber ``w_o r.r``;
* ``w_o == 0``: a select -- exact zeros whatever the raw values are, non-finite ones included.

The cull at a state: with ``err2 = r.r`` and ``z`` the camera-frame depth, an active observation is
deactivated iff ``max_chi2 > 0 and w err2 > max_chi2``, or ``z <= min_depth``, or either is not
finite; then every landmark with fewer than ``min_track`` active observations loses all of them.
"""

from __future__ import annotations

import contextlib
import dataclasses

import numpy as np

from oracle import ba_ref
from tests import ba_lm_ref as lmr
from tests import ba_robust_ref as rr


def whiten(r: np.ndarray, w: np.ndarray, delta: float):
    """(scale (M,), rho (M,)) of raw residuals r (M,2) under weights w: ``scale`` multiplies r and
    both Jacobians (sqrt(w) times the Huber scale of the whitened residual, 0 where w == 0), ``rho``
    is the observation's cost term (0 where w == 0)."""
    w = np.asarray(w, dtype=np.float64)
    on = w > 0
    sw = np.sqrt(w)
    with np.errstate(all="ignore"):
        rw = np.where(on[:, None], r * sw[:, None], 0.0)
    if delta > 0:
        s, rho, _ = rr.huber_scale(rw, delta)
    else:
        s, rho = np.ones(r.shape[0]), (rw * rw).sum(-1)
    return np.where(on, sw * s, 0.0), np.where(on, rho, 0.0)


def _scaled(a: np.ndarray, scale: np.ndarray) -> np.ndarray:
    """a * scale per observation, exact zeros where scale == 0 (a may be non-finite there)."""
    sc = scale.reshape((-1,) + (1,) * (a.ndim - 1))
    with np.errstate(all="ignore"):
        return np.where(sc > 0, a * sc, 0.0)


def cost(st: ba_ref.BAState, s: ba_ref.BAStructure, w, delta: float = 0.0) -> float:
    with np.errstate(all="ignore"):
        r, _ = ba_ref.residuals(st, s)
    return float(whiten(r, w, delta)[1].sum())


@contextlib.contextmanager
def _weighted_linearisation(w, delta: float, out: dict):
    """Inside: the oracle's ``residuals`` / ``jacobians`` return the whitened quantities
    (``ba_robust_ref._scaled_linearisation``'s device, and its caveat: main thread only)."""
    res0, jac0 = ba_ref.residuals, ba_ref.jacobians

    def res(st, s):
        with np.errstate(all="ignore"):
            r, pc = res0(st, s)
        out["scale"], rho = whiten(r, w, delta)
        out["rho"] = float(rho.sum())
        return _scaled(r, out["scale"]), pc

    def jac(st, s, pc):
        with np.errstate(all="ignore"):
            Jc, Jp = jac0(st, s, pc)
        return _scaled(Jc, out["scale"]), _scaled(Jp, out["scale"])

    ba_ref.residuals, ba_ref.jacobians = res, jac
    try:
        yield
    finally:
        ba_ref.residuals, ba_ref.jacobians = res0, jac0


def gn_step(st: ba_ref.BAState, s: ba_ref.BAStructure, lam: float, w, delta: float = 0.0) -> ba_ref.GNStep:
    """One GN step under the weights (and Huber delta); ``system.cost`` is the weighted cost at ``st``."""
    out: dict = {}
    with _weighted_linearisation(np.asarray(w, dtype=np.float64), delta, out):
        step = ba_ref.gn_step(st, s, lam)
    return dataclasses.replace(step, system=dataclasses.replace(step.system, cost=out["rho"]))


def solve(st: ba_ref.BAState, s: ba_ref.BAStructure, iters: int, lam: float, w, delta: float = 0.0):
    """``iters`` weighted GN steps, all accepted -> (state, costs[iters + 1])."""
    costs = []
    for _ in range(iters):
        step = gn_step(st, s, lam, w, delta)
        costs.append(step.system.cost)
        st = step.state
    costs.append(cost(st, s, w, delta))
    return st, np.array(costs)


def solve_lm(st: ba_ref.BAState, s: ba_ref.BAStructure, iters: int, w, delta: float, lam0: float,
             up: float = lmr.UP, down: float = lmr.DOWN, lam_min: float = lmr.LAM_MIN,
             lam_max: float = lmr.LAM_MAX) -> lmr.LMLog:
    """``ba_lm_ref.solve``'s loop over the weighted step and cost."""
    lam = float(min(max(lam0 if lam0 > 0 else lmr.LAM0_DEFAULT, lam_min), lam_max))
    c = cost(st, s, w, delta)
    cs, lams, trial, acc = [], [], [], []
    for _ in range(iters):
        cs.append(c)
        lams.append(lam)
        cand = gn_step(st, s, lam, w, delta).state
        t = cost(cand, s, w, delta)
        trial.append(t)
        if t < c:
            st, c = cand, t
            lam = max(lam * down, lam_min)
            acc.append(1)
        else:
            lam = min(lam * up, lam_max)
            acc.append(0)
    cs.append(c)
    lams.append(lam)
    return lmr.LMLog(st, np.array(cs), np.array(lams), np.array(trial), np.array(acc, dtype=np.uint8))


def gradient(st: ba_ref.BAState, s: ba_ref.BAStructure, w, delta: float = 0.0):
    """2 (sJ)^T (s r) with s the whitening scale: (n_poses, 6) and (L, 3), as
    ``ba_robust_ref.irls_gradient``."""
    with np.errstate(all="ignore"):
        r, pc = ba_ref.residuals(st, s)
        Jc, Jp = ba_ref.jacobians(st, s, pc)
    sc = whiten(r, w, delta)[0]
    sr = _scaled(r, sc)
    g_pose = np.zeros((s.n_poses, 6))
    np.add.at(g_pose, s.obs_cam, 2.0 * np.einsum("mki,mk->mi", _scaled(Jc, sc), sr))
    g_pt = np.zeros_like(st.X)
    np.add.at(g_pt, s.obs_pt, 2.0 * np.einsum("mki,mk->mi", _scaled(Jp, sc), sr))
    return g_pose, g_pt


def raw_err2_depth(st: ba_ref.BAState, s: ba_ref.BAStructure):
    """(err2, z) per observation: what ``vo_ba_residuals`` reports."""
    with np.errstate(all="ignore"):
        r, pc = ba_ref.residuals(st, s)
        return (r * r).sum(-1), pc[:, 2].copy()


def cull_weights(err2, z, w, point_ptr, max_chi2: float = 0.0, min_depth: float = 0.0, min_track: int = 2):
    """The cull rule on given per-observation values -> the new weights (a copy of ``w`` with the
    deactivated observations at 0)."""
    err2, z = np.asarray(err2, dtype=np.float64), np.asarray(z, dtype=np.float64)
    w = np.array(w, dtype=np.float64)
    active = w > 0
    with np.errstate(all="ignore"):
        bad = ~(np.isfinite(err2) & np.isfinite(z)) | (z <= min_depth)
        if max_chi2 > 0:
            bad |= w * err2 > max_chi2
    w[active & bad] = 0.0
    if min_track > 0:
        point_ptr = np.asarray(point_ptr)
        obs_pt = np.repeat(np.arange(point_ptr.size - 1), np.diff(point_ptr))
        n_act = np.bincount(obs_pt[w > 0], minlength=point_ptr.size - 1)
        w[(n_act < min_track)[obs_pt]] = 0.0
    return w


def cull(st: ba_ref.BAState, s: ba_ref.BAStructure, w, max_chi2: float = 0.0, min_depth: float = 0.0,
         min_track: int = 2):
    err2, z = raw_err2_depth(st, s)
    return cull_weights(err2, z, w, s.point_ptr, max_chi2, min_depth, min_track)


# The outlier schedule the device test runs (tests/test_gpu_ba_weights.py) on
# ``ba_robust_ref.with_outliers``: window, Huber delta, chi^2 bound (3 px at unit weight), rounds,
# iterations per part; lambda = 1.  No chi^2 decision of the restatement lies within CULL_MARGIN of
# the bound at either cull (the nearest is 8e-2 away): tests/test_ba_weight_ref.py re-establishes it.
SCHEDULE = dict(win=(8, 300, 21), delta=2.0, max_chi2=9.0, rounds=2, iters=5)
CULL_MARGIN = 1e-6


def cull_schedule(st: ba_ref.BAState, s: ba_ref.BAStructure, rounds: int, iters: int, lam: float, delta: float,
                  max_chi2: float, min_depth: float = 0.0, min_track: int = 2, w=None, near_rel: float = 1e-6):
    """``rounds + 1`` GN solves of ``iters`` each with a cull between them -> (state, weights,
    [costs per part], smallest chi^2 margin met at any cull, mask of the observations whose
    ``w err2`` lay within ``near_rel`` of ``max_chi2`` at a cull)."""
    w = np.ones(s.obs_cam.size) if w is None else np.array(w, dtype=np.float64)
    parts, margin, near = [], np.inf, np.zeros(s.obs_cam.size, bool)
    for k in range(rounds + 1):
        st, costs = solve(st, s, iters, lam, w, delta)
        parts.append(costs)
        if k < rounds:
            err2, _ = raw_err2_depth(st, s)
            ok = (w > 0) & np.isfinite(err2)
            m = np.full(w.size, np.inf)
            m[ok] = np.abs(w[ok] * err2[ok] - max_chi2) / max_chi2
            margin = min(margin, float(m.min()))
            near |= m < near_rel
            w = cull(st, s, w, max_chi2, min_depth, min_track)
    return st, w, parts, margin, near


def cov_dense(st: ba_ref.BAState, s: ba_ref.BAStructure, lam: float, w, delta: float = 0.0):
    """``ba_cov_ref.route_b`` fed the whitened Jacobians: (Sigma_cc, Sigma_pp) from the dense inverse
    of J^T W J + lam I (no landmark is frozen here)."""
    import scipy.linalg

    with np.errstate(all="ignore"):
        r, pc = ba_ref.residuals(st, s)
        Jc, Jp = ba_ref.jacobians(st, s, pc)
    sc = whiten(r, w, delta)[0]
    Jc, Jp = _scaled(Jc, sc), _scaled(Jp, sc)
    nf, NF, L = s.n_fixed, s.n_free, s.n_points
    n = 6 * NF + 3 * L
    J = np.zeros((2 * r.shape[0], n))
    for o in range(r.shape[0]):
        c, p = s.obs_cam[o], s.obs_pt[o]
        if c >= nf:
            J[2 * o : 2 * o + 2, 6 * (c - nf) : 6 * (c - nf) + 6] = Jc[o]
        J[2 * o : 2 * o + 2, 6 * NF + 3 * p : 6 * NF + 3 * p + 3] = Jp[o]
    H = J.T @ J + lam * np.eye(n)
    Hi = scipy.linalg.cho_solve(scipy.linalg.cho_factor(H, lower=True), np.eye(n))
    Hi = 0.5 * (Hi + Hi.T)
    idx = 6 * NF + 3 * np.arange(L)[:, None] + np.arange(3)[None, :]
    return Hi[: 6 * NF, : 6 * NF], Hi[idx[:, :, None], idx[:, None, :]]


def cov_schur(st: ba_ref.BAState, s: ba_ref.BAStructure, lam: float, w, delta: float = 0.0):
    """``ba_cov_ref.route_a`` on the weighted system (the definition the library follows)."""
    from tests import ba_cov_ref as cr

    sys0 = cr._system
    out: dict = {}

    def system(st_, s_, lam_, delta_):
        with _weighted_linearisation(np.asarray(w, dtype=np.float64), delta_, out):
            return ba_ref.build_system(st_, s_, lam_)

    cr._system = system
    try:
        return cr.route_a(st, s, lam, delta)
    finally:
        cr._system = sys0


def repeated_structure(p, reps, uv=None):
    """The problem with observation ``o`` repeated ``reps[o]`` times (0: dropped), every landmark
    kept (one without observations has an empty track) -> (BAStructure, the source observation of
    each new one)."""
    reps = np.asarray(reps, dtype=np.int64)
    src = np.repeat(np.arange(reps.size), reps)
    obs_pt = np.repeat(np.arange(p.point_ptr.size - 1), np.diff(p.point_ptr))
    ptr = np.zeros(p.point_ptr.size, dtype=np.int32)
    ptr[1:] = np.cumsum(np.bincount(obs_pt[src], minlength=p.point_ptr.size - 1))
    uv = p.obs_uv if uv is None else uv
    s = ba_ref.BAStructure(p.K, ptr, np.ascontiguousarray(p.obs_cam[src]), np.ascontiguousarray(uv[src]),
                           p.n_fixed, p.n_poses)
    return s, src
