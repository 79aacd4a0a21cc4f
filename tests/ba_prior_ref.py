"""CPU restatement of the BA's pose prior (DESIGN.md §Pose prior, ``vo_ba_setup_prior`` in
include/vo_hip.h) and of the marginalisation that produces one.

Test infrastructure on ``oracle/ba_ref.py`` in the style of ``tests/ba_weight_ref.py``: the oracle's
linearisation, Schur complement, solve, back substitution and update are used as they are (through
``ba_weight_ref`` when weights or a Huber delta are given).  Restated here is only what the prior adds.

Model: the prior covers free poses ``0 .. K-1``.  With ``xi_f = log(T_f T0_f^-1)`` (the inverse of the
oracle's ``se3_exp``, twist ``(rho, phi)``) stacked into ``xi``,

    E_prior = cost0 - 2 eta^T xi + xi^T Lambda xi

is added to the cost, and with the first-order Jacobian ``d xi / d delta ~ I`` the reduced system
``S dc = b`` becomes ``(S + Lambda^) dc = b + (eta^ - Lambda^ xi^)``, the hats padding to ``6F``.

:func:`marginalize` builds the prior of a slide with dense numpy: the Schur complement, onto the
remaining free poses, of every factor that touches a landmark seen from the dropped cameras.
"""

from __future__ import annotations

import dataclasses

import numpy as np

from oracle import ba_ref
from tests import ba_lm_ref as lmr
from tests import ba_weight_ref as wr


@dataclasses.dataclass
class Prior:
    info: np.ndarray  # (6K,6K) Lambda, symmetric
    rhs: np.ndarray  # (6K,) eta
    poses0: np.ndarray  # (K,4,4) linearisation poses
    cost0: float = 0.0

    @property
    def k(self) -> int:
        return self.poses0.shape[0]


def se3_log(R: np.ndarray, t: np.ndarray) -> np.ndarray:
    """Twists (...,6) = (rho, phi) with ``ba_ref.se3_exp(twist) == (R, t)``; rotations below pi.
    The coefficients are ``se3_exp``'s own (its series below its threshold), so the two invert each
    other to rounding on both sides of it."""
    v = 0.5 * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    c = 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1.0)
    th = np.arctan2(np.sqrt(np.sum(v * v, -1)), c)
    th2 = th * th
    small = th < ba_ref.EXP_TAYLOR_THETA
    ths = np.where(small, 1.0, th)
    A = np.where(small, 1.0 - th2 / 6.0, np.sin(ths) / ths)
    B = np.where(small, 0.5 - th2 / 24.0, (1.0 - np.cos(ths)) / ths**2)
    C = np.where(small, 1.0 / 6.0 - th2 / 120.0, (ths - np.sin(ths)) / ths**3)
    phi = v / A[..., None]
    P = ba_ref.skew(phi)
    V = np.broadcast_to(np.eye(3), P.shape) + B[..., None, None] * P + C[..., None, None] * (P @ P)
    rho = np.linalg.solve(V, t[..., None])[..., 0]
    return np.concatenate([rho, phi], -1)


def twists(st: ba_ref.BAState, s: ba_ref.BAStructure, prior: Prior) -> np.ndarray:
    """xi (6K): the log of T_f T0_f^-1 for the prior's poses at state ``st``."""
    nf, k = s.n_fixed, prior.k
    R0, t0 = prior.poses0[:, :3, :3], prior.poses0[:, :3, 3]
    D = st.R[nf:nf + k] @ np.swapaxes(R0, -1, -2)
    d = st.t[nf:nf + k] - np.einsum("nij,nj->ni", D, t0)
    return se3_log(D, d).ravel()


def prior_cost(xi: np.ndarray, prior: Prior) -> float:
    return float(prior.cost0 - 2.0 * prior.rhs @ xi + xi @ prior.info @ xi)


def prior_terms(st: ba_ref.BAState, s: ba_ref.BAStructure, prior: Prior):
    """(S_add (6F,6F), b_add (6F), E_prior) at ``st``."""
    n, m = 6 * s.n_free, 6 * prior.k
    xi = twists(st, s, prior)
    S = np.zeros((n, n))
    b = np.zeros(n)
    S[:m, :m] = prior.info
    b[:m] = prior.rhs - prior.info @ xi
    return S, b, prior_cost(xi, prior)


def cost(st, s, prior: Prior | None, w=None, delta: float = 0.0) -> float:
    w = np.ones(s.obs_cam.size) if w is None else w
    c = wr.cost(st, s, w, delta)
    return c if prior is None else c + prior_cost(twists(st, s, prior), prior)


def gn_step(st, s, lam: float, prior: Prior | None, w=None, delta: float = 0.0) -> ba_ref.GNStep:
    """One GN step with the prior in S, b and the cost (``system`` holds all three)."""
    w = np.ones(s.obs_cam.size) if w is None else w
    if prior is None:
        return wr.gn_step(st, s, lam, w, delta)
    # the system first, the solve behind the prior: without it S may be singular (no fixed pose)
    out: dict = {}
    with wr._weighted_linearisation(np.asarray(w, dtype=np.float64), delta, out):
        sys0 = ba_ref.build_system(st, s, lam)
    Sa, ba, e = prior_terms(st, s, prior)
    sys_ = dataclasses.replace(sys0, S=sys0.S + Sa, b=sys0.b + ba, cost=out["rho"] + e)
    dc = ba_ref.solve_reduced(sys_.S, sys_.b)
    dp = ba_ref.back_substitute(sys_, s, dc)
    return ba_ref.GNStep(sys_, dc, dp, ba_ref.apply_update(st, s, dc, dp))


def solve(st, s, iters: int, lam: float, prior: Prior | None, w=None, delta: float = 0.0):
    """``iters`` GN steps, all accepted -> (state, costs[iters + 1])."""
    costs = []
    for _ in range(iters):
        step = gn_step(st, s, lam, prior, w, delta)
        costs.append(step.system.cost)
        st = step.state
    costs.append(cost(st, s, prior, w, delta))
    return st, np.array(costs)


def solve_lm(st, s, iters: int, prior: Prior | None, lam0: float, w=None, delta: float = 0.0, up: float = lmr.UP,
             down: float = lmr.DOWN, lam_min: float = lmr.LAM_MIN, lam_max: float = lmr.LAM_MAX) -> lmr.LMLog:
    """``ba_lm_ref.solve``'s loop over the step and cost with the prior."""
    lam = float(min(max(lam0 if lam0 > 0 else lmr.LAM0_DEFAULT, lam_min), lam_max))
    c = cost(st, s, prior, w, delta)
    cs, lams, trial, acc = [], [], [], []
    for _ in range(iters):
        cs.append(c)
        lams.append(lam)
        cand = gn_step(st, s, lam, prior, w, delta).state
        t = cost(cand, s, prior, w, delta)
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


def marginalize(st, s, n_drop: int, prior: Prior | None = None, w=None, delta: float = 0.0, lam: float = 0.0):
    """The prior a slide by ``n_drop`` cameras leaves, at state ``st`` -> (Prior | None over the
    remaining free poses it touches, K, mask (L,) of the landmarks marginalised, info (6R,6R), rhs (6R)).

    D = cameras ``0 .. n_drop-1``; P_D = the landmarks with an active observation in D.  Marginalised
    are all active observations of P_D's landmarks (weights and Huber scale as the linearisation
    applies them) and the old prior in full; eliminated are P_D's landmarks (the oracle's 3x3 route:
    a frozen landmark leaves the system) and the ``m = max(0, n_drop - n_fixed)`` leading free poses,
    ``lam`` on the eliminated blocks only.  ``cost0`` is the marginalised factors' cost at ``st`` (the
    old prior's included), so the new prior's xi is 0 there."""
    w = np.ones(s.obs_cam.size) if w is None else np.asarray(w, dtype=np.float64)
    active = w > 0
    in_d = active & (s.obs_cam < n_drop)
    mask = np.zeros(s.n_points, bool)
    mask[s.obs_pt[in_d]] = True
    wm = np.where(mask[s.obs_pt], w, 0.0)  # the marginalised factors: the rest contribute by select
    # the masked linearisation: points eliminated with lam on their blocks, none on the cameras yet
    step_sys = _masked_system(st, s, wm, delta, lam)
    S, b, c0 = step_sys.S.copy(), step_sys.b.copy(), step_sys.cost
    if prior is not None:
        Sa, ba, e = prior_terms(st, s, prior)
        S, b, c0 = S + Sa, b + ba, c0 + e
    m = 6 * max(0, n_drop - s.n_fixed)
    if m:
        See = S[:m, :m] + lam * np.eye(m)
        L = np.linalg.cholesky(See)  # raises LinAlgError when an eliminated block is not SPD
        Y = np.linalg.solve(L, S[:m, m:])
        y = np.linalg.solve(L, b[:m])
        info = S[m:, m:] - Y.T @ Y
        rhs = b[m:] - Y.T @ y
    else:
        info, rhs = S, b
    info = 0.5 * (info + info.T)
    nz = np.nonzero(np.abs(info).reshape(info.shape[0] // 6, 6, -1).max(axis=(1, 2)) > 0)[0] if info.size else []
    k = int(nz[-1]) + 1 if len(nz) else 0
    r0 = s.n_fixed + m // 6  # the first remaining free camera
    poses0 = st.poses_cw()[r0:r0 + k]
    pr = Prior(info[:6 * k, :6 * k].copy(), rhs[:6 * k].copy(), poses0, c0) if k else None
    return pr, k, mask, info, rhs


def _masked_system(st, s, wm, delta: float, lam: float) -> ba_ref.GNSystem:
    """The oracle's reduced system under weights ``wm`` with ``lam`` on the landmark blocks only."""
    out: dict = {}
    with wr._weighted_linearisation(wm, delta, out):
        sys_ = ba_ref.build_system(st, s, lam)
    n = sys_.S.shape[0]
    return dataclasses.replace(sys_, S=sys_.S - lam * np.eye(n), cost=out["rho"])


def reduced_window(p, st, n_drop: int, mask: np.ndarray):
    """The next window of a slide: cameras ``n_drop ..`` and the landmarks outside ``mask`` ->
    (BAStructure, BAState, kept landmark indices)."""
    keep_pt = np.nonzero(~mask)[0]
    obs_pt = np.repeat(np.arange(p.point_ptr.size - 1), np.diff(p.point_ptr))
    keep_obs = ~mask[obs_pt]
    assert (p.obs_cam[keep_obs] >= n_drop).all(), "a kept landmark is seen from a dropped camera"
    ptr = np.zeros(keep_pt.size + 1, dtype=np.int32)
    remap = -np.ones(mask.size, dtype=np.int64)
    remap[keep_pt] = np.arange(keep_pt.size)
    ptr[1:] = np.cumsum(np.bincount(remap[obs_pt[keep_obs]], minlength=keep_pt.size))
    s2 = ba_ref.BAStructure(p.K, ptr, np.ascontiguousarray(p.obs_cam[keep_obs] - n_drop),
                            np.ascontiguousarray(p.obs_uv[keep_obs]), max(0, p.n_fixed - n_drop), p.n_poses - n_drop)
    st2 = ba_ref.BAState(st.R[n_drop:].copy(), st.t[n_drop:].copy(), st.X[keep_pt].copy())
    return s2, st2, keep_pt


def slide_identity(st, s, n_drop: int, prior: Prior | None = None):
    """The marginalisation identity at lambda = 0: one GN step of the full window against one of the
    reduced window under the prior ``marginalize`` gives at the same state -> (max |dc_full(remaining)
    - dc_reduced| / max |dc|, the full step, new prior, K, mask, info, reduced structure and state)."""
    full = gn_step(st, s, 0.0, prior)
    new, k, mask, info, _ = marginalize(st, s, n_drop, prior)
    s2, st2, _ = reduced_window(s, st, n_drop, mask)
    red = gn_step(st2, s2, 0.0, new)
    m = 6 * max(0, n_drop - s.n_fixed)
    return np.abs(full.dc[m:] - red.dc).max() / np.abs(full.dc).max(), full, new, k, mask, info, s2, st2
