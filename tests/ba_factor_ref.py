"""CPU restatement of the BA's pose factors (DESIGN.md §Pose factors, ``vo_ba_setup_factors`` in
include/vo_hip.h).

Test infrastructure on ``oracle/ba_ref.py`` in the style of ``tests/ba_prior_ref.py``, which it
imports: the oracle's linearisation, Schur complement, solve, back substitution and update are used
as they are, the prior's terms as ``ba_prior_ref`` restates them.  Restated here is only what the
factors add.

Model: a factor on window cameras ``(i, j)`` (``j`` -1: unary) with measurement ``Z`` (4,4) and
information ``Lambda`` (6,6).  With ``A = T_i T_j^-1`` (``A = T_i`` for a unary one), the residual is
the twist ``xi = log(A Z^-1)`` (``ba_prior_ref.se3_log``), the cost gains ``xi^T Lambda xi``, and with
the first-order expansion ``xi' ~ xi + delta_i - G delta_j``, ``G = Ad(A)``, the reduced system gains

    S_ii += Lambda,  S_jj += G^T Lambda G,  S_ij += -Lambda G,  b_i += -Lambda xi,  b_j += G^T Lambda xi

over the free cameras only.
"""

from __future__ import annotations

import dataclasses

import numpy as np

from oracle import ba_ref
from tests import ba_lm_ref as lmr
from tests import ba_prior_ref as pr
from tests import ba_weight_ref as wr


@dataclasses.dataclass
class Factor:
    cam_i: int
    cam_j: int  # -1: unary
    meas: np.ndarray  # (4,4) Z
    info: np.ndarray  # (6,6) Lambda, symmetric


def relative(st: ba_ref.BAState, f: Factor):
    """(R_A, t_A): A = T_i T_j^-1, or T_i for a unary factor."""
    Ri, ti = st.R[f.cam_i], st.t[f.cam_i]
    if f.cam_j < 0:
        return Ri, ti
    R = Ri @ st.R[f.cam_j].T
    return R, ti - R @ st.t[f.cam_j]


def adjoint(R: np.ndarray, t: np.ndarray) -> np.ndarray:
    """Ad(A) in (rho, phi) order."""
    G = np.zeros((6, 6))
    G[:3, :3] = G[3:, 3:] = R
    G[:3, 3:] = ba_ref.skew(t) @ R
    return G


def residual(st: ba_ref.BAState, f: Factor) -> np.ndarray:
    """xi = log(A Z^-1)."""
    R, t = relative(st, f)
    Rz, tz = f.meas[:3, :3], f.meas[:3, 3]
    D = R @ Rz.T
    return pr.se3_log(D, t - D @ tz)


def factors_cost(st, factors) -> float:
    return float(sum(residual(st, f) @ f.info @ residual(st, f) for f in factors))


def factor_terms(st, s, factors, n_drop: int = 0):
    """(S_add (6F,6F), b_add (6F), cost) at ``st``, in factor order.  ``n_drop`` > 0: only the
    factors with a camera among ``0 .. n_drop-1`` (the marginalisation's mask rule)."""
    n, nf = 6 * s.n_free, s.n_fixed
    S, b, e = np.zeros((n, n)), np.zeros(n), 0.0
    for f in factors:
        if n_drop > 0 and not (f.cam_i < n_drop or 0 <= f.cam_j < n_drop):
            continue
        xi = residual(st, f)
        L = 0.5 * (f.info + f.info.T)
        e += float(xi @ L @ xi)
        fi, fj = f.cam_i - nf, (f.cam_j - nf if f.cam_j >= 0 else -1)
        a = slice(6 * fi, 6 * fi + 6)
        if fi >= 0:
            S[a, a] += L
            b[a] -= L @ xi
        if fj >= 0:
            G = adjoint(*relative(st, f))
            c = slice(6 * fj, 6 * fj + 6)
            S[c, c] += G.T @ L @ G
            b[c] += G.T @ L @ xi
            if fi >= 0:
                S[a, c] -= L @ G
                S[c, a] -= (L @ G).T
    return S, b, e


def cost(st, s, factors, prior: pr.Prior | None = None, w=None, delta: float = 0.0) -> float:
    return pr.cost(st, s, prior, w, delta) + factors_cost(st, factors)


def gn_step(st, s, lam: float, factors, prior: pr.Prior | None = None, w=None, delta: float = 0.0) -> ba_ref.GNStep:
    """One GN step with the factors (and the prior) in S, b and the cost."""
    w = np.ones(s.obs_cam.size) if w is None else w
    out: dict = {}
    with wr._weighted_linearisation(np.asarray(w, dtype=np.float64), delta, out):
        sys0 = ba_ref.build_system(st, s, lam)
    S, b, e = sys0.S.copy(), sys0.b.copy(), out["rho"]
    Sf, bf, ef = factor_terms(st, s, factors)
    S, b, e = S + Sf, b + bf, e + ef
    if prior is not None:
        Sa, ba, ep = pr.prior_terms(st, s, prior)
        S, b, e = S + Sa, b + ba, e + ep
    sys_ = dataclasses.replace(sys0, S=S, b=b, cost=e)
    dc = ba_ref.solve_reduced(sys_.S, sys_.b)
    dp = ba_ref.back_substitute(sys_, s, dc)
    return ba_ref.GNStep(sys_, dc, dp, ba_ref.apply_update(st, s, dc, dp))


def solve(st, s, iters: int, lam: float, factors, prior=None, w=None, delta: float = 0.0):
    """``iters`` GN steps, all accepted -> (state, costs[iters + 1])."""
    costs = []
    for _ in range(iters):
        step = gn_step(st, s, lam, factors, prior, w, delta)
        costs.append(step.system.cost)
        st = step.state
    costs.append(cost(st, s, factors, prior, w, delta))
    return st, np.array(costs)


def solve_lm(st, s, iters: int, factors, lam0: float, prior=None, w=None, delta: float = 0.0, up: float = lmr.UP,
             down: float = lmr.DOWN, lam_min: float = lmr.LAM_MIN, lam_max: float = lmr.LAM_MAX) -> lmr.LMLog:
    """``ba_lm_ref.solve``'s loop over the step and cost with the factors."""
    lam = float(min(max(lam0 if lam0 > 0 else lmr.LAM0_DEFAULT, lam_min), lam_max))
    c = cost(st, s, factors, prior, w, delta)
    cs, lams, trial, acc = [], [], [], []
    for _ in range(iters):
        cs.append(c)
        lams.append(lam)
        cand = gn_step(st, s, lam, factors, prior, w, delta).state
        t = cost(cand, s, factors, prior, w, delta)
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


def marginalize(st, s, n_drop: int, factors, prior: pr.Prior | None = None, w=None, delta: float = 0.0,
                lam: float = 0.0):
    """``ba_prior_ref.marginalize`` with the factor rule: a factor with an endpoint among the dropped
    cameras enters the masked system and ``cost0``; every other factor is left out.  Returns what
    ``ba_prior_ref.marginalize`` returns."""
    w = np.ones(s.obs_cam.size) if w is None else np.asarray(w, dtype=np.float64)
    in_d = (w > 0) & (s.obs_cam < n_drop)
    mask = np.zeros(s.n_points, bool)
    mask[s.obs_pt[in_d]] = True
    wm = np.where(mask[s.obs_pt], w, 0.0)
    sys_ = pr._masked_system(st, s, wm, delta, lam)
    S, b, c0 = sys_.S.copy(), sys_.b.copy(), sys_.cost
    Sf, bf, ef = factor_terms(st, s, factors, n_drop)
    S, b, c0 = S + Sf, b + bf, c0 + ef
    if prior is not None:
        Sa, ba, e = pr.prior_terms(st, s, prior)
        S, b, c0 = S + Sa, b + ba, c0 + e
    m = 6 * max(0, n_drop - s.n_fixed)
    if m:
        L = np.linalg.cholesky(S[:m, :m] + lam * np.eye(m))
        Y = np.linalg.solve(L, S[:m, m:])
        y = np.linalg.solve(L, b[:m])
        info = S[m:, m:] - Y.T @ Y
        rhs = b[m:] - Y.T @ y
    else:
        info, rhs = S, b
    info = 0.5 * (info + info.T)
    nz = np.nonzero(np.abs(info).reshape(info.shape[0] // 6, 6, -1).max(axis=(1, 2)) > 0)[0] if info.size else []
    k = int(nz[-1]) + 1 if len(nz) else 0
    r0 = s.n_fixed + m // 6
    new = pr.Prior(info[:6 * k, :6 * k].copy(), rhs[:6 * k].copy(), st.poses_cw()[r0:r0 + k], c0) if k else None
    return new, k, mask, info, rhs


def remaining(factors, n_drop: int):
    """The factors a slide by ``n_drop`` keeps, re-indexed: those with no camera among the dropped."""
    return [Factor(f.cam_i - n_drop, f.cam_j - n_drop if f.cam_j >= 0 else -1, f.meas, f.info)
            for f in factors if not (f.cam_i < n_drop or 0 <= f.cam_j < n_drop)]


def slide_identity(st, s, n_drop: int, factors, prior: pr.Prior | None = None):
    """The marginalisation identity at lambda = 0 with factors: one GN step of the full window
    against one of the reduced window under the prior ``marginalize`` gives and the remaining
    factors -> (max |dc_full(remaining) - dc_reduced| / max |dc|, full step, new prior, K, mask, info,
    reduced structure, state and factors)."""
    full = gn_step(st, s, 0.0, factors, prior)
    new, k, mask, info, _ = marginalize(st, s, n_drop, factors, prior)
    s2, st2, _ = pr.reduced_window(s, st, n_drop, mask)
    f2 = remaining(factors, n_drop)
    red = gn_step(st2, s2, 0.0, f2, new)
    m = 6 * max(0, n_drop - s.n_fixed)
    return np.abs(full.dc[m:] - red.dc).max() / np.abs(full.dc).max(), full, new, k, mask, info, s2, st2, f2


def twist_pose(d: np.ndarray, T: np.ndarray) -> np.ndarray:
    """exp(d^) T as a (4,4) pose."""
    R, t = ba_ref.se3_exp(np.asarray(d, dtype=np.float64))
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = R, t
    return E @ T


def make_factors(poses_cw: np.ndarray, pairs, seed: int = 0, noise: float = 1e-2, info_scale: float = 1.0):
    """Factors on ``pairs`` (``(i, j)``, ``j`` -1 for a unary one) whose measurements are the true
    relative poses of ``poses_cw`` perturbed by a twist of about ``noise``, with random SPD Lambda."""
    rng = np.random.default_rng(seed)
    out = []
    for i, j in pairs:
        A = poses_cw[i] @ np.linalg.inv(poses_cw[j]) if j >= 0 else poses_cw[i]
        M = rng.normal(size=(6, 6))
        out.append(Factor(int(i), int(j), twist_pose(noise * rng.normal(size=6), A), info_scale * (M.T @ M + np.eye(6))))
    return out
