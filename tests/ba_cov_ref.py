"""CPU restatement of the BA covariance read-out (``vo_ba_covariance``).

Test infrastructure, built on ``oracle/ba_ref.py`` (and ``tests/ba_robust_ref.py`` for the Huber
scale).  Two routes to the same numbers:

* Route A, the definition the library follows: ``ba_ref.build_system(st, s, lam)`` gives the
  reduced camera system S, the landmark inverses ``Vinv``, ``W`` and ``valid``;
  ``Sigma_cc = S^-1`` by Cholesky, and per landmark
  ``Sigma_pp = Vinv + T Sigma_cc T^T`` with ``T`` (3 x 6F) holding, in the columns of free camera
  f, the sum over the landmark's observations o in f of ``(W_o Vinv)^T``.  A frozen landmark
  (``valid`` false) is NaN.
* Route B, independent and for small problems: the dense inverse of the full ``J^T J + lam I``
  with J built as ``ba_ref.full_system_step`` builds it; its pose block and its 3x3 landmark
  blocks.  (It has no frozen-landmark rule: compare non-frozen problems only.)

All values are for unit pixel variance.
"""

from __future__ import annotations

import numpy as np
import scipy.linalg

from oracle import ba_ref
from tests import ba_robust_ref as rr

# (n_poses, n_points, seed, make_ba_problem keywords): the inputs whose routes agree to <= 1e-9
INPUTS = {
    "tiny": (5, 60, 7, {}),
    "small": (8, 300, 21, {}),
    "mid": (12, 600, 3, {}),
    "narrow": (16, 400, 5, {"max_track": 4}),  # F = 14, row span 3: entries outside S's band
}


def _system(st, s, lam: float, delta: float) -> ba_ref.GNSystem:
    if delta <= 0:
        return ba_ref.build_system(st, s, lam)
    out: dict = {}
    with rr._scaled_linearisation(delta, out):
        return ba_ref.build_system(st, s, lam)


def route_a(st: ba_ref.BAState, s: ba_ref.BAStructure, lam: float = 0.0, delta: float = 0.0):
    """(Sigma_cc (6F,6F), Sigma_pp (L,3,3)); raises ``LinAlgError`` when S is not positive definite."""
    sys_ = _system(st, s, lam, delta)
    n = 6 * s.n_free
    if n:
        c = scipy.linalg.cho_factor(sys_.S, lower=True)
        cc = scipy.linalg.cho_solve(c, np.eye(n))
        cc = 0.5 * (cc + cc.T)
    else:
        cc = np.zeros((0, 0))
    L = s.n_points
    T = np.zeros((L, 3, n))
    Y = np.einsum("mij,mjk->mik", sys_.W, sys_.Vinv[s.obs_pt])  # W V^-1 (M,6,3)
    for o in np.nonzero(s.obs_cam >= s.n_fixed)[0]:
        f = s.obs_cam[o] - s.n_fixed
        T[s.obs_pt[o], :, 6 * f : 6 * f + 6] += Y[o].T
    pp = sys_.Vinv + np.einsum("lia,ab,ljb->lij", T, cc, T)
    pp = 0.5 * (pp + pp.transpose(0, 2, 1))
    pp[~sys_.valid] = np.nan
    return cc, pp


def route_b(st: ba_ref.BAState, s: ba_ref.BAStructure, lam: float = 0.0, delta: float = 0.0):
    """The same from the dense inverse of the full normal matrix (no landmark is frozen here)."""
    r, pc = ba_ref.residuals(st, s)
    Jc, Jp = ba_ref.jacobians(st, s, pc)
    if delta > 0:
        sc = rr.huber_scale(r, delta)[0]
        Jc, Jp = Jc * sc[:, None, None], Jp * sc[:, None, None]
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
    cc = Hi[: 6 * NF, : 6 * NF]
    idx = 6 * NF + 3 * np.arange(L)[:, None] + np.arange(3)[None, :]
    pp = Hi[idx[:, :, None], idx[:, None, :]]
    return cc, pp


def rel_err(A: np.ndarray, B: np.ndarray) -> float:
    """max_ij |A_ij - B_ij| / sqrt(B_ii B_jj) over the last two axes (one matrix, or a stack of
    blocks, each scaled by its own diagonal); NaN blocks of B must be NaN in A and are left out."""
    A, B = np.asarray(A, float), np.asarray(B, float)
    if B.size == 0:
        return 0.0
    if B.ndim == 3:
        nan = np.isnan(B).any(axis=(1, 2))
        assert np.isnan(A[nan]).all(), "a frozen landmark's block must be NaN"
        A, B = A[~nan], B[~nan]
        if B.size == 0:
            return 0.0
    d = np.sqrt(np.diagonal(B, axis1=-2, axis2=-1))
    return float((np.abs(A - B) / (d[..., :, None] * d[..., None, :])).max())


def routes_disagreement(st, s, lam: float, delta: float = 0.0):
    """(eps_ref, route A's result): the disagreement of the two routes, poses and landmarks."""
    cc_a, pp_a = route_a(st, s, lam, delta)
    cc_b, pp_b = route_b(st, s, lam, delta)
    assert not np.isnan(pp_a).any(), "route B has no frozen landmarks: use a problem without them"
    return max(rel_err(cc_a, cc_b), rel_err(pp_a, pp_b)), (cc_a, pp_a)


def degenerate_problem(p, duplicate: bool):
    """``tests/test_gpu_ba.py::test_degenerate_landmarks_frozen``'s construction on problem p:
    landmark 0 cut to its first observation, landmark 2 moved to the fixed cameras 0 / 1, and
    (``duplicate``) landmark 1's first observation doubled, 0.5 px apart -> (point_ptr, cam, uv)."""
    pp, cam, uv = np.array(p.point_ptr), p.obs_cam.copy(), p.obs_uv.copy()
    keep = np.ones(cam.size, bool)
    keep[pp[0] + 1 : pp[1]] = False
    counts = np.diff(pp)
    counts[0] = 1
    cam2, uv2 = cam[keep], uv[keep]
    if duplicate:
        cam2 = np.insert(cam2, 1, cam[pp[1]])
        uv2 = np.insert(uv2, 1, uv[pp[1]] + 0.5, axis=0)
        counts[1] += 1
    ptr2 = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    cam2[ptr2[2] : ptr2[3]] = np.arange(ptr2[3] - ptr2[2]) % 2
    return ptr2, cam2.astype(np.int32), uv2.astype(np.float32)


WIDE = (50, 400, 11)  # make_ba_problem arguments of wide_problem


def wide_problem():
    """A window whose reduced system has a block row span of 46 of its F = 48 rows, so that one
    block column of the factorisation has more than 256 rows below its diagonal block:
    ``make_ba_problem(*WIDE)`` with the last observation of up to 12 landmarks that start at one of
    the first two free cameras moved to one of the last three cameras (where the landmark lies in
    front of it; the measurement is its projection at the initial guess)
    -> (problem, obs_cam, obs_uv).  Usable at lambda = 1 only: at lambda = 0 the routes of this
    50-pose chain disagree by 9e-8."""
    from visualodometry_amd.synthetic import make_ba_problem

    n = WIDE[0]
    p = make_ba_problem(*WIDE)
    cam, uv, pp = p.obs_cam.copy(), p.obs_uv.copy(), p.point_ptr
    R, t = p.poses_cw[:, :3, :3], p.poses_cw[:, :3, 3]
    moved = 0
    for q in range(p.n_points):
        o0, o1 = pp[q], pp[q + 1]
        if not p.n_fixed <= cam[o0] <= p.n_fixed + 1:
            continue
        for c in range(n - 1, n - 4, -1):
            pc = R[c] @ p.points[q] + t[c]
            if pc[2] > 1.0:
                u = p.K[0, 0] * pc[0] / pc[2] + p.K[0, 2]
                v = p.K[1, 1] * pc[1] / pc[2] + p.K[1, 2]
                if abs(u) < 5000 and abs(v) < 5000:
                    cam[o1 - 1], uv[o1 - 1] = c, (u, v)
                    moved += 1
                    break
        if moved >= 12:
            break
    assert moved > 0
    return p, cam, uv
