"""Sliding-window bundle adjustment on MI355X (Gauss-Newton with Schur complement).

The reference has no BA: ``pyceres``/``pycolmap`` are declared
(``pyproject.toml:11-12``) but never imported, and pose comes only from
``cv2.solvePnPRansac`` (``src/modules/vo.py:135-141``).  This module is the
build-defined BA API of SURVEY.md §8b, meant to be called from the keyframe
hook ``VisualOdometry._create_keyframe`` (``src/modules/vo.py:252-288``):

    ba = SlidingWindowBA(K, cfg)
    result = ba.optimize(window)        # never raises on a degenerate window

Model (identical to ``oracle/ba_ref.py``): residual ``pi(K (R_cw X + t_cw)) - uv``
with the no-distortion pinhole of ``frontend.py:139``, cost ``sum ||r||^2``,
left se(3) pose increments, the first ``n_fixed`` poses fixed, pure GN.

Robust cost (off by default): ``huber=delta`` in pixels replaces ``||r||^2`` by the Huber
``rho`` (``||r||^2`` up to ``delta``, ``2 delta ||r|| - delta^2`` beyond) and scales each
observation's residual and Jacobians by ``sqrt(delta / ||r||)`` in the linearisation
(first-order IRLS; ``tests/ba_robust_ref.py`` restates it on the oracle); every reported cost is
then ``sum rho``.  ``residuals()`` / ``optimize(..., return_residuals=True)`` give the raw squared
reprojection error and depth per observation, so a caller can drop the tracks the solve ended
up disagreeing with.

Step control (off by default): ``lm=True`` (or ``cfg.ba_lm``) runs ``vo_ba_run_lm`` instead of the
fixed-damping ``vo_ba_run``: each step is tried, kept only if the cost went down, and the damping
is adapted (x0.1 / x10), all on the device; ``lam`` is then the starting damping.  It guarantees a
non-increasing cost, not a smaller error against ground truth (``tests/ba_lm_ref.py`` restates the
loop on the oracle).  ``lm_ftol`` / ``lm_xtol`` / ``lm_max_rejects`` (``cfg.ba_lm_*``) end the loop
on the device once it has converged or keeps rejecting (``vo_ba_set_lm_stop``;
``tests/ba_lm_stop_ref.py``); ``BAResult.lm_trials`` / ``lm_stop`` say how it ended.

Covariance (off by default): ``BASession.covariance()`` / ``optimize(..., return_covariance=True)``
(or ``cfg.ba_covariance``) read out the covariance of the free poses and of every landmark at the
device state (``vo_ba_covariance``: the dense inverse of the reduced camera system and the 3x3
landmark blocks, for unit pixel variance; ``tests/ba_cov_ref.py`` restates it on the oracle).  The
weakly constrained, low-parallax landmarks are the ones with a huge variance; no culling policy
is built on it.

Observation weights and culling (off by default): ``BAWindow.obs_weight`` /
``BASession.set_obs_weights`` give every observation an information weight (1 / sigma^2; 0: it does
not count), applied as ``sqrt(w)`` on the residual and Jacobians ahead of the Huber rule.
``BASession.cull`` / ``cull_async`` deactivate, on the device and without a new setup, the
observations with ``w * err2 > max_chi2``, a depth at or below ``min_depth`` or a non-finite
residual, then the tracks left shorter than ``min_track``.  ``cull_rounds = R`` (``cfg.ba_cull_rounds``,
with ``ba_cull_chi2`` / ``ba_cull_min_depth``) makes ``optimize`` run ``R + 1`` solves with a cull
between them; ``BAResult.obs_active`` says what survived (``tests/ba_weight_ref.py`` restates both on
the oracle).

Pose prior (off by default): ``BAWindow.prior`` / ``BASession(..., prior=PosePrior(...))`` add a
quadratic cost ``cost0 - 2 eta^T xi + xi^T Lambda xi`` on the leading free poses, ``xi`` the se(3)
log of each pose against its linearisation pose (``vo_ba_setup_prior``) -- the form in which what
left a sliding window stays in its cost; the solve honours it in every linearisation and every
reported cost (``tests/ba_prior_ref.py`` restates it on the oracle).  ``BASession.marginalize(n)`` /
``optimize(..., marginalize=n)`` compute that prior on the device for the window's first ``n``
cameras (``vo_ba_marginalize``): ``BAResult.prior`` and ``BAResult.point_marginalised``.

Pose factors (off by default): ``BAWindow.factors`` / ``BASession(..., factors=[PoseFactor(...)])`` add
6x6 costs ``xi^T info xi`` on one camera (``cam_j`` -1: ``xi = log(T_i Z^-1)``) or between two
(``xi = log(T_i T_j^-1 Z^-1)``), e.g. the front end's relative motion, an odometry increment or a soft
anchor (``vo_ba_setup_factors``; ``tests/ba_factor_ref.py`` restates them on the oracle).  They enter
every linearisation, every reported cost and the covariance; ``marginalize`` folds the factors that
touch a dropped camera into the prior, and the caller passes the others on, re-indexed.
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import (BACullOptionsC, BALmOptionsC, BALmStopC, BAPoseFactorC, BAPosePriorC, BAProblemC, C, VoError, check,
                   ptr)


@dataclass
class PosePrior:
    """A quadratic cost on the leading ``K`` free poses of a window (``vo_ba_pose_prior``):
    ``cost0 - 2 rhs^T xi + xi^T info xi``, with ``xi`` (6K) the stacked se(3) logs ``(rho, phi)`` of
    ``T_f T0_f^-1`` against the linearisation poses ``poses0``."""

    info: np.ndarray  # (6K,6K) Lambda, symmetric (the lower triangle is read)
    rhs: np.ndarray  # (6K,) eta
    poses0: np.ndarray  # (K,4,4) linearisation poses, world -> camera
    cost0: float = 0.0

    @property
    def n_poses(self) -> int:
        return int(np.asarray(self.poses0).shape[0])


@dataclass
class PoseFactor:
    """A 6x6 cost on window cameras (``vo_ba_pose_factor``): ``xi^T info xi`` with
    ``xi = log(A meas^-1)`` in twist order ``(rho, phi)``; ``A = T_i T_j^-1`` for a between factor,
    ``A = T_i`` for a unary one (``cam_j`` -1); ``T`` world -> camera."""

    cam_i: int
    cam_j: int  # a second window camera, or -1
    meas: np.ndarray  # (4,4) the measured A
    info: np.ndarray  # (6,6) Lambda, symmetric (the lower triangle is read)


@dataclass
class BAWindow:
    """Keyframe window handed to :meth:`SlidingWindowBA.optimize`.

    ``obs_pt`` gives the landmark of each observation in any order; it is
    grouped by landmark (CSR) before the C-ABI call.
    """

    poses_cw: np.ndarray  # (N,4,4) float64, world -> camera
    points: np.ndarray  # (L,3) float64
    obs_uv: np.ndarray  # (M,2) float32 pixels
    obs_cam: np.ndarray  # (M,) int
    obs_pt: np.ndarray  # (M,) int
    n_fixed: int = 2
    # (M,) information weights (1 / sigma^2, px^-2) in the window's own observation order, 0 for an
    # observation that does not count; None: all ones
    obs_weight: np.ndarray | None = None
    # a quadratic cost on the leading free poses (cameras n_fixed .. n_fixed + K - 1); None: none
    prior: PosePrior | None = None
    # pose factors on the window's cameras; None: none
    factors: list | None = None


@dataclass
class BAResult:
    poses_cw: np.ndarray
    points: np.ndarray
    cost_per_iter: np.ndarray = field(default_factory=lambda: np.zeros(0))
    status: str = "ok"  # "ok" | "not_spd" | "skipped"
    message: str = ""
    # optimize(return_residuals=True): raw squared reprojection error (px^2) and camera-frame
    # depth per observation at the returned state, in the window's own observation order
    obs_err2: np.ndarray | None = None
    obs_depth: np.ndarray | None = None
    # step control (lm=True): the damping before each trial and after the last, and each trial's
    # verdict; cost_per_iter then holds the accepted-state costs
    lambdas: np.ndarray | None = None
    accepted: np.ndarray | None = None
    # how the LM loop ended (None without lm): the trials that ran, and "ran_all", or the
    # termination criterion that stopped it: "ftol", "xtol", "rejects"
    lm_trials: int | None = None
    lm_stop: str | None = None
    # optimize(return_covariance=True): the Gauss-Newton covariance at the returned state for unit
    # pixel variance -- pose_cov (F,6,6) over the free poses' left twists (rho, phi), point_cov
    # (L,3,3) in the window's landmark order (NaN for a frozen landmark) -- and cov_sigma2, the
    # variance estimate to scale both by: final cost / max(1, 2M - 6F - 3 (non-frozen landmarks)).
    # None when not asked for, or when the reduced system was not positive definite.
    pose_cov: np.ndarray | None = None
    point_cov: np.ndarray | None = None
    cov_sigma2: float | None = None
    # culling (cull_rounds > 0): which observations were still active after the last solve, in the
    # window's own observation order; cost_per_iter then concatenates the parts' costs
    obs_active: np.ndarray | None = None
    # optimize(marginalize=n): the prior that dropping the first n cameras leaves at the returned
    # state (None when it touches no remaining pose, or when the elimination was not positive
    # definite) and the (L,) bool mask of the landmarks it absorbed, in the window's landmark order
    prior: PosePrior | None = None
    point_marginalised: np.ndarray | None = None


def poses_to_rt(poses_cw: np.ndarray) -> np.ndarray:
    """(N,4,4) -> (N,12) = R row-major, t (the C-ABI pose layout)."""
    P = np.asarray(poses_cw, dtype=np.float64)
    out = np.empty((P.shape[0], 12))
    out[:, :9] = P[:, :3, :3].reshape(-1, 9)
    out[:, 9:] = P[:, :3, 3]
    return out


def rt_to_poses(rt: np.ndarray) -> np.ndarray:
    T = np.tile(np.eye(4), (rt.shape[0], 1, 1))
    T[:, :3, :3] = rt[:, :9].reshape(-1, 3, 3)
    T[:, :3, 3] = rt[:, 9:]
    return T


def _as_index32(obs_pt) -> np.ndarray:
    """obs_pt as contiguous int32, checked in its own (wider) type first: an int64 index of
    2^31 or more, or a large negative one, must not wrap into [0, n_points)."""
    a = np.asarray(obs_pt).reshape(-1)
    if a.dtype != np.int32 and a.size:
        if not np.issubdtype(a.dtype, np.integer):
            raise ValueError("obs_pt must be integer")
        if int(a.min()) < 0 or int(a.max()) > np.iinfo(np.int32).max:
            raise ValueError("obs_pt out of range")
    return np.ascontiguousarray(a, dtype=np.int32)


def csr_from_obs_pt(n_points: int, obs_pt: np.ndarray):
    """Stable grouping of observations by landmark -> (order, point_ptr)
    (``vo_ba_group_by_point``: one counting sort on the host)."""
    obs_pt = _as_index32(obs_pt)
    order = np.empty(obs_pt.size, dtype=np.int32)
    ptr_ = np.empty(int(n_points) + 1, dtype=np.int32)
    rc = _lib.load().vo_ba_group_by_point(int(n_points), obs_pt.size, ptr(obs_pt, C.c_int32),
                                          ptr(order, C.c_int32), ptr(ptr_, C.c_int32))
    if rc != _lib.VO_OK:
        raise ValueError("obs_pt out of range")
    return order, ptr_


def group_window(n_points: int, window: "BAWindow", return_order: bool = False):
    """The window's observations grouped by landmark -> (point_ptr, obs_cam, obs_uv).
    Windows built landmark by landmark (dropin/hooks.py ``KeyframeWindow.build``) are
    already grouped: their arrays pass through unchanged; others are reordered by
    ``csr_from_obs_pt``.  ``return_order``: also the reordering (grouped position -> window
    observation), ``None`` when the arrays passed through."""
    obs_pt = _as_index32(window.obs_pt)
    obs_cam = np.asarray(window.obs_cam)
    obs_uv = np.asarray(window.obs_uv, dtype=np.float32).reshape(-1, 2)
    point_ptr = np.empty(int(n_points) + 1, dtype=np.int32)
    # order == NULL: one pass that checks the grouping and fills point_ptr
    rc = _lib.load().vo_ba_group_by_point(int(n_points), obs_pt.size, ptr(obs_pt, C.c_int32), None,
                                          ptr(point_ptr, C.c_int32))
    if rc == _lib.VO_OK:
        return (point_ptr, obs_cam, obs_uv, None) if return_order else (point_ptr, obs_cam, obs_uv)
    if rc != 1:
        raise ValueError("obs_pt out of range")
    order, point_ptr = csr_from_obs_pt(n_points, obs_pt)
    if return_order:
        return point_ptr, obs_cam[order], obs_uv[order], order
    return point_ptr, obs_cam[order], obs_uv[order]


def _problem_struct(K, point_ptr, obs_cam, obs_uv, n_poses, n_fixed, lam):
    K = np.asarray(K, dtype=np.float64)
    prob = BAProblemC()
    prob.n_poses = int(n_poses)
    prob.n_points = point_ptr.size - 1
    prob.n_obs = obs_cam.size
    prob.n_fixed = int(n_fixed)
    prob.fx, prob.fy, prob.cx, prob.cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    prob.lam = float(lam)
    prob.point_ptr = ptr(point_ptr, C.c_int32)
    prob.obs_cam = ptr(obs_cam, C.c_int32)
    prob.obs_uv = ptr(obs_uv, C.c_float)
    return prob


def _prior_struct(prior: PosePrior):
    """``(vo_ba_pose_prior, the arrays it points into)``; shapes are checked here, before the
    library reads past a short array."""
    poses0 = np.asarray(prior.poses0, dtype=np.float64)
    if poses0.ndim != 3 or poses0.shape[1:] != (4, 4):
        raise ValueError("PosePrior.poses0 must be (K,4,4)")
    k = poses0.shape[0]
    info = np.ascontiguousarray(prior.info, dtype=np.float64)
    rhs = np.ascontiguousarray(prior.rhs, dtype=np.float64).reshape(-1)
    if info.shape != (6 * k, 6 * k) or rhs.size != 6 * k:
        raise ValueError("PosePrior: info must be (6K,6K) and rhs (6K,) for poses0 (K,4,4)")
    rt = np.ascontiguousarray(poses_to_rt(poses0))
    pc = BAPosePriorC(k, 0, ptr(info, C.c_double), ptr(rhs, C.c_double), ptr(rt, C.c_double), float(prior.cost0))
    return pc, (info, rhs, rt)


def _factor_array(factors):
    """``(vo_ba_pose_factor[n], n)``; shapes are checked here, before the library reads a short array."""
    factors = list(factors)
    arr = (BAPoseFactorC * max(1, len(factors)))()
    for k, f in enumerate(factors):
        meas = np.asarray(f.meas, dtype=np.float64)
        info = np.asarray(f.info, dtype=np.float64)
        if meas.shape != (4, 4) or info.shape != (6, 6):
            raise ValueError("PoseFactor: meas must be (4,4) and info (6,6)")
        arr[k].cam_i, arr[k].cam_j = int(f.cam_i), int(f.cam_j)
        arr[k].meas[:] = poses_to_rt(meas[None])[0].tolist()
        arr[k].info[:] = info.reshape(-1).tolist()
    return arr, len(factors)


def plan_probe(K, point_ptr, obs_cam, obs_uv, n_poses: int, n_fixed: int = 2,
               target_segments: int = 512) -> dict:
    """Host-only static plan statistics (no device needed): ``vo_ba_plan_probe``."""
    point_ptr = np.ascontiguousarray(point_ptr, dtype=np.int32)
    obs_cam = np.ascontiguousarray(obs_cam, dtype=np.int32)
    obs_uv = np.ascontiguousarray(obs_uv, dtype=np.float32).reshape(-1, 2)
    prob = _problem_struct(K, point_ptr, obs_cam, obs_uv, n_poses, n_fixed, 0.0)
    out = np.zeros(14, dtype=np.int64)
    n = check(_lib.load().vo_ba_plan_probe(C.byref(prob), int(target_segments),
                                           ptr(out, C.c_int64), 14), "vo_ba_plan_probe")
    keys = ["chunks", "segments", "slab_blocks", "profile_blocks", "track_entries",
            "max_chunk_pairs", "max_segment_slots", "max_segment_cameras", "free_poses",
            "max_row_span", "band_solver", "band_top_rows", "band_separator_rows", "band_bottom_rows"]
    return dict(zip(keys[:n], out[:n].tolist()))


def plan_digest(K, point_ptr, obs_cam, obs_uv, n_poses: int, n_fixed: int = 2, target_segments: int = 512) -> int:
    """Host-only 64-bit digest of the whole static plan (``vo_ba_plan_digest``): pins the
    planner's output, and with it every kernel's summation order."""
    point_ptr = np.ascontiguousarray(point_ptr, dtype=np.int32)
    obs_cam = np.ascontiguousarray(obs_cam, dtype=np.int32)
    obs_uv = np.ascontiguousarray(obs_uv, dtype=np.float32).reshape(-1, 2)
    prob = _problem_struct(K, point_ptr, obs_cam, obs_uv, n_poses, n_fixed, 0.0)
    d = C.c_uint64(0)
    check(_lib.load().vo_ba_plan_digest(C.byref(prob), int(target_segments), C.byref(d)), "vo_ba_plan_digest")
    return int(d.value)


def plan_slide_digest(K, prev, cur, seg_obs: int, seg_chunks: int = 1) -> tuple:
    """Host-only (test): ``(digest, reused_chunks)`` of the plan of window ``cur`` packed for
    ``seg_obs`` observations per segment (1: the one-wave K1's plan of ``seg_chunks`` chunks per
    segment), built from scratch (``prev`` None) or by taking over
    the unchanged first-camera groups of ``prev``'s plan, as ``vo_ba_setup`` does on a slide
    (``vo_ba_testing_plan_slide``).  Windows: ``(point_ptr, obs_cam, obs_uv, n_poses, n_fixed)``."""
    keep = []

    def struct(w):
        pp, oc, uv, n, nf = w
        a = (np.ascontiguousarray(pp, dtype=np.int32), np.ascontiguousarray(oc, dtype=np.int32),
             np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2))
        keep.append(a)
        return _problem_struct(K, a[0], a[1], a[2], n, nf, 0.0)

    pc = struct(cur)
    pv = struct(prev) if prev is not None else None
    d = C.c_uint64(0)
    r = C.c_int64(0)
    check(_lib.load().vo_ba_testing_plan_slide(C.byref(pv) if pv is not None else None, C.byref(pc), int(seg_obs),
                                               int(seg_chunks), C.byref(d), C.byref(r)), "vo_ba_testing_plan_slide")
    return int(d.value), int(r.value)


class BASession:
    """A BA problem resident on one device (structure + state in HBM).

    Thin wrapper of the ``vo_ba_*`` C-ABI: ``setup`` uploads the structure and
    builds the static plan, ``set_state``/``get_state`` move poses and points,
    ``run`` performs GN iterations on the device-resident state.
    """

    def __init__(self, K, point_ptr, obs_cam, obs_uv, n_poses: int, n_fixed: int = 2,
                 lam: float = 0.0, ctx: _lib.Context | None = None, huber: float = 0.0,
                 prior: PosePrior | None = None, factors=None):
        self.ctx = ctx or _lib.context()
        self.point_ptr = np.ascontiguousarray(point_ptr, dtype=np.int32)
        self.obs_cam = np.ascontiguousarray(obs_cam, dtype=np.int32)
        self.obs_uv = np.ascontiguousarray(obs_uv, dtype=np.float32).reshape(-1, 2)
        self.n_poses = int(n_poses)
        self.n_points = self.point_ptr.size - 1
        self.n_fixed = int(n_fixed)
        prob = _problem_struct(K, self.point_ptr, self.obs_cam, self.obs_uv, self.n_poses,
                               self.n_fixed, lam)
        self._prob = prob
        sid = C.c_uint64(0)
        self.prior = prior
        self.factors = list(factors) if factors is not None else None
        if self.factors:
            pc, keep = _prior_struct(prior) if prior is not None else (None, None)
            fa, n = _factor_array(self.factors)
            check(self.ctx.lib.vo_ba_setup_factors(self.ctx.handle, C.byref(prob), C.byref(pc) if pc is not None else None,
                                                   fa, n, C.byref(sid)), "vo_ba_setup_factors")
            del keep, fa  # (the library copied the arrays)
        elif prior is None:
            check(self.ctx.lib.vo_ba_setup(self.ctx.handle, C.byref(prob), C.byref(sid)), "vo_ba_setup")
        else:
            pc, keep = _prior_struct(prior)
            check(self.ctx.lib.vo_ba_setup_prior(self.ctx.handle, C.byref(prob), C.byref(pc), C.byref(sid)),
                  "vo_ba_setup_prior")
            del keep  # (the library copied the arrays)
        # the problem's id on this context: a later setup on the same context (another
        # session) makes every call below fail with VO_ERR_STATE instead of misreading
        self.session = int(sid.value)
        if huber:  # a new problem starts with the plain cost
            self.set_robust(huber)

    def set_robust(self, delta: float) -> None:
        """Huber ``delta`` in pixels for the later linearisations; 0 is the plain cost."""
        check(self.ctx.lib.vo_ba_set_robust(self.ctx.handle, self.session, float(delta)), "vo_ba_set_robust")

    def residuals(self):
        """``(err2, depth)`` per observation in the order of ``obs_cam``: the raw (unweighted)
        squared reprojection error and the camera-frame depth at the device state."""
        err2 = np.empty(self.obs_cam.size)
        depth = np.empty(self.obs_cam.size)
        check(self.ctx.lib.vo_ba_residuals(self.ctx.handle, self.session, ptr(err2, C.c_double),
                                           ptr(depth, C.c_double)), "vo_ba_residuals")
        return err2, depth

    def set_obs_weights(self, w) -> None:
        """Information weights (1 / sigma^2, px^-2) per observation in the order of ``obs_cam``
        (``vo_ba_set_obs_weights``); 0 deactivates an observation, ``None`` restores all ones."""
        if w is None:
            check(self.ctx.lib.vo_ba_set_obs_weights(self.ctx.handle, self.session, None), "vo_ba_set_obs_weights")
            return
        w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
        if w.size != self.obs_cam.size:
            raise ValueError("one weight per observation expected")
        check(self.ctx.lib.vo_ba_set_obs_weights(self.ctx.handle, self.session, ptr(w, C.c_double)),
              "vo_ba_set_obs_weights")

    def obs_weights(self) -> np.ndarray:
        """Synchronises; the current weights in the order of ``obs_cam``, culled observations at 0."""
        w = np.empty(self.obs_cam.size)
        check(self.ctx.lib.vo_ba_get_obs_weights(self.ctx.handle, self.session, ptr(w, C.c_double)),
              "vo_ba_get_obs_weights")
        return w

    def cull(self, max_chi2: float = 0.0, min_depth: float = 0.0, min_track: int = 2):
        """Deactivates, on the device and at the device state, every active observation with
        ``w * err2 > max_chi2`` (``max_chi2`` 0: not tested), depth ``<= min_depth`` or a non-finite
        residual, then what is left of every track shorter than ``min_track`` (``vo_ba_cull``);
        returns ``(n_culled, n_active)``."""
        opt = BACullOptionsC(float(max_chi2), float(min_depth), int(min_track), 0)
        culled, active = C.c_int32(0), C.c_int32(0)
        check(self.ctx.lib.vo_ba_cull(self.ctx.handle, self.session, C.byref(opt), C.byref(culled), C.byref(active)),
              "vo_ba_cull")
        return int(culled.value), int(active.value)

    def cull_async(self, max_chi2: float = 0.0, min_depth: float = 0.0, min_track: int = 2) -> None:
        """:meth:`cull` enqueued on the context stream without a host synchronisation; its outcome
        is read with :meth:`obs_weights`."""
        opt = BACullOptionsC(float(max_chi2), float(min_depth), int(min_track), 0)
        check(self.ctx.lib.vo_ba_cull_async(self.ctx.handle, self.session, C.byref(opt)), "vo_ba_cull_async")

    def covariance(self, lam: float = 0.0, dense: bool = False):
        """``(pose_cov (F,6,6), point_cov (L,3,3))`` at the device state for unit pixel variance
        (``vo_ba_covariance``; the caller scales by its sigma^2), plus the dense ``(6F,6F)`` pose
        covariance when ``dense``.  ``lam`` is the damping of this linearisation (0: the
        Gauss-Newton covariance).  A frozen landmark's block is NaN.  Raises ``VoError`` with
        ``code == VO_ERR_NOT_SPD`` when the reduced camera system is not positive definite (the
        session stays usable)."""
        F = self.n_poses - self.n_fixed
        pose = np.empty((F, 6, 6))
        pts = np.empty((self.n_points, 3, 3))
        full = np.empty((6 * F, 6 * F)) if dense else None
        rc = self.ctx.lib.vo_ba_covariance(self.ctx.handle, self.session, float(lam), ptr(pose, C.c_double),
                                           ptr(full, C.c_double) if dense else None, ptr(pts, C.c_double))
        check(rc, "vo_ba_covariance")
        return (pose, pts, full) if dense else (pose, pts)

    def marginalize(self, n_drop: int, lam: float = 0.0):
        """``(PosePrior | None, point_mask)``: the prior that dropping the window's first ``n_drop``
        cameras leaves at the device state (``vo_ba_marginalize``) -- over the next window's leading
        free poses, ``None`` when it touches none -- and the (L,) bool mask of the landmarks it
        absorbed, which the next window leaves out.  ``lam`` damps the eliminated blocks only.
        Raises ``VoError`` with ``code == VO_ERR_NOT_SPD`` when an eliminated pose block is not
        positive definite (the session stays usable)."""
        r = (self.n_poses - self.n_fixed) - max(0, int(n_drop) - self.n_fixed)
        info = np.empty((6 * max(r, 0), 6 * max(r, 0)))
        rhs = np.empty(6 * max(r, 0))
        poses0 = np.empty((max(r, 0), 12))
        cost0, k = C.c_double(0.0), C.c_int32(0)
        mask = np.zeros(max(self.n_points, 1), dtype=np.uint8)
        check(self.ctx.lib.vo_ba_marginalize(self.ctx.handle, self.session, int(n_drop), float(lam), C.byref(k),
                                             ptr(info, C.c_double), ptr(rhs, C.c_double), ptr(poses0, C.c_double),
                                             C.byref(cost0), ptr(mask, C.c_uint8)), "vo_ba_marginalize")
        k = int(k.value)
        mask = mask[:self.n_points].astype(bool)
        if k == 0:
            return None, mask
        return PosePrior(info[:6 * k, :6 * k].copy(), rhs[:6 * k].copy(), rt_to_poses(poses0[:k]), float(cost0.value)), mask

    def set_state(self, poses_cw: np.ndarray, points: np.ndarray) -> None:
        rt = np.ascontiguousarray(poses_to_rt(poses_cw))
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        if rt.shape[0] != self.n_poses or pts.shape[0] != self.n_points:
            raise ValueError("state shape does not match the problem")
        check(self.ctx.lib.vo_ba_set_state(self.ctx.handle, self.session, ptr(rt, C.c_double),
                                           ptr(pts, C.c_double)),
              "vo_ba_set_state")

    def get_state(self):
        rt = np.empty((self.n_poses, 12))
        pts = np.empty((self.n_points, 3))
        check(self.ctx.lib.vo_ba_get_state(self.ctx.handle, self.session, ptr(rt, C.c_double),
                                           ptr(pts, C.c_double)),
              "vo_ba_get_state")
        return rt_to_poses(rt), pts

    def run(self, iters: int):
        """``iters`` GN iterations; returns (status_code, costs[iters+1])."""
        costs = np.empty(iters + 1)
        rc = self.ctx.lib.vo_ba_run(self.ctx.handle, self.session, int(iters), ptr(costs, C.c_double))
        if rc not in (_lib.VO_OK, _lib.VO_ERR_NOT_SPD):
            check(rc, "vo_ba_run")
        return rc, costs

    @staticmethod
    def _lm_options(lam0, up, down, lam_min, lam_max) -> BALmOptionsC:
        return BALmOptionsC(float(lam0), float(up), float(down), float(lam_min), float(lam_max))

    def _lm_buffers(self, n: int):
        n = max(n, 0)  # (a negative count is the library's to refuse)
        return np.empty(n + 1), np.empty(n + 1), np.empty(n), np.empty(n, dtype=np.uint8)

    def run_lm(self, iters: int, lam0: float = 0.0, up: float = 0.0, down: float = 0.0, lam_min: float = 0.0,
               lam_max: float = 0.0):
        """``iters`` Levenberg-Marquardt trial steps (``vo_ba_run_lm``; a zero option takes the
        library's default); returns ``(status_code, costs[iters+1], lambdas[iters+1], trials[iters],
        accepted[iters])``."""
        costs, lambdas, trials, accepted = self._lm_buffers(int(iters))
        opt = self._lm_options(lam0, up, down, lam_min, lam_max)
        rc = self.ctx.lib.vo_ba_run_lm(self.ctx.handle, self.session, int(iters), C.byref(opt), ptr(costs, C.c_double),
                                       ptr(lambdas, C.c_double), ptr(trials, C.c_double), ptr(accepted, C.c_uint8))
        if rc not in (_lib.VO_OK, _lib.VO_ERR_NOT_SPD):
            check(rc, "vo_ba_run_lm")
        return rc, costs, lambdas, trials, accepted

    def run_lm_async(self, iters: int, lam0: float = 0.0, up: float = 0.0, down: float = 0.0, lam_min: float = 0.0,
                     lam_max: float = 0.0) -> None:
        opt = self._lm_options(lam0, up, down, lam_min, lam_max)
        check(self.ctx.lib.vo_ba_run_lm_async(self.ctx.handle, self.session, int(iters), C.byref(opt)),
              "vo_ba_run_lm_async")

    def lm_log(self, n: int):
        """Synchronises; the first ``n`` iterations of the last ``run_lm`` / ``run_lm_async``'s log, as
        ``run_lm`` returns it."""
        costs, lambdas, trials, accepted = self._lm_buffers(int(n))
        rc = self.ctx.lib.vo_ba_lm_log(self.ctx.handle, self.session, int(n), ptr(costs, C.c_double),
                                       ptr(lambdas, C.c_double), ptr(trials, C.c_double), ptr(accepted, C.c_uint8))
        if rc not in (_lib.VO_OK, _lib.VO_ERR_NOT_SPD):
            check(rc, "vo_ba_lm_log")
        return rc, costs, lambdas, trials, accepted

    def set_lm_stop(self, ftol: float = 0.0, xtol: float = 0.0, max_rejects: int = 0) -> None:
        """Termination criteria of the later ``run_lm`` / ``run_lm_async`` calls (``vo_ba_set_lm_stop``):
        a relative cost decrease of at most ``ftol``, a largest pose-update entry of at most ``xtol``,
        ``max_rejects`` rejections in a row; a zero is not tested, all zero never stops."""
        stop = BALmStopC(float(ftol), float(xtol), int(max_rejects), 0)
        check(self.ctx.lib.vo_ba_set_lm_stop(self.ctx.handle, self.session, C.byref(stop)), "vo_ba_set_lm_stop")

    def lm_stop_info(self):
        """Synchronises; ``(trials, reason)`` of the last LM run: the trials that ran before it
        ended and one of ``_lib.BA_LM_*`` (``vo_ba_lm_stop_info``)."""
        trials, reason = C.c_int32(0), C.c_int32(0)
        check(self.ctx.lib.vo_ba_lm_stop_info(self.ctx.handle, self.session, C.byref(trials), C.byref(reason)),
              "vo_ba_lm_stop_info")
        return int(trials.value), int(reason.value)

    def run_async(self, iters: int) -> None:
        check(self.ctx.lib.vo_ba_run_async(self.ctx.handle, self.session, int(iters)), "vo_ba_run_async")

    def synchronize(self) -> None:
        check(self.ctx.lib.vo_synchronize(self.ctx.handle), "vo_synchronize")

    def gn_step(self):
        """One GN step exporting (rc, S dense, b, dc, cost-before-step)."""
        F = self.n_poses - self.n_fixed
        S = np.empty((6 * F, 6 * F))
        b = np.empty(6 * F)
        dc = np.empty(6 * F)
        cost = np.empty(1)
        rc = self.ctx.lib.vo_ba_gn_step(self.ctx.handle, self.session, ptr(S, C.c_double), ptr(b, C.c_double),
                                           ptr(dc, C.c_double), ptr(cost, C.c_double))
        if rc not in (_lib.VO_OK, _lib.VO_ERR_NOT_SPD):
            check(rc, "vo_ba_gn_step")
        return rc, S, b, dc, float(cost[0])

    SETUP_SECTIONS = ["sync", "order", "segments", "lists_images", "plan_rest", "plan_checks", "images",
                      "profile", "uploads", "buffers", "band_tables", "attributes"]

    def plan_stats(self) -> dict:
        out = np.zeros(24, dtype=np.int64)
        n = check(self.ctx.lib.vo_ba_plan_stats(self.ctx.handle, ptr(out, C.c_int64), 24), "stats")
        keys = ["chunks", "segments", "slab_blocks", "reduced_blocks", "profile_blocks",
                "track_entries", "algorithmic_bytes_per_iter", "band_solver", "reused_groups",
                "reused_chunks", "seg_obs"]
        st = dict(zip(keys[:n], out[:n].tolist()))
        if n > 11:  # the last setup's host sections (ns)
            st["setup_us"] = {k: round(v / 1e3, 1) for k, v in zip(self.SETUP_SECTIONS, out[11:23].tolist())}
        if n > 23:  # the banded K3's layout
            st["band_mode"] = ["none", "full", "ring", "split"][int(out[23])]
        return st


class SlidingWindowBA:
    """``SlidingWindowBA(K, cfg).optimize(window) -> BAResult``.

    ``cfg`` may be a ``VOConfig`` carrying ``ba_iters`` / ``ba_lambda`` / ``ba_huber`` / ``ba_lm`` / ``ba_covariance``; any
    missing knob takes the keyword default.  ``lm`` (``cfg.ba_lm``): Levenberg-Marquardt step
    control on the device, ``lam`` its starting damping, ``lm_ftol`` / ``lm_xtol`` / ``lm_max_rejects``
    (``cfg.ba_lm_ftol`` / ``ba_lm_xtol`` / ``ba_lm_max_rejects``, all 0: off) its termination
    criteria.  Degenerate windows come back with
    ``status != "ok"`` instead of raising, so ``process_frame`` keeps the
    reference's print-and-continue failure style (``vo.py:240-245``).
    """

    def __init__(self, K, cfg=None, *, iters: int = 10, lam: float = 0.0, huber: float = 0.0,
                 device: int | None = None, lm: bool = False, lm_ftol: float = 0.0, lm_xtol: float = 0.0,
                 lm_max_rejects: int = 0, covariance: bool = False, cull_rounds: int = 0, cull_chi2: float = 0.0,
                 cull_min_depth: float = 0.0):
        self.K = np.asarray(K, dtype=np.float64)
        self.iters = int(getattr(cfg, "ba_iters", iters))
        self.lam = float(getattr(cfg, "ba_lambda", lam))
        self.huber = float(getattr(cfg, "ba_huber", huber))  # Huber delta in pixels, 0: off
        # a configuration error must not turn into "every window skipped" (optimize() maps the
        # library's VO_ERR_ARG to a skipped window)
        if not (np.isfinite(self.huber) and self.huber >= 0.0):
            raise ValueError(f"ba_huber must be finite and >= 0, got {self.huber}")
        self.lm = bool(getattr(cfg, "ba_lm", lm))
        # termination of the LM loop (used with lm only); all zero: every trial runs
        self.lm_ftol = float(getattr(cfg, "ba_lm_ftol", lm_ftol))
        self.lm_xtol = float(getattr(cfg, "ba_lm_xtol", lm_xtol))
        self.lm_max_rejects = int(getattr(cfg, "ba_lm_max_rejects", lm_max_rejects))
        if not (0.0 <= self.lm_ftol < 1.0 and np.isfinite(self.lm_xtol) and self.lm_xtol >= 0.0
                and self.lm_max_rejects >= 0):
            raise ValueError("ba_lm_ftol must be in [0, 1), ba_lm_xtol finite and >= 0, ba_lm_max_rejects >= 0")
        # covariance read-out of every optimize() (cfg.ba_covariance); off by default
        self.covariance = bool(getattr(cfg, "ba_covariance", covariance))
        # device-side culling (cfg.ba_cull_*): cull_rounds = R > 0 runs R + 1 solves of `iters` each
        # with a cull between them (w * err2 > cull_chi2, depth <= cull_min_depth, tracks shorter
        # than 2); 0: off
        self.cull_rounds = int(getattr(cfg, "ba_cull_rounds", cull_rounds))
        self.cull_chi2 = float(getattr(cfg, "ba_cull_chi2", cull_chi2))
        self.cull_min_depth = float(getattr(cfg, "ba_cull_min_depth", cull_min_depth))
        if not (self.cull_rounds >= 0 and np.isfinite(self.cull_chi2) and self.cull_chi2 >= 0.0
                and np.isfinite(self.cull_min_depth)):
            raise ValueError("ba_cull_rounds must be >= 0, ba_cull_chi2 finite and >= 0, ba_cull_min_depth finite")
        self.device = device

    def reserve(self, n_poses: int, n_points: int, obs_per_point: float = 5.0, n_fixed: int = 2) -> None:
        """Pre-size the device context for windows of up to about ``n_poses`` keyframes and
        ``n_points`` landmarks (``vo_ba_reserve``), once, before the drive's first keyframe:
        the first :meth:`optimize` then allocates nothing and faults in no page."""
        n_points = max(1, int(n_points))
        n_obs = max(2 * n_points, int(round(obs_per_point * n_points)))
        _lib.ba_reserve(_lib.context(self.device), max(2, int(n_poses)), n_points, n_obs, int(n_fixed))

    def optimize(self, window: BAWindow, return_residuals: bool = False, return_covariance: bool = False,
                 marginalize: int = 0) -> BAResult:
        poses = np.asarray(window.poses_cw, dtype=np.float64)
        pts = np.asarray(window.points, dtype=np.float64).reshape(-1, 3)
        n_fixed = min(int(window.n_fixed), poses.shape[0])
        if poses.shape[0] == 0 or pts.shape[0] == 0 or np.asarray(window.obs_cam).size == 0 \
                or poses.shape[0] <= n_fixed:
            return BAResult(poses.copy(), pts.copy(), np.zeros(0), "skipped", "empty window")
        point_ptr, obs_cam, obs_uv, order = group_window(pts.shape[0], window, return_order=True)
        ctx = _lib.context(self.device)
        err2 = depth = pose_cov = point_cov = sigma2 = new_prior = marg_mask = None
        try:
            sess = BASession(self.K, point_ptr, obs_cam, obs_uv, poses.shape[0], n_fixed, self.lam, ctx,
                             huber=self.huber, prior=window.prior, factors=window.factors)
            sess.set_state(poses, pts)
            if window.obs_weight is not None:
                w = np.asarray(window.obs_weight, dtype=np.float64).reshape(-1)
                if w.size != obs_cam.size:
                    raise ValueError("obs_weight: one weight per observation expected")
                sess.set_obs_weights(w if order is None else w[order])
            lambdas = accepted = lm_trials = lm_stop = active = None
            if self.lm and (self.lm_ftol or self.lm_xtol or self.lm_max_rejects):
                sess.set_lm_stop(self.lm_ftol, self.lm_xtol, self.lm_max_rejects)
            # cull_rounds + 1 solves with a cull between them (one solve without culling)
            parts = []
            for k in range(self.cull_rounds + 1):
                if self.lm:
                    rc, c, lams, _, acc = sess.run_lm(self.iters, lam0=self.lam)
                    trials, reason = sess.lm_stop_info()
                    parts.append((c, lams, acc, trials))
                    lm_stop = _lib.BA_LM_REASONS[reason]
                else:
                    rc, c = sess.run(self.iters)
                    parts.append((c,))
                if rc != _lib.VO_OK or k == self.cull_rounds:
                    break
                sess.cull_async(self.cull_chi2, self.cull_min_depth, 2)
            costs = np.concatenate([q[0] for q in parts])
            if self.lm:
                lambdas = np.concatenate([q[1] for q in parts])
                accepted = np.concatenate([q[2] for q in parts])
                lm_trials = int(sum(q[3] for q in parts))
            if self.cull_rounds > 0:
                active = sess.obs_weights() > 0
                if order is not None:
                    a = np.empty_like(active)
                    a[order] = active
                    active = a
            P, X = sess.get_state()
            if return_residuals:
                err2, depth = sess.residuals()
                if order is not None:  # back from the grouped order to the window's own
                    e, d = np.empty_like(err2), np.empty_like(depth)
                    e[order], d[order] = err2, depth
                    err2, depth = e, d
            if (return_covariance or self.covariance) and rc == _lib.VO_OK:
                # the Gauss-Newton covariance (no damping) at the returned state; landmarks keep
                # the window's own indices (grouping reorders observations only)
                try:
                    pose_cov, point_cov = sess.covariance(0.0)
                    live = int(np.isfinite(point_cov[:, 0, 0]).sum())
                    n_act = obs_cam.size if active is None else int(active.sum())  # culled ones left the system
                    dof = 2 * n_act - 6 * (poses.shape[0] - n_fixed) - 3 * live
                    sigma2 = float(costs[-1]) / max(1, dof)
                except VoError as e:
                    if e.code != _lib.VO_ERR_NOT_SPD:
                        raise
                    pose_cov = point_cov = sigma2 = None
            if marginalize > 0 and rc == _lib.VO_OK:
                # what the next window keeps of its first `marginalize` cameras (landmarks keep the
                # window's own indices).  The solve stands whatever becomes of this: an elimination
                # that is not positive definite, a panel beyond the kernel's LDS (VO_ERR_ARG) or a K1
                # layout without a weighted form (VO_ERR_STATE) all mean "no prior"
                try:
                    new_prior, marg_mask = sess.marginalize(marginalize, self.lam)
                except VoError as e:
                    if e.code not in (_lib.VO_ERR_NOT_SPD, _lib.VO_ERR_ARG, _lib.VO_ERR_STATE):
                        raise
                    new_prior = marg_mask = None
        except VoError as e:
            if e.code == _lib.VO_ERR_ARG:
                return BAResult(poses.copy(), pts.copy(), np.zeros(0), "skipped", str(e))
            raise
        status = "ok" if rc == _lib.VO_OK else "not_spd"
        return BAResult(P, X, costs, status, obs_err2=err2, obs_depth=depth, lambdas=lambdas, accepted=accepted,
                        lm_trials=lm_trials, lm_stop=lm_stop, pose_cov=pose_cov, point_cov=point_cov, cov_sigma2=sigma2,
                        obs_active=active, prior=new_prior, point_marginalised=marg_mask)
