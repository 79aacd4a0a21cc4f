"""Essential-matrix initialisation on the MI355X (reference ``src/modules/vo.py:87-101``).

:func:`findEssentialMat` and :func:`recoverPose` have the call signatures and return values of
``cv2.findEssentialMat`` / ``cv2.recoverPose`` as the reference's initialisation branch uses
them: ``findEssentialMat(uv_ref, uv_curr, K, method=RANSAC, prob=..., threshold=...) -> (E,
mask (n,1) uint8)`` and ``recoverPose(E, uv_ref, uv_curr, K) -> (good, R, t (3,1), mask (n,1)
uint8 of 0/255)``.  Five-point RANSAC over OpenCV's subsets with its loop bookkeeping, Sampson
scoring and the cheirality vote run in ``vo_essential_ransac`` / ``vo_recover_pose``
(``csrc/essential.hip``); the behaviour they are checked against is DESIGN.md §Essential,
restated in ``tests/essential_ref.py``.  Fails loudly without the HIP library (no CPU
fallback).  Only what the reference uses is accepted: RANSAC, no distortion, no input mask.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, ptr

RANSAC = 8  # cv2.RANSAC
DISTANCE_THRESH = 50.0  # cv2.recoverPose's default distanceThresh


def _points(p1, p2):
    a = np.ascontiguousarray(np.asarray(p1, dtype=np.float32).reshape(-1, 2))
    b = np.ascontiguousarray(np.asarray(p2, dtype=np.float32).reshape(-1, 2))
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"{a.shape[0]} points in the first image but {b.shape[0]} in the second")
    return a, b


def _camera(K):
    return np.ascontiguousarray(np.asarray(K, dtype=np.float64).reshape(3, 3))


def find_essential_ransac(p1, p2, K, threshold: float = 1.0, prob: float = 0.999, max_iters: int = 1000,
                          ctx: _lib.Context | None = None):
    """-> (ok bool, E (3,3) of unit Frobenius norm, inlier mask (n,) bool)."""
    a, b = _points(p1, p2)
    ctx = ctx or _lib.context()
    n = a.shape[0]
    E = np.zeros(9)
    mask = np.zeros(max(n, 1), dtype=np.uint8)
    ok, inl = C.c_int32(0), C.c_int32(0)
    check(ctx.lib.vo_essential_ransac(ctx.handle, ptr(a, C.c_float), ptr(b, C.c_float), n, ptr(_camera(K), C.c_double),
                                      int(max_iters), float(threshold), float(prob), ptr(E, C.c_double),
                                      ptr(mask, C.c_uint8), C.byref(ok), C.byref(inl)), "vo_essential_ransac")
    return bool(ok.value), E.reshape(3, 3), mask[:n].astype(bool)


def recover_pose(E, p1, p2, K, ctx: _lib.Context | None = None):
    """-> (good int, R (3,3), t (3,) unit, mask (n,) bool) with ``X2 = R X1 + t``."""
    a, b = _points(p1, p2)
    ctx = ctx or _lib.context()
    n = a.shape[0]
    Em = np.ascontiguousarray(np.asarray(E, dtype=np.float64).reshape(9))
    R, t = np.zeros(9), np.zeros(3)
    mask = np.zeros(max(n, 1), dtype=np.uint8)
    good = C.c_int32(0)
    check(ctx.lib.vo_recover_pose(ctx.handle, ptr(Em, C.c_double), ptr(a, C.c_float), ptr(b, C.c_float), n,
                                  ptr(_camera(K), C.c_double), DISTANCE_THRESH, ptr(R, C.c_double),
                                  ptr(t, C.c_double), ptr(mask, C.c_uint8), C.byref(good)), "vo_recover_pose")
    return int(good.value), R.reshape(3, 3), t, mask[:n].astype(bool)


def findEssentialMat(points1, points2, cameraMatrix=None, method=RANSAC, prob=0.999, threshold=1.0, *args,
                     ctx: _lib.Context | None = None, **kw):
    """Drop-in for ``cv2.findEssentialMat`` in the reference's initialisation (``vo.py:87-93``):
    ``(E (3,3), mask (n,1) uint8)``, or ``(None, None)`` when no model was found."""
    if args or kw:
        raise ValueError(f"findEssentialMat (MI355X): unsupported arguments {list(kw) or len(args)} "
                         "(distortion, maxIters and an input mask are not supported)")
    if cameraMatrix is None or np.ndim(cameraMatrix) != 2:
        raise ValueError("findEssentialMat (MI355X): a 3x3 cameraMatrix is required")
    if method != RANSAC:
        raise ValueError("findEssentialMat (MI355X): only method=RANSAC")
    ok, E, mask = find_essential_ransac(points1, points2, cameraMatrix, threshold, prob, ctx=ctx)
    if not ok:
        return None, None
    return E, mask.astype(np.uint8).reshape(-1, 1)


def recoverPose(E, points1, points2, cameraMatrix=None, *args, ctx: _lib.Context | None = None, **kw):
    """Drop-in for ``cv2.recoverPose`` in the reference's initialisation (``vo.py:95-101``):
    ``(good, R (3,3), t (3,1), mask (n,1) uint8 of 0/255)``."""
    if args or kw:
        raise ValueError(f"recoverPose (MI355X): unsupported arguments {list(kw) or len(args)} "
                         "(distortion, distanceThresh and an input mask are not supported)")
    if cameraMatrix is None or np.ndim(cameraMatrix) != 2:
        raise ValueError("recoverPose (MI355X): a 3x3 cameraMatrix is required")
    good, R, t, mask = recover_pose(E, points1, points2, cameraMatrix, ctx)
    return good, R, t.reshape(3, 1), (mask.astype(np.uint8) * 255).reshape(-1, 1)
