"""Shi-Tomasi corner detection on the MI355X (``vo_good_features``, ``csrc/corners.hip``).

:func:`good_features` finds the pixels where a Lucas-Kanade window is well conditioned (the
minimum-eigenvalue criterion :func:`visualodometry_amd.klt.track` tests), strongest first, at least
``min_distance`` apart and at least that far from a set of existing points: what a KLT front end
replenishes its tracks with.  The arithmetic is DESIGN.md §Corners, restated in
``tests/corners_ref.py``: the structure of OpenCV's ``goodFeaturesToTrack``, defined to the bit.
Fails loudly without the HIP library (no CPU fallback).
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .klt import _gray, _points

MAX_DISTANCE = 1024.0


def _block_radius(block_size: int) -> int:
    if block_size not in (3, 5, 7):
        raise ValueError(f"block_size must be 3, 5 or 7, got {block_size}")
    return int(block_size) // 2


def _keep(keep):
    if keep is None:
        return None, 0
    k = _points(keep, "keep")
    return (k, len(k)) if len(k) else (None, 0)


def response(img, block_size: int = 3, ctx: _lib.Context | None = None) -> np.ndarray:
    """The minimum-eigenvalue response map of ``img``, (h, w) float32 (parity / debug)."""
    im = _gray(img, "img")
    k = _block_radius(block_size)
    out = np.zeros(im.shape, np.float32)
    ctx = ctx or _lib.context()
    check(ctx.lib.vo_corner_response(ctx.handle, im.ctypes.data, im.shape[0], im.shape[1], k, out.ctypes.data),
          "vo_corner_response")
    return out


def good_features(img, max_corners, quality: float = 0.01, min_distance: float = 8.0, mask=None, block_size: int = 3,
                  keep=None, tag: int = 0, ctx: _lib.Context | None = None, shape=None):
    """-> ``(pts (N, 2) float32, resp (N,) float32)``: up to ``max_corners`` (``None``: no limit)
    corners of the 2-D uint8 ``img``, strongest first, at least ``min_distance`` from each other and
    from every finite row of ``keep`` (M, 2).  ``mask`` (h, w) uint8 confines them to its nonzero
    pixels.  A nonzero ``tag`` names the image's pixels as in :func:`visualodometry_amd.klt.track`:
    once that call has cached the pyramid, ``img`` may be ``None`` (with ``shape`` = (h, w))."""
    k = _block_radius(block_size)
    if img is None:
        if not tag or shape is None:
            raise ValueError("img is None without a tag and a shape")
        im, (h, w) = None, (int(shape[0]), int(shape[1]))
    else:
        im = _gray(img, "img")
        h, w = im.shape
    m = None
    if mask is not None:
        m = np.ascontiguousarray(mask)
        if m.dtype == np.bool_:
            m = m.view(np.uint8)
        if m.dtype != np.uint8 or m.shape != (h, w):
            raise ValueError(f"mask must be uint8 {(h, w)}, got {m.dtype} {m.shape}")
    kp, n_keep = _keep(keep)
    limit = h * w if max_corners is None else int(max_corners)
    opt = _lib.CornerOptionsC(max_corners=limit, block_radius=k, quality=float(quality),
                              min_distance=float(min_distance), flags=0, reserved=0)
    cap = max(min(limit, max((h - 2) * (w - 2), 0)), 1)
    pts = np.zeros((cap, 2), np.float32)
    resp = np.zeros(cap, np.float32)
    n = C.c_int32(0)
    ctx = ctx or _lib.context()
    check(ctx.lib.vo_good_features(ctx.handle, None if im is None else im.ctypes.data, int(tag), h, w,
                                   None if m is None else m.ctypes.data, None if kp is None else kp.ctypes.data,
                                   n_keep, C.byref(opt), pts.ctypes.data, resp.ctypes.data, C.byref(n)),
          "vo_good_features")
    return pts[:n.value].copy(), resp[:n.value].copy()


def select(xy, resp, min_distance: float, max_corners=None, keep=None, ctx: _lib.Context | None = None) -> np.ndarray:
    """The selection rule alone: candidates ``xy`` (n, 2) integers taken in the order ``resp``
    descending (ties by row) -> the accepted rows (int64), in order of acceptance."""
    p = np.ascontiguousarray(np.asarray(xy, np.int32).reshape(-1, 2))
    r = np.ascontiguousarray(resp, np.float32).reshape(-1)
    if len(r) != len(p):
        raise ValueError(f"resp has {len(r)} rows for {len(p)} candidates")
    kp, n_keep = _keep(keep)
    limit = max(len(p), 1) if max_corners is None else int(max_corners)
    out = np.zeros(max(min(limit, len(p)), 1), np.int32)
    n = C.c_int32(0)
    ctx = ctx or _lib.context()
    check(ctx.lib.vo_corner_select(ctx.handle, p.ctypes.data, r.ctypes.data, len(p),
                                   None if kp is None else kp.ctypes.data, n_keep, float(min_distance), limit,
                                   out.ctypes.data, C.byref(n)), "vo_corner_select")
    return out[:n.value].astype(np.int64)


def last_stats(ctx: _lib.Context | None = None) -> dict:
    """What the context's last :func:`good_features` / :func:`select` call did (debug)."""
    ctx = ctx or _lib.context()
    out = (C.c_int32 * 4)()
    check(ctx.lib.vo_corner_stats(ctx.handle, out), "vo_corner_stats")
    return dict(candidates=out[0], rounds=out[1], accepted=out[2], cell_side=out[3])


def goodFeaturesToTrack(image, maxCorners, qualityLevel, minDistance, mask=None, blockSize=3,
                        useHarrisDetector=False, k=0.04, ctx: _lib.Context | None = None):
    """``cv2.goodFeaturesToTrack``'s call: corners as (N, 1, 2) float32, strongest first;
    ``maxCorners <= 0`` means no limit.  It has OpenCV's structure, not its bits: the arithmetic is
    this project's (integer Sobel sums, the response in double), so the corners
    agree with cv2's where the responses are well separated, not to the last place.  Only the
    minimum-eigenvalue detector with an odd ``blockSize`` of 3..7 is accepted."""
    if useHarrisDetector:
        raise ValueError("goodFeaturesToTrack (MI355X): the Harris detector is not supported")
    if blockSize % 2 != 1 or not 3 <= blockSize <= 7:
        raise ValueError(f"goodFeaturesToTrack (MI355X): blockSize {blockSize} is not odd and in 3..7")
    pts, _ = good_features(image, None if maxCorners <= 0 else int(maxCorners), float(qualityLevel), float(minDistance),
                           mask=mask, block_size=int(blockSize), ctx=ctx)
    return pts.reshape(-1, 1, 2)
