"""Sparse pyramidal Lucas-Kanade tracking on the MI355X (``vo_klt_track``, ``csrc/klt.hip``).

:func:`track` follows keypoints from one image into the next; between two keyframes that is all
the VO loop needs from detection and matching (reference ``src/modules/vo.py:64-66``).  The
arithmetic is DESIGN.md §KLT, restated in ``tests/klt_ref.py``: the structure of OpenCV's
``calcOpticalFlowPyrLK`` with fixed-point patches, defined to the bit.  Fails loudly without the
HIP library (no CPU fallback).
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, ptr

# status codes of vo_klt_track
TRACKED, START_OUTSIDE, DEGENERATE, LEFT_IMAGE, FB_FAILED, ERR_ABOVE, BAD_INPUT = range(7)
STATUS_NAMES = ("tracked", "start window outside", "degenerate texture", "left the image",
                "forward-backward check failed", "err above max_err", "bad input")


def _gray(img, name: str) -> np.ndarray:
    a = np.asarray(img)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError(f"{name} must be a 2-D uint8 image, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def _points(p, name: str) -> np.ndarray:
    a = np.asarray(p, dtype=np.float32)
    if a.ndim == 3 and a.shape[1] == 1:  # cv2's (N, 1, 2)
        a = a[:, 0]
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"{name} must be (N, 2), got {a.shape}")
    return np.ascontiguousarray(a)


def layout(h: int, w: int, levels: int, win_radius: int):
    """-> (L_eff, bytes, [(h, w, offset) per level]) of the pyramid ``vo_klt_track`` builds (host only)."""
    out = np.zeros(2 + 3 * 8, np.int64)
    n = check(_lib.load().vo_klt_layout(int(h), int(w), int(levels), int(win_radius), ptr(out, C.c_int64), out.size),
              "vo_klt_layout")
    L = int(out[0])
    assert n == 2 + 3 * L
    return L, int(out[1]), [tuple(int(v) for v in out[2 + 3 * l:5 + 3 * l]) for l in range(L)]


def pyramid(img, levels: int = 4, win_radius: int = 10, ctx: _lib.Context | None = None) -> list:
    """The ``L_eff`` uint8 levels the tracker uses for ``img`` (parity / debug)."""
    im = _gray(img, "img")
    L, nbytes, lv = layout(im.shape[0], im.shape[1], levels, win_radius)
    ctx = ctx or _lib.context()
    out = np.zeros(nbytes, np.uint8)
    got = C.c_int32(0)
    check(ctx.lib.vo_klt_pyramid(ctx.handle, im.ctypes.data, im.shape[0], im.shape[1], L, out.ctypes.data, out.size,
                                 C.byref(got)), "vo_klt_pyramid")
    assert got.value == L
    return [out[o:o + h * w].reshape(h, w) for h, w, o in lv]


def track(img0, img1, pts0, guess=None, win_radius: int = 10, levels: int = 4, max_iters: int = 30,
          eps: float = 0.01, min_eig: float = 1e-4, fb_thresh: float | None = None, max_err: float | None = None,
          tags=(0, 0), ctx: _lib.Context | None = None):
    """Tracks ``pts0`` (N, 2) from ``img0`` into ``img1`` -> ``(pts1 (N, 2) float32, status (N,) uint8,
    err (N,) float32)``.  ``status`` 0 is a tracked point (:data:`STATUS_NAMES`); a failed point keeps
    ``pts0`` and err 0.  ``guess`` (N, 2) starts the search elsewhere than at ``pts0``;
    ``fb_thresh`` switches the forward-backward check on; ``max_err`` > 0 rejects by the mean absolute
    patch difference.  A nonzero tag in ``tags`` names its image's pixels: the device pyramid is kept
    under that tag and the image may then be ``None`` on later calls."""
    p0 = _points(pts0, "pts0")
    n = p0.shape[0]
    ims = [None if im is None else _gray(im, f"img{k}") for k, im in enumerate((img0, img1))]
    shapes = {im.shape for im in ims if im is not None}
    if len(shapes) > 1:
        raise ValueError(f"img0 and img1 differ in shape: {sorted(shapes)}")
    tags = tuple(int(t) for t in tags)
    for k in range(2):
        if ims[k] is None and tags[k] == 0:
            raise ValueError(f"img{k} is None without a tag")
    if not shapes:
        raise ValueError("at least one image is needed for the shape")
    h, w = next(iter(shapes))
    flags = 0
    p1 = np.zeros((max(n, 1), 2), np.float32)
    if guess is not None:
        g = _points(guess, "guess")
        if g.shape != p0.shape:
            raise ValueError(f"guess has {g.shape[0]} rows for {n} points")
        p1[:n] = g
        flags |= _lib.VO_KLT_GUESS
    if fb_thresh is not None:
        flags |= _lib.VO_KLT_FB
    opt = _lib.KltOptionsC(win_radius=int(win_radius), levels=int(levels), max_iters=int(max_iters), eps=float(eps),
                           min_eig=float(min_eig), fb_thresh=float(fb_thresh or 0.0), max_err=float(max_err or 0.0),
                           flags=flags, reserved=0)
    status = np.zeros(max(n, 1), np.uint8)
    err = np.zeros(max(n, 1), np.float32)
    good = C.c_int32(0)
    ctx = ctx or _lib.context()
    check(ctx.lib.vo_klt_track(ctx.handle, None if ims[0] is None else ims[0].ctypes.data, tags[0],
                               None if ims[1] is None else ims[1].ctypes.data, tags[1], h, w, p0.ctypes.data,
                               p1.ctypes.data, n, C.byref(opt), status.ctypes.data, err.ctypes.data, C.byref(good)),
          "vo_klt_track")
    return p1[:n], status[:n], err[:n]


# cv2.TERM_CRITERIA_COUNT | cv2.TERM_CRITERIA_EPS, 30 iterations, eps 0.01: calcOpticalFlowPyrLK's default
_DEFAULT_CRITERIA = (3, 30, 0.01)
OPTFLOW_USE_INITIAL_FLOW = 4  # cv2.OPTFLOW_USE_INITIAL_FLOW


def calcOpticalFlowPyrLK(prevImg, nextImg, prevPts, nextPts=None, winSize=(21, 21), maxLevel=3,
                         criteria=_DEFAULT_CRITERIA, flags=0, minEigThreshold=1e-4,
                         ctx: _lib.Context | None = None):
    """``cv2.calcOpticalFlowPyrLK``'s call: ``(nextPts (N, 1, 2) float32, status (N, 1) uint8 with 1 = found,
    err (N, 1) float32)``.  It has OpenCV's structure, not its bits: the arithmetic is this project's
    (DESIGN.md §KLT), so positions agree with cv2's to a fraction of a pixel, not to the last place.
    Only square odd windows up to 31 and the ``OPTFLOW_USE_INITIAL_FLOW`` flag are accepted."""
    if winSize[0] != winSize[1] or winSize[0] % 2 != 1 or not 3 <= winSize[0] <= 31:
        raise ValueError(f"calcOpticalFlowPyrLK (MI355X): winSize {winSize} is not a square odd window of 3..31")
    if flags & ~OPTFLOW_USE_INITIAL_FLOW:
        raise ValueError(f"calcOpticalFlowPyrLK (MI355X): unsupported flags {flags}")
    kind, count, eps = criteria
    max_iters = min(max(int(count), 1), 100) if kind & 1 else 30
    eps = float(eps) if kind & 2 else 0.0
    guess = nextPts if flags & OPTFLOW_USE_INITIAL_FLOW else None
    if flags & OPTFLOW_USE_INITIAL_FLOW and nextPts is None:
        raise ValueError("calcOpticalFlowPyrLK (MI355X): OPTFLOW_USE_INITIAL_FLOW without nextPts")
    p1, status, err = track(prevImg, nextImg, prevPts, guess, win_radius=winSize[0] // 2, levels=int(maxLevel) + 1,
                            max_iters=max_iters, eps=eps, min_eig=float(minEigThreshold), ctx=ctx)
    return p1.reshape(-1, 1, 2), (status == TRACKED).astype(np.uint8).reshape(-1, 1), err.reshape(-1, 1)
