"""Steered BRIEF descriptors on the MI355X (``vo_brief_describe``, ``csrc/brief.hip``).

:func:`describe` gives a point a 256-bit descriptor of the 31 x 31 patch around it, turned to the
patch's intensity-centroid direction: ORB's structure, not its bits.  It is what the corners of
:func:`visualodometry_amd.corners.good_features` are matched by
(:func:`visualodometry_amd.matcher.match_hamming`) once their tracks have broken.  The arithmetic
is ``include/vo_hip.h``'s and DESIGN.md §BRIEF's, restated in ``tests/brief_ref.py``: integers
throughout, defined to the bit.  Fails loudly without the HIP library (no CPU fallback).
"""

from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import check
from .klt import _gray, _points

BINS, TESTS, WORDS = 32, 256, 8


def pattern():
    """-> ``(P int8 (32, 256, 4), C int32 (32,), S int32 (32,))``: the rotated tests ``(px, py, qx, qy)``
    of every bin and the direction tables (``vo_brief_pattern``; needs no device)."""
    P = np.zeros((BINS, TESTS, 4), np.int8)
    d = np.zeros(2 * BINS, np.int32)
    check(_lib.load().vo_brief_pattern(P.ctypes.data, d.ctypes.data), "vo_brief_pattern")
    return P, d[:BINS].copy(), d[BINS:].copy()


def describe(img, pts, tag: int = 0, ctx: _lib.Context | None = None, shape=None):
    """-> ``(des uint32 (n, 8), bins int32 (n,), status uint8 (n,))`` of the points ``pts`` (n, 2) of the
    2-D uint8 ``img``.  ``status`` 1 marks a point that is not finite or rounds to a pixel outside
    the image: its descriptor is zero.  A nonzero ``tag`` names the image's pixels as in
    :func:`visualodometry_amd.klt.track`: once that call has cached the pyramid, ``img`` may be
    ``None`` (with ``shape`` = (h, w))."""
    p = _points(pts, "pts")
    n = len(p)
    if img is None:
        if not tag or shape is None:
            raise ValueError("img is None without a tag and a shape")
        im, (h, w) = None, (int(shape[0]), int(shape[1]))
    else:
        im = _gray(img, "img")
        h, w = im.shape
    des = np.zeros((max(n, 1), WORDS), np.uint32)
    bins = np.zeros(max(n, 1), np.int32)
    status = np.zeros(max(n, 1), np.uint8)
    lib = _lib.load() if n == 0 and ctx is None else None  # no point, no device
    handle = None
    if lib is None:
        ctx = ctx or _lib.context()
        lib, handle = ctx.lib, ctx.handle
    check(lib.vo_brief_describe(handle, None if im is None else im.ctypes.data, int(tag), h, w,
                                p.ctypes.data if n else None, n, 0, des.ctypes.data, bins.ctypes.data,
                                status.ctypes.data), "vo_brief_describe")
    return des[:n], bins[:n], status[:n]


def unpack(des) -> np.ndarray:
    """Binary rows uint32 ``(n, words)`` -> float32 ``(n, 32 words)`` of 0 / 1, bit ``t`` of a row in
    column ``t``: rows whose squared L2 distance is the Hamming distance."""
    d = np.ascontiguousarray(des, np.uint32)
    if d.ndim != 2:
        raise ValueError(f"binary descriptors must be (N, words), got shape {d.shape}")
    shifts = np.arange(32, dtype=np.uint32)
    return ((d[:, :, None] >> shifts) & np.uint32(1)).reshape(len(d), -1).astype(np.float32)
