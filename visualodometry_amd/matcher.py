"""Brute-force descriptor matching on MI355X (knn k=2 + Lowe ratio test).

Drop-in for the SIFT branch of ``FeatureFrontend.match_frames``
(reference ``src/modules/frontend.py:86-111``): the reference calls
``cv2.BFMatcher(cv2.NORM_L2, crossCheck=False).knnMatch(des0, des1, k=2)``
(``:34``, ``:101``) and keeps ``[m.queryIdx, m.trainIdx]`` when
``m.distance < 0.75 * n.distance`` (``:103-109``).  Here both steps run in
``libvo_hip.so`` (``vo_match_knn2_ratio``); see DESIGN.md §Matcher for the
exact semantics and the one documented divergence (no pair passing the test
returns shape ``(0, 2)``, not the reference's ``(0,)``).
"""

from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import C, check, ptr

RATIO_THRESH = 0.75  # frontend.py:104


def _as_des(d) -> np.ndarray:
    if hasattr(d, "detach"):  # torch tensor, possibly on the GPU (frontend.py:92-95)
        d = d.detach().cpu().numpy()
    d = np.asarray(d)
    if d.ndim == 3 and d.shape[0] == 1:  # (1, N, D) feature-dict layout (frontend.py:71)
        d = d[0]
    if d.ndim != 2:
        raise ValueError(f"descriptors must be (N, D), got shape {d.shape}")
    return np.ascontiguousarray(d, dtype=np.float32)


class _QueryTags:
    """Tags for the library's cached query side (``vo_match_knn2_ratio_q`` / ``_dev``).

    A descriptor object gets a tag while it is the cached query: the cache holds a strong
    reference to it, so neither the object nor its memory can be recycled under the same
    identity, and torch tensors carry a version counter that every in-place write bumps.  A
    numpy array has no such counter (a write could go unnoticed), so it is never cached."""

    def __init__(self):
        self.obj, self.version, self.tag, self.next = None, None, 0, 1

    def tag_for(self, d) -> int:
        version = getattr(d, "_version", None)
        if version is None:
            return 0
        if d is not self.obj or version != self.version:
            self.obj, self.version, self.tag = d, version, self.next
            self.next += 1
        return self.tag


def _tensor_2d(d):
    """A torch tensor as its (N, D) float32 contiguous view (the feature dict's (1, N, D))."""
    if d.dim() == 3 and d.shape[0] == 1:
        d = d[0]
    if d.dim() != 2:
        raise ValueError(f"descriptors must be (N, D), got shape {tuple(d.shape)}")
    return d.detach().float().contiguous()


def match_knn2_ratio(des0, des1, ratio: float = RATIO_THRESH, ctx: _lib.Context | None = None,
                     kind: int | None = None, cache_query: bool = False,
                     cross_check: bool = False) -> np.ndarray:
    """Ratio-test matches as an ``int64`` array ``(M, 2)`` of (query, train), ascending query.

    ``kind`` (``DESC_SIFT`` / ``DESC_FLOAT``) is a hint for this call only: the context's own
    hint (:func:`set_descriptor_kind`) is restored afterwards.  Results never depend on it.

    ``cache_query``: ``des0`` is the keyframe side the reference matches every frame against
    (``vo.py:64-65``): the library keeps its device copy and packed rows across calls while the
    same unmodified torch tensor comes back.  Torch tensors already on the GPU are read in place
    (``vo_match_knn2_ratio_dev``: no descriptor crosses PCIe); results never depend on either.

    ``cross_check``: a kept pair ``(i, j)`` survives only if ``i`` is also the nearest query row
    of train row ``j`` (OpenCV's ``BFMatcher(crossCheck=True)`` rule on top of the ratio test,
    equal distances keeping the lower query index; ``vo_match_mutual``).  The pairs are then
    one-to-one.  ``False`` takes exactly the calls above."""
    ctx = ctx or _lib.context()
    dev = None if getattr(ctx, "_foreign_tensors", False) else _gpu_tensors(des0, des1, ctx)
    if dev is not None:
        a, b = dev
        n0, n1, dim = a.shape[0], b.shape[0], a.shape[1]
    else:
        a, b = _as_des(des0), _as_des(des1)
        n0, n1, dim = a.shape[0], b.shape[0], a.shape[1]
    if n0 == 0 or n1 == 0:  # frontend.py:97-98
        return np.empty((0, 2), dtype=np.int64)
    if dim != b.shape[1]:
        raise ValueError(f"descriptor dims differ: {dim} vs {b.shape[1]}")
    tag = _tags(ctx).tag_for(des0) if cache_query else 0
    out = np.empty((n0, 2), dtype=np.int32)
    cnt = np.zeros(1, dtype=np.int32)
    prior = getattr(ctx, "desc_kind", DESC_AUTO)
    scoped = kind is not None and kind != prior
    if scoped:
        check(ctx.lib.vo_match_hint(ctx.handle, int(kind)), "vo_match_hint")
    try:
        if cross_check:
            if dev is not None:
                import torch

                torch.cuda.current_stream(a.device).synchronize()  # the tensors' producer is done
                p0, p1, flags = a.data_ptr(), b.data_ptr(), _lib.VO_MATCH_DEVICE_PTRS
            else:
                p0, p1, flags = a.ctypes.data, b.ctypes.data, 0
            rc = ctx.lib.vo_match_mutual(
                ctx.handle, C.c_void_p(p0), n0, C.c_uint64(tag), C.c_void_p(p1), n1, dim, float(ratio), flags,
                ptr(out, C.c_int32), ptr(cnt, C.c_int32))
            if dev is not None and rc == _lib.VO_ERR_ARG:
                # as below: torch's device memory is not this library's HIP runtime's
                ctx._foreign_tensors = True
                return match_knn2_ratio(des0.detach().cpu(), des1.detach().cpu(), ratio, ctx, kind, False, True)
            check(rc, "vo_match_mutual")
        elif dev is not None:
            import torch

            torch.cuda.current_stream(a.device).synchronize()  # the tensors' producer is done
            rc = ctx.lib.vo_match_knn2_ratio_dev(
                ctx.handle, C.c_void_p(a.data_ptr()), n0, C.c_uint64(tag), C.c_void_p(b.data_ptr()), n1, dim,
                float(ratio), ptr(out, C.c_int32), ptr(cnt, C.c_int32))
            if rc == _lib.VO_ERR_ARG and n0 and n1:
                # torch's device memory is not this library's HIP runtime's (the library refuses
                # such pointers before any launch): the host path from here on
                ctx._foreign_tensors = True
                return match_knn2_ratio(des0.detach().cpu(), des1.detach().cpu(), ratio, ctx, kind, False)
            check(rc, "vo_match_knn2_ratio_dev")
        elif tag:
            check(ctx.lib.vo_match_knn2_ratio_q(
                ctx.handle, ptr(a, C.c_float), n0, C.c_uint64(tag), ptr(b, C.c_float), n1, dim, float(ratio),
                ptr(out, C.c_int32), ptr(cnt, C.c_int32)), "vo_match_knn2_ratio_q")
        else:
            check(ctx.lib.vo_match_knn2_ratio(
                ctx.handle, ptr(a, C.c_float), n0, ptr(b, C.c_float), n1, dim, float(ratio),
                ptr(out, C.c_int32), ptr(cnt, C.c_int32)), "vo_match_knn2_ratio")
    finally:
        if scoped:
            check(ctx.lib.vo_match_hint(ctx.handle, int(prior)), "vo_match_hint")
    return out[: int(cnt[0])].astype(np.int64)


def _tags(ctx) -> _QueryTags:
    t = getattr(ctx, "_query_tags", None)
    if t is None:
        t = ctx._query_tags = _QueryTags()
    return t


def _gpu_tensors(des0, des1, ctx):
    """Both descriptor sets as (N, D) float32 torch tensors on the context's GPU, or None (host
    path): only tensors torch already holds on ``cuda:<ctx.device>`` qualify."""
    if not (hasattr(des0, "is_cuda") and hasattr(des1, "is_cuda")):
        return None
    if not (des0.is_cuda and des1.is_cuda):
        return None
    if des0.device.index != ctx.device or des1.device.index != ctx.device:
        return None
    return _tensor_2d(des0), _tensor_2d(des1)


def _as_xy(p, what: str, cols: int = 2) -> np.ndarray:
    if hasattr(p, "detach"):
        p = p.detach().cpu().numpy()
    p = np.asarray(p)
    if p.ndim == 3 and p.shape[0] == 1:  # (1, N, 2) feature-dict layout
        p = p[0]
    if p.ndim != 2 or p.shape[1] != cols:
        raise ValueError(f"{what} must be (N, {cols}), got shape {p.shape}")
    return np.ascontiguousarray(p, dtype=np.float32)


def match_gated(des0, pred, radius, des1, kp1, ratio: float = RATIO_THRESH, max_dist: float = 0.0,
                unique: bool = True, image_size=None, return_dist: bool = False,
                ctx: _lib.Context | None = None):
    """Projection-gated matching (``vo_match_gated``): query row ``i`` (a landmark's descriptor) is
    compared only with the train rows whose keypoint ``kp1[j]`` lies within ``radius[i]`` pixels of
    its predicted position ``pred[i]``; see ``include/vo_hip.h`` for the exact gate and keep rule.

    ``des0 (n0, D)``, ``pred (n0, 2)`` and ``radius`` (a scalar, or ``(n0,)``; negative or NaN = the
    query is inactive) are host data.  ``des1 (n1, D)`` and ``kp1 (n1, 2)`` may be the feature
    dict's tensors: torch tensors on the context's GPU are read in place, and the call falls back
    to host arrays as :func:`match_knn2_ratio` does when the library refuses the pointers.
    ``max_dist`` 0 is not tested; a lone candidate passes the ratio test, so set it.  ``unique``
    keeps, per train row, only the pair with the smallest ``(dist, query)``: needed before ids are
    written.  ``image_size`` ``(width, height)`` only sizes the search grid; results never depend
    on it.

    Returns ``(M, 2)`` int64 (query, train) pairs in ascending query order, and with
    ``return_dist`` also their float32 distances."""
    return _match_gate("circle", des0, pred, radius, des1, kp1, ratio, max_dist, unique, image_size, return_dist, ctx)


def match_segment(des0, seg, radius, des1, kp1, ratio: float = RATIO_THRESH, max_dist: float = 0.0,
                  unique: bool = True, image_size=None, return_dist: bool = False,
                  ctx: _lib.Context | None = None):
    """Segment-gated matching (``vo_match_segment``): :func:`match_gated` with a capsule for a gate.
    Query row ``i`` is compared only with the train rows whose keypoint ``kp1[j]`` lies within
    ``radius[i]`` pixels of the segment ``seg[i] = (ax, ay, bx, by)`` given in the train image; see
    ``include/vo_hip.h`` for the exact gate.  A zero-length segment is :func:`match_gated`'s circle to
    the bit; :func:`epipolar_segments` makes the segments of the epipolar search for new landmarks.

    ``seg`` is ``(n0, 4)`` host data (a non-finite value makes the query inactive, as a negative or
    NaN radius does); every other argument, the tensors read in place, the fallback, the return
    types, the empty-input behaviour and the errors are :func:`match_gated`'s."""
    return _match_gate("segment", des0, seg, radius, des1, kp1, ratio, max_dist, unique, image_size, return_dist, ctx)


# gate -> (C entry, its options struct, the per-query array's field, its columns)
_GATES = {"circle": ("vo_match_gated", _lib.MatchGateOptionsC, "pred", 2),
          "segment": ("vo_match_segment", _lib.MatchSegmentOptionsC, "seg", 4)}


def _match_gate(gate, des0, query, radius, des1, kp1, ratio, max_dist, unique, image_size, return_dist, ctx):
    ctx = ctx or _lib.context()
    a = _as_des(des0)
    fn, options, what, cols = _GATES[gate]
    p = _as_xy(query, what, cols)
    n0, dim = a.shape
    if p.shape[0] != n0:
        raise ValueError(f"{what} has {p.shape[0]} rows for {n0} query rows")
    rad = None
    radius0 = 0.0
    if np.ndim(radius) == 0:
        radius0 = float(radius)
    else:
        rad = np.ascontiguousarray(radius, dtype=np.float32).reshape(-1)
        if rad.shape[0] != n0:
            raise ValueError(f"radius has {rad.shape[0]} entries for {n0} query rows")
    dev = None if getattr(ctx, "_foreign_tensors", False) else _gpu_tensors(des1, kp1, ctx)
    if dev is not None:
        b, k = dev
    else:
        b, k = _as_des(des1), _as_xy(kp1, "kp1")
    n1 = b.shape[0]
    if tuple(k.shape) != (n1, 2):
        raise ValueError(f"kp1 must be ({n1}, 2), got shape {tuple(k.shape)}")
    empty = np.empty((0, 2), dtype=np.int64)
    if n0 == 0 or n1 == 0:
        return (empty, np.empty(0, np.float32)) if return_dist else empty
    if dim != b.shape[1]:
        raise ValueError(f"descriptor dims differ: {dim} vs {b.shape[1]}")
    width, height = (int(image_size[0]), int(image_size[1])) if image_size is not None else (0, 0)
    flags = _lib.VO_MATCH_GATE_UNIQUE if unique else 0
    if dev is not None:
        import torch

        torch.cuda.current_stream(b.device).synchronize()  # the tensors' producer is done
        p1, pk = b.data_ptr(), k.data_ptr()
        flags |= _lib.VO_MATCH_DEVICE_PTRS
    else:
        p1, pk = b.ctypes.data, k.ctypes.data
    opt = options(radius=rad.ctypes.data if rad is not None else None, kp1=pk, radius0=radius0, width=width,
                  height=height, ratio=float(ratio), max_dist=float(max_dist), flags=flags, reserved=0,
                  **{what: p.ctypes.data})
    out = np.empty((n0, 2), dtype=np.int32)
    dist = np.empty(n0, dtype=np.float32)
    cnt = np.zeros(1, dtype=np.int32)
    rc = getattr(ctx.lib, fn)(ctx.handle, C.c_void_p(a.ctypes.data), n0, C.c_void_p(p1), n1, dim, C.byref(opt),
                              ptr(out, C.c_int32), ptr(dist, C.c_float), ptr(cnt, C.c_int32))
    if dev is not None and rc == _lib.VO_ERR_ARG:
        # torch's device memory is not this library's HIP runtime's (the library refuses such
        # pointers before any launch): the host path from here on
        ctx._foreign_tensors = True
        return _match_gate(gate, a, p, rad if rad is not None else radius0, des1.detach().cpu(), kp1.detach().cpu(),
                           ratio, max_dist, unique, image_size, return_dist, ctx)
    check(rc, fn)
    m = int(cnt[0])
    pairs = out[:m].astype(np.int64)
    return (pairs, dist[:m].copy()) if return_dist else pairs


def project_points(points_w, T_cw, K, image_size, min_depth: float = 0.0):
    """Pinhole projection of world points into a frame: ``(pred float32 (n, 2), valid bool (n,))``.

    ``T_cw`` (4, 4) world -> camera, ``K`` (3, 3), ``image_size`` ``(width, height)``.  Computed in
    numpy float64 and cast once.  A point is invalid when its depth ``z <= min_depth`` or its
    projection falls outside ``[0, width) x [0, height)`` (or is not finite); the caller gives
    invalid points radius -1 in :func:`match_gated`."""
    X = np.asarray(points_w, np.float64).reshape(-1, 3)
    T = np.asarray(T_cw, np.float64)
    K = np.asarray(K, np.float64)
    Xc = X @ T[:3, :3].T + T[:3, 3]
    z = Xc[:, 2]
    front = z > float(min_depth)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = K[0, 0] * Xc[:, 0] / z + K[0, 2]
        v = K[1, 1] * Xc[:, 1] / z + K[1, 2]
    width, height = float(image_size[0]), float(image_size[1])
    with np.errstate(invalid="ignore"):
        valid = front & np.isfinite(u) & np.isfinite(v) & (u >= 0) & (u < width) & (v >= 0) & (v < height)
    with np.errstate(over="ignore", invalid="ignore"):
        pred = np.stack([u, v], axis=1).astype(np.float32)
    return pred, valid


EPIPOLAR_NEAR = 1e-3  # depth in the second camera at which a ray crossing its camera plane is cut


def epipolar_segments(kp0, T_cw0, T_cw1, K, image_size, z_min: float, z_max: float = np.inf,
                      min_length: float = 0.0):
    """Where keypoints of view 0 can reappear in view 1: ``(seg float32 (n, 4), valid bool (n,))``,
    ``seg[i] = (ax, ay, bx, by)`` for :func:`match_segment`.

    ``kp0[i]`` is back-projected to the depths ``z_min`` and ``z_max`` in camera 0 (``inf``: the
    point at infinity of its ray, whose image is the vanishing point), both are taken into camera 1
    (``T_cw`` (4, 4) world -> camera), the 3-D segment is cut at depth ``EPIPOLAR_NEAR`` where it
    crosses camera 1's plane, its ends are projected with ``K`` and the image segment is clipped to
    ``[0, width] x [0, height]``.  ``a`` is the near end.  ``valid`` is false when nothing is left
    (the whole range lies behind camera 1 or projects outside the image), when the result is not
    finite, or when the clipped segment is shorter than ``min_length`` pixels: the depth of such a
    keypoint is not observable from this pair.  An invalid row is NaN: an inactive query of
    :func:`match_segment`.
    Computed in numpy float64 and cast once."""
    kp = np.asarray(kp0, np.float64).reshape(-1, 2)
    K = np.asarray(K, np.float64)
    T10 = np.asarray(T_cw1, np.float64) @ np.linalg.inv(np.asarray(T_cw0, np.float64))
    R, t = T10[:3, :3], T10[:3, 3]
    n = len(kp)
    width, height = float(image_size[0]), float(image_size[1])
    z_min, z_max = float(z_min), float(z_max)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d0 = np.stack([(kp[:, 0] - K[0, 2]) / K[0, 0], (kp[:, 1] - K[1, 2]) / K[1, 1], np.ones(n)], axis=1)
        d = d0 @ R.T  # the ray in camera 1: X(z) = z d + t, z the depth in camera 0
        c = d[:, 2]
        # the depths z at which the point is at least EPIPOLAR_NEAR in front of camera 1
        cut = (EPIPOLAR_NEAR - t[2]) / c
        lo = np.where(c > 0, np.maximum(z_min, cut), z_min)
        hi = np.where(c < 0, np.minimum(z_max, cut), z_max)
        ok = (lo <= hi) & ((c != 0) | (t[2] >= EPIPOLAR_NEAR))

        def project(z):
            far = np.isinf(z)  # the vanishing point: the projection of the direction
            zz = np.where(far, 0.0, z)
            X = np.where(far[:, None], d, zz[:, None] * d + t)
            return np.stack([K[0, 0] * X[:, 0] / X[:, 2] + K[0, 2], K[1, 1] * X[:, 1] / X[:, 2] + K[1, 2]], axis=1)

        a, b = project(lo), project(hi)
        ok &= np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1)
        # Liang-Barsky: the part a + s (b - a), s in [s0, s1], inside the rectangle
        e = b - a
        s0, s1 = np.zeros(n), np.ones(n)
        for p, q in ((-e[:, 0], a[:, 0]), (e[:, 0], width - a[:, 0]), (-e[:, 1], a[:, 1]), (e[:, 1], height - a[:, 1])):
            ok &= (p != 0) | (q >= 0)  # parallel to this border and outside it
            r = q / p
            s0 = np.where(p < 0, np.maximum(s0, r), s0)
            s1 = np.where(p > 0, np.minimum(s1, r), s1)
        ok &= s0 <= s1
        ca, cb = a + s0[:, None] * e, a + s1[:, None] * e
        hi_xy = np.array([width, height])
        ca, cb = np.clip(ca, 0.0, hi_xy), np.clip(cb, 0.0, hi_xy)  # (rounding only: the ends are on the border)
        seg = np.concatenate([ca, cb], axis=1)
        ok &= np.isfinite(seg).all(axis=1)
        ok &= np.hypot(cb[:, 0] - ca[:, 0], cb[:, 1] - ca[:, 1]) >= float(min_length)
        seg = np.where(ok[:, None], seg, np.nan).astype(np.float32)
    return seg, ok


def match_knn2(des0, des1, ctx: _lib.Context | None = None):
    """knnMatch(k=2) alone: ``idx (n0, 2) int32`` (-1 = none), ``dist (n0, 2) float32``."""
    a, b = _as_des(des0), _as_des(des1)
    n0 = a.shape[0]
    idx = np.full((n0, 2), -1, dtype=np.int32)
    dist = np.full((n0, 2), np.finfo(np.float32).max, dtype=np.float32)
    if n0 == 0:
        return idx, dist
    if b.shape[0] and a.shape[1] != b.shape[1]:
        raise ValueError(f"descriptor dims differ: {a.shape[1]} vs {b.shape[1]}")
    ctx = ctx or _lib.context()
    check(
        ctx.lib.vo_match_knn2(
            ctx.handle, ptr(a, C.c_float), n0, ptr(b, C.c_float), b.shape[0], a.shape[1],
            ptr(idx, C.c_int32), ptr(dist, C.c_float),
        ),
        "vo_match_knn2",
    )
    return idx, dist


HAMMING_RATIO = 0.8
HAMMING_MAX_WORDS = 16


def _as_bits(d) -> np.ndarray:
    """Binary rows as contiguous uint32 (n, words): uint32 / int32 as they are, uint8 (n, 4 words)
    viewed (OpenCV's layout of ORB / BRIEF rows, little endian)."""
    if hasattr(d, "detach"):
        d = d.detach().cpu().numpy()
    d = np.asarray(d)
    if d.ndim != 2:
        raise ValueError(f"binary descriptors must be (N, words), got shape {d.shape}")
    if d.dtype == np.uint8:
        if d.shape[1] % 4:
            raise ValueError(f"uint8 binary descriptors must have a multiple of 4 columns, got {d.shape[1]}")
        return np.ascontiguousarray(d).view(np.uint32)
    if d.dtype not in (np.uint32, np.int32):
        raise ValueError(f"binary descriptors must be uint32, int32 or uint8, got {d.dtype}")
    return np.ascontiguousarray(d).view(np.uint32)


def _device_bits(d, ctx):
    """(pointer, n, words, keep-alive) of rows already on the context's GPU, or None: a
    :class:`_lib.DeviceArray` of 32-bit words, or a torch int32 tensor on ``cuda:<ctx.device>``."""
    if isinstance(d, _lib.DeviceArray):
        if len(d.shape) != 2 or d.dtype.itemsize != 4:
            raise ValueError("a DeviceArray of binary descriptors must be (N, words) of 32-bit words")
        return d.ptr, d.shape[0], d.shape[1], d
    if getattr(d, "is_cuda", False) and d.device.index == ctx.device and not getattr(ctx, "_foreign_tensors", False):
        import torch

        if d.dtype != torch.int32 or d.dim() != 2:
            raise ValueError("a CUDA tensor of binary descriptors must be int32 (N, words)")
        t = d.detach().contiguous()
        return t.data_ptr(), t.shape[0], t.shape[1], t
    return None


def match_hamming(des0, des1, ratio: float = HAMMING_RATIO, max_dist=None, cross_check: bool = False,
                  return_dist: bool = False, return_knn: bool = False, ctx: _lib.Context | None = None):
    """Brute-force Hamming matching of binary descriptors (``vo_match_hamming``): the structure of
    ``cv2.BFMatcher(cv2.NORM_HAMMING)`` with ``knnMatch(k=2)`` and a ratio test; see
    ``include/vo_hip.h`` for the exact keys and the keep rule.

    ``des0``, ``des1``: numpy ``uint32 (n, words)`` (:func:`visualodometry_amd.brief.describe`'s
    rows) or ``uint8 (n, 4 words)``, ``words`` in 1..16.  Both being torch int32 tensors on the
    context's GPU (or :class:`_lib.DeviceArray`), they are read in place; the call falls back to
    host arrays as :func:`match_knn2_ratio` does when the library refuses torch's pointers.
    ``max_dist`` ``None`` or 0 is not tested.  ``cross_check``: a kept pair ``(i, j)`` survives only
    if ``i`` is the nearest query row of ``j`` (ties to the lower ``i``); the pairs are then
    one-to-one.

    Returns ``(M, 2)`` int64 (query, train) pairs in ascending query order; with ``return_dist`` also
    their int32 distances; with ``return_knn`` also ``(idx (n0, 2) int32, dist (n0, 2) int32)``, -1
    and ``INT32_MAX`` where no neighbour exists."""
    on_device = [isinstance(d, _lib.DeviceArray) or bool(getattr(d, "is_cuda", False)) for d in (des0, des1)]
    if all(on_device):
        ctx = ctx or _lib.context()
    d0, d1 = (_device_bits(des0, ctx), _device_bits(des1, ctx)) if all(on_device) else (None, None)
    dev = d0 is not None and d1 is not None
    if dev:
        (p0, n0, words, _k0), (p1, n1, w1, _k1) = d0, d1
        if any(hasattr(d, "is_cuda") for d in (des0, des1)):
            import torch

            torch.cuda.current_stream(torch.device("cuda", ctx.device)).synchronize()  # the tensors' producer is done
    else:
        a = des0.numpy() if isinstance(des0, _lib.DeviceArray) else _as_bits(des0)
        b = des1.numpy() if isinstance(des1, _lib.DeviceArray) else _as_bits(des1)
        a, b = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
        (n0, words), (n1, w1) = a.shape, b.shape
        p0, p1 = a.ctypes.data, b.ctypes.data
    if words != w1:
        raise ValueError(f"descriptor widths differ: {words} vs {w1} words")
    if not 1 <= words <= HAMMING_MAX_WORDS:
        raise ValueError(f"binary descriptors must have 1..{HAMMING_MAX_WORDS} 32-bit words, got {words}")
    kidx = np.full((n0, 2), -1, np.int32)
    kdist = np.full((n0, 2), np.iinfo(np.int32).max, np.int32)
    if n0 == 0 or n1 == 0:  # nothing to match: no device is needed
        res = [np.empty((0, 2), np.int64)] + ([np.empty(0, np.int32)] if return_dist else []) + \
            ([(kidx, kdist)] if return_knn else [])
        return res[0] if len(res) == 1 else tuple(res)
    ctx = ctx or _lib.context()
    flags = (_lib.VO_MATCH_HAMMING_MUTUAL if cross_check else 0) | (_lib.VO_MATCH_DEVICE_PTRS if dev else 0)
    opt = _lib.MatchHammingOptionsC(ratio=float(ratio), max_dist=int(max_dist or 0), flags=flags, reserved=0)
    out = np.empty((n0, 2), dtype=np.int32)
    dist = np.empty(n0, dtype=np.int32)
    cnt = np.zeros(1, dtype=np.int32)
    rc = ctx.lib.vo_match_hamming(ctx.handle, C.c_void_p(p0), n0, C.c_void_p(p1), n1,
                                  words, C.byref(opt), out.ctypes.data, dist.ctypes.data, ptr(cnt, C.c_int32),
                                  kidx.ctypes.data if return_knn else None, kdist.ctypes.data if return_knn else None)
    if dev and rc == _lib.VO_ERR_ARG and hasattr(des0, "is_cuda") and hasattr(des1, "is_cuda"):
        # torch's device memory is not this library's HIP runtime's (the library refuses such
        # pointers before any launch): the host path from here on
        ctx._foreign_tensors = True
        return match_hamming(des0.detach().cpu(), des1.detach().cpu(), ratio, max_dist, cross_check, return_dist,
                             return_knn, ctx)
    check(rc, "vo_match_hamming")
    m = int(cnt[0])
    res = [out[:m].astype(np.int64)]
    if return_dist:
        res.append(dist[:m].copy())
    if return_knn:
        res.append((kidx, kdist))
    return res[0] if len(res) == 1 else tuple(res)


def match_batch_device(des0: _lib.DeviceArray, des1: _lib.DeviceArray, ratio: float = RATIO_THRESH,
                       out: _lib.DeviceArray | None = None, ctx: _lib.Context | None = None,
                       cross_check: bool = False):
    """Batched frame pairs already resident in HBM.

    ``des0`` (B, n0, D) and ``des1`` (B, n1, D) float32 :class:`DeviceArray`;
    returns the (B, n0) int32 :class:`DeviceArray` of kept train indices
    (-1 = rejected).  Enqueued on the library stream; call :func:`synchronize`.
    ``cross_check`` as in :func:`match_knn2_ratio` (``vo_match_mutual_batch_async``).
    """
    if len(des0.shape) != 3 or len(des1.shape) != 3 or des0.shape[0] != des1.shape[0] \
            or des0.shape[2] != des1.shape[2]:
        raise ValueError("expected (B, n0, D) and (B, n1, D)")
    if des0.dtype != np.float32 or des1.dtype != np.float32:
        raise ValueError("expected float32 descriptors")
    B, n0, D = des0.shape
    ctx = ctx or des0.ctx
    if out is None:
        out = _lib.DeviceArray(ctx, (B, n0), np.int32)
    name = "vo_match_mutual_batch_async" if cross_check else "vo_match_batch_async"
    check(
        getattr(ctx.lib, name)(
            ctx.handle, C.c_void_p(des0.ptr), C.c_void_p(des1.ptr), B, n0, des1.shape[1], D,
            float(ratio), C.c_void_p(out.ptr),
        ),
        name,
    )
    return out


DESC_AUTO, DESC_SIFT, DESC_FLOAT = 0, 1, 2  # vo_match_hint kinds (include/vo_hip.h)


def set_descriptor_kind(kind: int, ctx: _lib.Context | None = None) -> None:
    """``vo_match_hint``: which descriptors later calls on ``ctx`` expect (results never
    depend on it).  ``DESC_SIFT`` leaves the float shortlist unlaunched (the drop-in sets it
    for the reference's SIFT extractor); ``DESC_AUTO`` launches both paths' kernels."""
    ctx = ctx or _lib.context()
    check(ctx.lib.vo_match_hint(ctx.handle, int(kind)), "vo_match_hint")
    ctx.desc_kind = int(kind)  # restored by match_knn2_ratio after a per-call hint


def synchronize(ctx: _lib.Context | None = None) -> None:
    ctx = ctx or _lib.context()
    check(ctx.lib.vo_synchronize(ctx.handle), "vo_synchronize")
