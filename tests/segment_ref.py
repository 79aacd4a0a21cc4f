"""Expected values of the segment-gated matcher (``vo_match_segment``), composed from the oracle.

``candidates`` is the capsule gate of ``include/vo_hip.h`` in numpy: float32 differences widened to
float64, products of two widened floats (exact), two-term sums (one rounding each; numpy never
fuses, and fusing would round the same exact sum once), the three tests in the header's order.
``segmented`` is ``gated_ref.gated``'s body behind that gate: ``cref.knn2`` per query over its
ascending candidate list, then the keep rule and the unique rule.  Also the two-view scene the
tests share: keypoints of one view, their epipolar segments in the other, and what is seen there.
"""

from dataclasses import dataclass

import numpy as np

from oracle import cref
from tests.gated_ref import Gated, informative  # noqa: F401  (informative: the scene tests' condition)
from visualodometry_amd import matcher
from visualodometry_amd.synthetic import KITTI_K, KITTI_WH


def candidates(seg, radius, kp1):
    """Per query the ascending train indices inside its capsule (empty for an inactive query)."""
    seg = np.asarray(seg, np.float32).reshape(-1, 4)
    kp1 = np.asarray(kp1, np.float32).reshape(-1, 2)
    r = np.broadcast_to(np.asarray(radius, np.float32), (len(seg),))
    kp_ok = np.isfinite(kp1).all(axis=1)
    kx, ky = kp1[:, 0], kp1[:, 1]
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(len(seg)):
            if not (np.isfinite(seg[i]).all() and r[i] >= 0):
                out.append(np.zeros(0, np.int64))
                continue
            ax, ay, bx, by = seg[i]
            dx, dy = np.float64(bx - ax), np.float64(by - ay)  # float32 subtractions, then widened
            vx, vy = (kx - ax).astype(np.float64), (ky - ay).astype(np.float64)
            wx, wy = (kx - bx).astype(np.float64), (ky - by).astype(np.float64)
            dd = dx * dx + dy * dy
            s = vx * dx + vy * dy
            cr = vx * dy - vy * dx
            r2 = np.float64(r[i]) * np.float64(r[i])
            at_a = s <= 0
            at_b = ~at_a & (s >= dd)
            mid = ~at_a & ~at_b  # a NaN s lands here with a NaN cr: comparisons false, as in the header
            inside = (at_a & (vx * vx + vy * vy <= r2)) | (at_b & (wx * wx + wy * wy <= r2)) | \
                (mid & (cr * cr <= r2 * dd))
            out.append(np.flatnonzero(inside & kp_ok))
    return out


def segmented(d0, seg, radius, d1, kp1, ratio=0.75, max_dist=0.0, unique=True) -> Gated:
    d0 = np.ascontiguousarray(d0, np.float32)
    d1 = np.ascontiguousarray(d1, np.float32)
    cands = candidates(seg, radius, kp1)
    kept = []  # (i, j, dist)
    n_ratio = 0
    for i, c in enumerate(cands):
        if len(c) == 0:
            continue
        idx, dist = cref.knn2(d0[i:i + 1], d1[c])
        if idx[0, 0] < 0:
            continue
        s1 = dist[0, 0]
        if idx[0, 1] >= 0 and not float(s1) < ratio * float(dist[0, 1]):
            continue
        n_ratio += 1
        if max_dist != 0 and not s1 <= np.float32(max_dist):
            continue
        kept.append((i, int(c[idx[0, 0]]), s1))
    n_near = len(kept)
    if unique:
        owner = {}
        for i, j, s in kept:  # ascending i: an equal distance never displaces the lower query
            if j not in owner or s < owner[j][1]:
                owner[j] = (i, s)
        kept = [(i, j, s) for i, j, s in kept if owner[j][0] == i]
    pairs = np.array([(i, j) for i, j, _ in kept], np.int64).reshape(-1, 2)
    dist = np.array([s for _, _, s in kept], np.float32)
    return Gated(pairs, dist, np.array([len(c) for c in cands]), n_ratio, n_near, len(kept))


def point_segment_distance(seg, kp1):
    """Plain float64 distances (n0, n1) from every keypoint to every segment (division and all)."""
    seg = np.asarray(seg, np.float64).reshape(-1, 4)
    k = np.asarray(kp1, np.float64).reshape(-1, 2)
    a, b = seg[:, None, :2], seg[:, None, 2:]
    d = b - a
    dd = (d * d).sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(dd > 0, ((k[None] - a) * d).sum(-1) / np.where(dd > 0, dd, 1.0), 0.0)
    t = np.clip(t, 0.0, 1.0)
    return np.linalg.norm(k[None] - (a + t[..., None] * d), axis=-1)


Z_MIN, Z_MAX = 2.0, 1e4


def two_view_pose(yaw=0.03, t=(-0.3, 0.02, -1.0)):
    """(T_cw0, T_cw1): camera 1 is camera 0 after a yaw and a translation (X1 = R X0 + t)."""
    c, s = np.cos(yaw), np.sin(yaw)
    T1 = np.eye(4)
    T1[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    T1[:3, 3] = t
    return np.eye(4), T1


@dataclass
class Scene:
    d0: np.ndarray      # (n0, dim) descriptors of view 0's keypoints (the queries)
    kp0: np.ndarray     # (n0, 2) float32 their positions in view 0
    depth: np.ndarray   # (n0,) their depths in camera 0
    seg: np.ndarray     # (n0, 4) float32 epipolar segments in view 1 (one NaN, one inf value planted)
    valid: np.ndarray   # (n0,) epipolar_segments' own flag
    radius: np.ndarray  # (n0,) per-query radii: `radius` with a -1 and a NaN
    d1: np.ndarray      # (n1, dim) descriptors of view 1's keypoints
    kp1: np.ndarray     # (n1, 2) float32
    size: tuple         # (width, height)
    truth: np.ndarray   # (n0,) the view-1 keypoint each query was seen as, or -1
    proj1: np.ndarray   # (n0, 2) float64 noise-free projection of each query's point into view 1
    quiet: np.ndarray   # the queries made inactive
    T_cw0: np.ndarray
    T_cw1: np.ndarray
    K: np.ndarray


def scene(kind, n0, n1, seed, dim=None, radius=3.0, found=0.6, dup=0.15, noise_px=0.7) -> Scene:
    """Two views of points at depths U(4, 60): ``found`` of the queries are seen in view 1 with
    ``noise_px`` of noise and a noisy descriptor, the other view-1 keypoints are clutter; ``dup``
    of the queries are near-duplicates 0.5 px from a seen one; four queries are inactive.
    ``kind`` "sift": integers 0..255 (dim 128); "float": unit rows (dim 256)."""
    rng = np.random.default_rng(seed)
    dim = dim or (128 if kind == "sift" else 256)
    w, h = KITTI_WH
    K = np.asarray(KITTI_K, np.float64)
    T0, T1 = two_view_pose()

    def fresh(n):
        if kind == "sift":
            return rng.integers(0, 256, (n, dim)).astype(np.float32)
        x = rng.standard_normal((n, dim)).astype(np.float32)
        return x / np.linalg.norm(x, axis=1, keepdims=True)

    def noisy(x, sigma_int, sigma_float):
        if kind == "sift":
            return np.clip(np.rint(x + rng.normal(0.0, sigma_int, x.shape)), 0, 255).astype(np.float32)
        y = x + (sigma_float * rng.standard_normal(x.shape)).astype(np.float32)
        return (y / np.linalg.norm(y, axis=1, keepdims=True)).astype(np.float32)

    def into_view1(kp, z):
        X0 = np.stack([(kp[:, 0] - K[0, 2]) / K[0, 0] * z, (kp[:, 1] - K[1, 2]) / K[1, 1] * z, z], axis=1)
        X1 = X0 @ T1[:3, :3].T + T1[:3, 3]
        uv = np.stack([K[0, 0] * X1[:, 0] / X1[:, 2] + K[0, 2], K[1, 1] * X1[:, 1] / X1[:, 2] + K[1, 2]], axis=1)
        return uv, (X1[:, 2] > 0.5) & (uv[:, 0] >= 0) & (uv[:, 0] <= w) & (uv[:, 1] >= 0) & (uv[:, 1] <= h)

    n_dup = int(dup * n0)
    n_base = n0 - n_dup
    kp0 = np.stack([rng.uniform(0, w, n_base), rng.uniform(0, h, n_base)], axis=1).astype(np.float32)
    depth = rng.uniform(4.0, 60.0, n_base)
    base = fresh(n_base)
    uv1, inside = into_view1(kp0.astype(np.float64), depth)
    n_found = min(int(found * n_base), n1, int(inside.sum()))
    seen = rng.permutation(np.flatnonzero(inside))[:n_found]
    kp_found = uv1[seen] + rng.normal(0.0, noise_px, (n_found, 2))
    d_found = noisy(base[seen], 8.0, 0.02)
    n_clutter = n1 - n_found
    kp = np.concatenate([kp_found, np.stack([rng.uniform(0, w, n_clutter), rng.uniform(0, h, n_clutter)], axis=1)])
    d1 = np.concatenate([d_found, fresh(n_clutter)])
    order = rng.permutation(n1)
    kp, d1 = kp[order], d1[order]
    where = np.empty(n1, np.int64)
    where[order] = np.arange(n1)
    truth = -np.ones(n0, np.int64)
    truth[seen] = where[:n_found]
    # near-duplicates of seen queries, 0.5 px beside them in view 0: the unique rule's work
    src = seen[rng.integers(0, n_found, n_dup)]
    ang = rng.uniform(0, 2 * np.pi, n_dup)
    kp0 = np.concatenate([kp0, kp0[src] + 0.5 * np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32)])
    depth = np.concatenate([depth, depth[src]])
    d0 = np.concatenate([base, noisy(base[src], 3.0, 0.01)])
    proj1, _ = into_view1(kp0.astype(np.float64), depth)
    seg, valid = matcher.epipolar_segments(kp0, T0, T1, K, (w, h), Z_MIN, Z_MAX)
    rad = np.full(n0, radius, np.float32)
    quiet = rng.permutation(np.flatnonzero(valid))[:4]
    rad[quiet[0]] = -1.0
    rad[quiet[1]] = np.nan
    seg[quiet[2], 0] = np.nan
    seg[quiet[3], 3] = np.inf
    truth[quiet] = -1
    return Scene(np.ascontiguousarray(d0), kp0, depth, seg, valid, rad, np.ascontiguousarray(d1),
                 kp.astype(np.float32), (w, h), truth, proj1, quiet, T0, T1, K)
