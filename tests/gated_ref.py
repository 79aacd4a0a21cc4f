"""Expected values of the projection-gated matcher (``vo_match_gated``), composed from the oracle.

The gate in numpy (float32 differences, float64 squares); per query ``cref.knn2`` over its
ascending candidate list -- the C oracle's k-ordered fmaf chain, ``sqrtf``, strict ``<`` insertion
scan (equal distances keep the lower index, a distance that is not ``< FLT_MAX`` is never
selected) -- with the indices mapped back; then the keep rule and the unique rule in plain Python.
Also the scene builder the GPU tests share.
"""

from dataclasses import dataclass

import numpy as np

from oracle import cref


def candidates(pred, radius, kp1):
    """Per query the ascending train indices inside its gate (empty for an inactive query)."""
    pred = np.asarray(pred, np.float32).reshape(-1, 2)
    kp1 = np.asarray(kp1, np.float32).reshape(-1, 2)
    r = np.broadcast_to(np.asarray(radius, np.float32), (len(pred),))
    kp_ok = np.isfinite(kp1).all(axis=1)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(len(pred)):
            if not (np.isfinite(pred[i]).all() and r[i] >= 0):
                out.append(np.zeros(0, np.int64))
                continue
            dx = (kp1[:, 0] - pred[i, 0]).astype(np.float64)  # float32 subtraction, then widened
            dy = (kp1[:, 1] - pred[i, 1]).astype(np.float64)
            inside = (dx * dx + dy * dy <= np.float64(r[i]) * np.float64(r[i])) & kp_ok
            out.append(np.flatnonzero(inside))
    return out


@dataclass
class Gated:
    pairs: np.ndarray      # (M, 2) int64, ascending query
    dist: np.ndarray       # (M,) float32, dist1 per pair
    n_cand: np.ndarray     # (n0,) candidates per query
    n_ratio: int           # pairs passing the selection and the ratio test alone
    n_near: int            # ... and max_dist
    n_final: int           # ... and the unique rule (== len(pairs))


def gated(d0, pred, radius, d1, kp1, ratio=0.75, max_dist=0.0, unique=True) -> Gated:
    d0 = np.ascontiguousarray(d0, np.float32)
    d1 = np.ascontiguousarray(d1, np.float32)
    cands = candidates(pred, radius, kp1)
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


def informative(g: Gated) -> bool:
    """A scene shows something only if every rule bites and none wipes the result out."""
    return bool((g.n_cand == 0).any() and (g.n_cand == 1).any() and (g.n_cand >= 3).any()
                and 0 < g.n_near < g.n_ratio and 0 < g.n_final < g.n_near)


@dataclass
class Scene:
    d0: np.ndarray      # (n0, dim) landmark descriptors
    pred: np.ndarray    # (n0, 2) predicted positions (one NaN row)
    radius: np.ndarray  # (n0,) per-query radii: `radius` with a few -1
    d1: np.ndarray      # (n1, dim) keypoint descriptors
    kp1: np.ndarray     # (n1, 2) keypoint positions
    size: tuple         # (width, height)
    truth: np.ndarray   # (n0,) the keypoint each landmark was observed as, or -1


def scene(kind, n0, n1, seed, dim=None, size=(1241, 376), radius=12.0, jitter=4.0, found=0.6, dup=0.15) -> Scene:
    """Landmarks with predictions; keypoints that are jittered, noisy copies of a share of them plus
    clutter; near-duplicate landmarks predicted near their originals; a few inactive queries.
    ``kind`` "sift": integers 0..255 (dim 128); "float": unit rows (dim 256)."""
    rng = np.random.default_rng(seed)
    dim = dim or (128 if kind == "sift" else 256)
    w, h = size

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

    n_dup = int(dup * n0)
    n_base = n0 - n_dup
    n_found = min(int(found * n_base), n1)
    pos = np.stack([rng.uniform(0, w, n_base), rng.uniform(0, h, n_base)], axis=1)
    base = fresh(n_base)
    seen = rng.permutation(n_base)[:n_found]
    kp_found = pos[seen] + rng.normal(0.0, jitter, (n_found, 2))
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
    # near-duplicates of observed landmarks, predicted near them: the unique rule's work
    src = seen[rng.integers(0, n_found, n_dup)]
    d0 = np.concatenate([base, noisy(base[src], 3.0, 0.01)])
    pred = np.concatenate([pos + rng.normal(0.0, 1.5, pos.shape), pos[src] + rng.normal(0.0, 2.0, (n_dup, 2))])
    pred = pred.astype(np.float32)
    rad = np.full(n0, radius, np.float32)
    quiet = rng.permutation(n0)[:6]
    rad[quiet[:3]] = -1.0
    rad[quiet[3]] = np.nan
    pred[quiet[4], 0] = np.nan
    pred[quiet[5], 1] = np.inf
    truth[quiet] = -1
    return Scene(np.ascontiguousarray(d0), pred, rad, np.ascontiguousarray(d1), kp.astype(np.float32), size, truth)
