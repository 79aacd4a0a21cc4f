"""Expected values of the mutual-check matcher, composed from the existing oracle.

``pairs = match_int / match_c(d0, d1, ratio)`` (the forward pass, unchanged), kept iff
``knn2_int / knn2_c(d1, d0)[0][j, 0] == i``: the nearest query row of train row ``j`` under
keys ``(sqrtf(d2), i')`` -- the oracle's own tie rule with the roles swapped.  Also the input
builders the GPU tests share (near-duplicate query rows, repeated query rows).
"""

import numpy as np

from oracle import match_ref
from visualodometry_amd.synthetic import sift_like_pair, superpoint_like_pair


def forward(d0, d1, ratio=match_ref.RATIO_THRESH, oracle="int"):
    if oracle == "int":
        return match_ref.match_int(d0, d1, ratio)
    return match_ref.match_c(d0, d1, ratio, nthreads=8)


def reverse_nearest(d0, d1, oracle="int"):
    """``rev[j]`` = the nearest query row of train row ``j`` (lower query index on equal distances)."""
    if len(d0) == 0 or len(d1) == 0:
        return np.full(len(d1), -1, np.int32)
    idx, _ = match_ref.knn2_int(d1, d0) if oracle == "int" else match_ref.knn2_c(d1, d0, nthreads=8)
    return idx[:, 0]


def mutual(d0, d1, ratio=match_ref.RATIO_THRESH, oracle="int"):
    """``(M, 2)`` int64 pairs surviving ratio test and cross check, and the forward pair count."""
    fwd = forward(d0, d1, ratio, oracle)
    if len(fwd) == 0:
        return fwd.reshape(0, 2), 0
    rev = reverse_nearest(d0, d1, oracle)
    keep = rev[fwd[:, 1]] == fwd[:, 0]
    return fwd[keep], len(fwd)


def informative(kept, n_forward):
    """A case shows something only if the cross check removes some pairs, not all."""
    return 0 < len(kept) < n_forward


def sift_near_duplicates(n0=300, n1=400, seed=3, extra=150, dim=128):
    """A SIFT-like pair with ``extra`` near-duplicates of the first query rows appended to the
    query side (``d0[:extra] + N(0, 3)``, rounded and clipped to 0..255): a keyframe with
    repeated structure, where the ratio test alone keeps many-to-one pairs."""
    d0, d1 = sift_like_pair(n0, n1, seed, dim=dim)
    rng = np.random.default_rng(1000 + seed)
    dup = np.clip(np.rint(d0[:extra] + rng.normal(0.0, 3.0, (extra, d0.shape[1]))), 0, 255).astype(np.float32)
    return np.concatenate([d0, dup]), d1


def superpoint_near_duplicates(n0=300, n1=400, seed=3, extra=150, dim=256):
    """The float counterpart: ``d0[:extra] + 0.1 N(0, 1)``, renormalised."""
    d0, d1 = superpoint_like_pair(n0, n1, seed, dim=dim)
    rng = np.random.default_rng(1000 + seed)
    dup = d0[:extra] + 0.1 * rng.standard_normal((extra, d0.shape[1])).astype(np.float32)
    dup /= np.linalg.norm(dup, axis=1, keepdims=True)
    return np.concatenate([d0, dup.astype(np.float32)]), d1


def repeated_queries(kind, seed=41, distinct=200, repeat=4, dim=128):
    """``distinct`` rows, each ``repeat`` times at shuffled positions among the query rows,
    against one noisy copy of each as train: every train row has ``repeat`` exactly equal
    reverse distances (inside a 16-lane group, across tiles, across splits), and the lowest
    query index must win."""
    rng = np.random.default_rng(seed)
    if kind == "int":
        base = rng.integers(0, 256, (distinct, dim)).astype(np.float32)
        d1 = np.clip(np.rint(base + rng.normal(0.0, 4.0, base.shape)), 0, 255).astype(np.float32)
    else:
        base = rng.standard_normal((distinct, dim)).astype(np.float32)
        base /= np.linalg.norm(base, axis=1, keepdims=True)
        d1 = (base + 0.05 * rng.standard_normal(base.shape)).astype(np.float32)
    d0 = base[rng.permutation(np.repeat(np.arange(distinct), repeat))]
    return np.ascontiguousarray(d0), d1[rng.permutation(distinct)]
