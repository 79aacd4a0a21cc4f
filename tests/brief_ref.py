"""The steered BRIEF descriptor's contract (``include/vo_hip.h``) restated
literally in numpy: the direction tables, the test pattern and its 32 rotations, and per point the
status, the reflected 31 x 31 patch, the disc moments, the bin, the 5 x 5 box sums and the 256 bits.
What ``csrc/brief_math.h`` and ``csrc/brief.hip`` compute must equal this bit for bit.

Every quantity is an integer, so there is nothing to round: numpy's int64 holds every intermediate.
Also here: the shared test images and points, and the Hamming distance.
"""

from __future__ import annotations

import functools
import math

import numpy as np

BINS, TESTS, WORDS = 32, 256, 8
R = 15


def reflect(i, n: int) -> np.ndarray:
    """Reflection without repeating the edge (-1 -> 1, n -> n - 2), total for any n >= 1."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    m = np.mod(i, p)
    return np.where(m >= n, p - m, m)


@functools.lru_cache(maxsize=None)
def tables():
    """-> (P int8 (32, 256, 4), C int32 (32,), S int32 (32,)), read-only."""
    C, S = np.zeros(BINS, np.int64), np.zeros(BINS, np.int64)
    for k in range(8):
        C[k] = int(np.rint(16384.0 * math.cos(2.0 * math.pi * k / 32.0)))
        S[k] = int(np.rint(16384.0 * math.sin(2.0 * math.pi * k / 32.0)))
    for k in range(8, BINS):
        C[k], S[k] = -S[k - 8], C[k - 8]
    state = [0x5EED]

    def draw():
        state[0] = (state[0] * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        return (state[0] >> 33) % 9 - 4

    base, taken = [], set()
    while len(base) < TESTS:
        t = tuple(draw() + draw() + draw() for _ in range(4))
        px, py, qx, qy = t
        if px * px + py * py > 144 or qx * qx + qy * qy > 144 or (px, py) == (qx, qy) or t in taken:
            continue
        taken.add(t)
        base.append(t)
    base = np.array(base, np.int64)
    P = np.zeros((BINS, TESTS, 4), np.int64)
    for k in range(BINS):
        for o in (0, 2):
            x, y = base[:, o], base[:, o + 1]
            P[k, :, o] = (x * C[k] - y * S[k] + 8192) >> 14
            P[k, :, o + 1] = (x * S[k] + y * C[k] + 8192) >> 14
    out = (P.astype(np.int8), C.astype(np.int32), S.astype(np.int32))
    for a in out:
        a.setflags(write=False)
    return out


_DY, _DX = np.meshgrid(np.arange(-R, R + 1), np.arange(-R, R + 1), indexing="ij")
_DISC = _DX * _DX + _DY * _DY <= R * R


def status_and_centre(x, y, h: int, w: int):
    """-> (status, cx, cy) of one float32 point."""
    x, y = np.float32(x), np.float32(y)
    if not (np.isfinite(x) and np.isfinite(y)) or abs(x) >= np.float32(2 ** 24) or abs(y) >= np.float32(2 ** 24):
        return 1, 0, 0
    cx, cy = int(np.rint(x)), int(np.rint(y))  # half to even
    if not (0 <= cx <= w - 1 and 0 <= cy <= h - 1):
        return 1, 0, 0
    return 0, cx, cy


def describe_point(img: np.ndarray, x, y):
    """-> (des uint32 (8,), bin, status)."""
    P, C, S = tables()
    h, w = img.shape
    des = np.zeros(WORDS, np.uint32)
    st, cx, cy = status_and_centre(x, y, h, w)
    if st:
        return des, 0, 1
    d = np.arange(-R, R + 1)
    patch = img[reflect(cy + d, h)][:, reflect(cx + d, w)].astype(np.int64)  # [dy + 15, dx + 15]
    m10 = int((_DX * patch)[_DISC].sum())
    m01 = int((_DY * patch)[_DISC].sum())
    score = m10 * C.astype(np.int64) + m01 * S.astype(np.int64)
    k = int(np.argmax(score))  # the first maximum
    box = np.zeros((27, 27), np.int64)  # [v + 13, u + 13]
    for j in range(5):
        for i in range(5):
            box += patch[j:j + 27, i:i + 27]
    T = P[k].astype(np.int64)
    bp = box[T[:, 1] + 13, T[:, 0] + 13]
    bq = box[T[:, 3] + 13, T[:, 2] + 13]
    bits = (bp < bq).astype(np.uint32)
    for t in np.flatnonzero(bits):
        des[t // 32] |= np.uint32(1) << np.uint32(t % 32)
    return des, k, 0


def describe(img: np.ndarray, pts):
    """-> (des uint32 (n, 8), bins int32 (n,), status uint8 (n,))."""
    img = np.ascontiguousarray(img, np.uint8)
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    n = len(pts)
    des, bins, status = np.zeros((n, WORDS), np.uint32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    for i, (x, y) in enumerate(pts):
        des[i], bins[i], status[i] = describe_point(img, x, y)
    return des, bins, status


_POP8 = np.array([bin(v).count("1") for v in range(256)], np.int64)


def hamming(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """uint32 (n, words), (m, words) -> int64 (n, m) bit differences."""
    a8 = np.ascontiguousarray(a, np.uint32).view(np.uint8)
    b8 = np.ascontiguousarray(b, np.uint32).view(np.uint8)
    out = np.zeros((len(a8), len(b8)), np.int64)
    for c in range(a8.shape[1]):
        out += _POP8[a8[:, c][:, None] ^ b8[:, c][None, :]]
    return out


# ---- shared test material -----------------------------------------------------------------------

def texture(h: int, w: int, seed: int = 0, smooth: int = 2) -> np.ndarray:
    """A box-smoothed random texture, uint8 (h, w)."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (h + 2 * smooth, w + 2 * smooth)).astype(np.float64)
    k = 2 * smooth + 1
    acc = np.zeros((h, w))
    for j in range(k):
        for i in range(k):
            acc += f[j:j + h, i:i + w]
    acc /= k * k
    acc = (acc - acc.min()) / max(acc.max() - acc.min(), 1e-9) * 255.0
    return np.rint(acc).astype(np.uint8)


def flat(h: int, w: int, v: int = 77) -> np.ndarray:
    return np.full((h, w), v, np.uint8)


def step_edge(h: int, w: int) -> np.ndarray:
    """Two grey levels split by a slanted edge: most box sums of a patch are equal."""
    ys, xs = np.mgrid[0:h, 0:w]
    return np.where(3 * xs + 2 * ys > (3 * w + 2 * h) // 2, 200, 40).astype(np.uint8)


def interior_points(h: int, w: int, n: int, seed: int = 1, margin: int = 20) -> np.ndarray:
    """Distinct integer points at least ``margin`` inside, float32 (n, 2) as (x, y)."""
    rng = np.random.default_rng(seed)
    xs = rng.integers(margin, w - margin, 4 * n)
    ys = rng.integers(margin, h - margin, 4 * n)
    p = np.unique(np.stack([xs, ys], 1), axis=0)
    rng.shuffle(p)
    assert len(p) >= n
    return p[:n].astype(np.float32)


def edge_points(h: int, w: int) -> np.ndarray:
    """Points that exercise the status rule, the rounding and the reflection of an h x w image."""
    big = float(2 ** 24)
    p = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (0, h // 2), (w - 1, h // 2), (w // 2, h - 1),
         (min(7, w - 1), min(3, h - 1)), (max(w - 8, 0), max(h - 4, 0)), (min(14, w - 1), min(14, h - 1)),
         (0.5, 0.5), (1.5, 2.5), (2.5, 1.5), (w / 2 + 0.5, h / 2 - 0.5), (0.49, 0.51),
         (-0.5, 0.0), (0.0, -0.5), (w - 0.5, 0.0), (0.0, h - 0.5), (-0.51, 0.0), (w - 0.49, h - 0.49), (-1.0, -1.0),
         (w, h), (float("nan"), 1.0), (1.0, float("nan")), (float("inf"), 0.0), (0.0, float("-inf")),
         (big, 0.0), (0.0, -big), (big - 1.0, 0.0), (-0.0, -0.0)]
    return np.array(p, np.float32)
