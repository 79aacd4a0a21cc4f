"""The corner detector's contract (``include/vo_hip.h``) restated literally in
numpy: Sobel gradients of a uint8 image, integer block sums, the minimum-eigenvalue response, the
candidate test, the order and the sequential selection loop.  What ``csrc/corners_math.h`` and
``csrc/corners.hip`` compute must equal this bit for bit.

Every sum over a block is an integer; the response is three double operations rounded once each and
one rounding to float32, which numpy performs as the contract says.
"""

from __future__ import annotations

import numpy as np


def reflect(i, n: int) -> np.ndarray:
    """Reflection without repeating the edge (-1 -> 1, n -> n - 2), total for any n >= 1."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    m = np.mod(i, p)
    return np.where(m >= n, p - m, m)


def gradients(img: np.ndarray):
    """-> (gx, gy) int32 (h, w): the 3 x 3 Sobel derivatives at every pixel, the image reflected."""
    I = np.asarray(img).astype(np.int32)
    h, w = I.shape
    ys, xs = np.arange(h), np.arange(w)

    def at(dx, dy):
        return I[reflect(ys + dy, h)][:, reflect(xs + dx, w)]

    gx = (at(1, -1) + 2 * at(1, 0) + at(1, 1)) - (at(-1, -1) + 2 * at(-1, 0) + at(-1, 1))
    gy = (at(-1, 1) + 2 * at(0, 1) + at(1, 1)) - (at(-1, -1) + 2 * at(0, -1) + at(1, -1))
    return gx, gy


def block_sum(P: np.ndarray, k: int) -> np.ndarray:
    """Sum of the int32 field ``P`` over the (2k+1)^2 block at every pixel, ``P`` read at reflected indices."""
    h, w = P.shape
    ys, xs = np.arange(h), np.arange(w)
    rows = np.zeros_like(P)
    for i in range(-k, k + 1):
        rows = rows + P[:, reflect(xs + i, w)]
    out = np.zeros_like(P)
    for j in range(-k, k + 1):
        out = out + rows[reflect(ys + j, h)]
    return out


def sums(img: np.ndarray, k: int):
    gx, gy = gradients(img)
    return block_sum(gx * gx, k), block_sum(gx * gy, k), block_sum(gy * gy, k)


def response_from_sums(a, b, c) -> np.ndarray:
    d = a.astype(np.int64) - c.astype(np.int64)
    b64 = b.astype(np.int64)
    q = d * d + 4 * (b64 * b64)
    tr = (a + c).astype(np.float64)  # int32: |a + c| <= 2 * 49 * 1020^2 < 2^31
    return (0.5 * (tr - np.sqrt(q.astype(np.float64)))).astype(np.float32)


def response(img: np.ndarray, block_radius: int = 1) -> np.ndarray:
    """The response map, (h, w) float32, defined at every pixel."""
    assert block_radius in (1, 2, 3)
    return response_from_sums(*sums(img, block_radius))


def candidates(resp: np.ndarray, quality: float, mask=None):
    """-> (xy (n, 2) int32, resp (n,) float32) in the contract's order: response descending, ties
    by y * w + x ascending."""
    h, w = resp.shape
    none = np.zeros((0, 2), np.int32), np.zeros(0, np.float32)
    m = np.ones((h, w), bool) if mask is None else np.asarray(mask) != 0
    if not m.any():
        return none
    rmax = resp[m].max()
    if not rmax > 0 or h < 3 or w < 3:
        return none
    thr = np.float64(np.float32(quality)) * np.float64(rmax)
    c = resp[1:-1, 1:-1]
    ok = m[1:-1, 1:-1] & (c.astype(np.float64) > thr)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                ok &= c >= resp[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
    ys, xs = np.nonzero(ok)
    ys, xs = ys + 1, xs + 1
    r = resp[ys, xs]
    order = np.lexsort((ys * w + xs, -r.astype(np.float64)))
    return np.stack([xs[order], ys[order]], 1).astype(np.int32), r[order]


def finite_keep(keep) -> np.ndarray:
    if keep is None:
        return np.zeros((0, 2), np.float32)
    k = np.asarray(keep, np.float32).reshape(-1, 2)
    return k[np.isfinite(k).all(1)]


def keep_rejects(xy: np.ndarray, keep, d: float) -> np.ndarray:
    """Per candidate: some finite keep-away point has dx*dx + dy*dy < d2, all in double."""
    k = finite_keep(keep).astype(np.float64)
    d2 = np.float64(np.float32(d)) * np.float64(np.float32(d))
    out = np.zeros(len(xy), bool)
    p = np.asarray(xy).astype(np.float64)
    for s in range(0, len(k), 256):
        dx = p[:, None, 0] - k[None, s:s + 256, 0]
        dy = p[:, None, 1] - k[None, s:s + 256, 1]
        out |= ((dx * dx + dy * dy) < d2).any(1)
    return out


def select(xy, d: float, keep=None, max_corners=None) -> np.ndarray:
    """The sequential selection loop over candidates already in order -> accepted rows, in order of
    acceptance.  A grid of ceil(d)-sized cells only finds the accepted corners near a candidate; the
    test itself is the contract's."""
    xy = np.asarray(xy, np.int64).reshape(-1, 2)
    n = len(xy)
    limit = n if max_corners is None else int(max_corners)
    d = np.float32(d)
    d2 = np.float64(d) * np.float64(d)
    if n == 0:
        return np.zeros(0, np.int64)
    rejected = keep_rejects(xy, keep, d)
    s = max(int(np.ceil(d)), 1)
    lo = xy.min(0)
    cells = (xy - lo) // s
    grid: dict = {}
    out = []
    for i in range(n):
        if len(out) >= limit:
            break
        if rejected[i]:
            continue
        cx, cy = int(cells[i, 0]), int(cells[i, 1])
        x, y = int(xy[i, 0]), int(xy[i, 1])
        ok = True
        for gy in (cy - 1, cy, cy + 1):
            for gx in (cx - 1, cx, cx + 1):
                for (ax, ay) in grid.get((gx, gy), ()):
                    if np.float64((x - ax) * (x - ax) + (y - ay) * (y - ay)) < d2:
                        ok = False
                        break
                if not ok:
                    break
            if not ok:
                break
        if ok:
            out.append(i)
            grid.setdefault((cx, cy), []).append((x, y))
    return np.asarray(out, np.int64)


def select_brute(xy, d: float, keep=None, max_corners=None) -> np.ndarray:
    """The same loop with every accepted corner tested: O(n^2), no grid."""
    xy = np.asarray(xy, np.int64).reshape(-1, 2)
    limit = len(xy) if max_corners is None else int(max_corners)
    d2 = np.float64(np.float32(d)) * np.float64(np.float32(d))
    rejected = keep_rejects(xy, keep, d)
    out: list = []
    for i in range(len(xy)):
        if len(out) >= limit:
            break
        if rejected[i]:
            continue
        if out:
            dd = ((xy[out] - xy[i]) ** 2).sum(1).astype(np.float64)
            if (dd < d2).any():
                continue
        out.append(i)
    return np.asarray(out, np.int64)


def select_rounds(xy, d: float, keep=None, max_corners=None):
    """The selection as the device runs it -> (accepted rows, rounds): the keep-away set rejects at
    once; then per round an undecided candidate whose closer-than-d neighbours of higher rank are all
    rejected is accepted, and one with an accepted such neighbour is rejected; the accepted rows in
    rank order, cut at the limit.  O(n^2) pairs: for the tests' small sets."""
    xy = np.asarray(xy, np.int64).reshape(-1, 2)
    n = len(xy)
    limit = n if max_corners is None else int(max_corners)
    d2 = np.float64(np.float32(d)) * np.float64(np.float32(d))
    dd = ((xy[:, None] - xy[None]) ** 2).sum(2).astype(np.float64)
    near = (dd < d2) & (np.arange(n)[None] < np.arange(n)[:, None])  # near[i, j]: j outranks i and is too close
    UNDECIDED, ACCEPTED, REJECTED = 0, 1, 2
    state = np.where(keep_rejects(xy, keep, d), REJECTED, UNDECIDED)
    rounds = 0
    while (state == UNDECIDED).any():
        rounds += 1
        und = state == UNDECIDED
        has_acc = (near & (state == ACCEPTED)[None]).any(1)
        has_und = (near & und[None]).any(1)
        new = state.copy()
        new[und & has_acc] = REJECTED
        new[und & ~has_acc & ~has_und] = ACCEPTED
        state = new
    return np.flatnonzero(state == ACCEPTED)[:limit], rounds


def good_features(img, max_corners=None, quality=0.01, min_distance=8.0, mask=None, block_size=3, keep=None,
                  info: dict | None = None):
    """-> (pts (N, 2) float32, resp (N,) float32) as ``vo_good_features`` defines them."""
    assert block_size in (3, 5, 7)
    xy, r = candidates(response(img, block_size // 2), quality, mask)
    idx = select(xy, min_distance, keep, max_corners)
    if info is not None:
        info["candidates"] = len(xy)
    return xy[idx].astype(np.float32), r[idx]
