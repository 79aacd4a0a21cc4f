"""Scenes for the KLT tests: crops of one textured image at integer offsets (planted, exactly known
motion), corner points to track, and the special points every status code needs."""

from __future__ import annotations

from functools import lru_cache

import numpy as np

from visualodometry_amd.synthetic import sift_scene

MARGIN = 48  # the base image is this much larger on every side than a crop


@lru_cache(maxsize=8)
def base_image(h: int, w: int, seed: int = 3) -> np.ndarray:
    """The textured image the crops are cut from (shared: treat as read-only)."""
    return sift_scene(h + 2 * MARGIN, w + 2 * MARGIN, seed=seed, n_blobs=max(40, h * w // 1200),
                      n_boxes=max(10, h * w // 8000), texture=12)


def crop(base: np.ndarray, h: int, w: int, shift=(0, 0)) -> np.ndarray:
    """The h x w view whose content sits ``shift`` = (sx, sy) pixels further right / down than in
    ``crop(base, h, w)``: a point at p there is at p + shift here."""
    sx, sy = shift
    assert abs(sx) <= MARGIN and abs(sy) <= MARGIN
    return np.ascontiguousarray(base[MARGIN - sy:MARGIN - sy + h, MARGIN - sx:MARGIN - sx + w])


def corner_points(img: np.ndarray, n: int, border: int, min_dist: int = 7) -> np.ndarray:
    """The ``n`` strongest local maxima of the minimum-eigenvalue corner response (7 x 7 sums of
    central differences), at least ``border`` from the edge -> (n, 2) float32 (x, y)."""
    from scipy.ndimage import maximum_filter, uniform_filter

    I = img.astype(np.float64)
    gx = np.zeros_like(I)
    gy = np.zeros_like(I)
    gx[:, 1:-1] = I[:, 2:] - I[:, :-2]
    gy[1:-1] = I[2:] - I[:-2]
    a, b, c = uniform_filter(gx * gx, 7), uniform_filter(gx * gy, 7), uniform_filter(gy * gy, 7)
    resp = 0.5 * (a + c - np.sqrt((a - c) ** 2 + 4 * b * b))
    peak = (resp == maximum_filter(resp, 2 * min_dist + 1))
    peak[:border] = peak[-border:] = False
    peak[:, :border] = peak[:, -border:] = False
    ys, xs = np.nonzero(peak)
    order = np.argsort(-resp[ys, xs], kind="stable")[:n]
    assert len(order) == n, f"only {len(order)} corners for {n} points"
    return np.stack([xs[order], ys[order]], 1).astype(np.float32)


def window_inside(p: np.ndarray, r: int, h: int, w: int) -> np.ndarray:
    """Whether the (2r+1)^2 window at each point, with its +1 taps, lies inside an h x w image."""
    q = np.floor(np.asarray(p, np.float32) - np.float32(r))
    return (q[:, 0] >= 0) & (q[:, 1] >= 0) & (q[:, 0] <= w - 2 * r - 2) & (q[:, 1] <= h - 2 * r - 2)


def paste_flat(img: np.ndarray, cx: int, cy: int, half: int, value: int = 128) -> None:
    img[max(cy - half, 0):cy + half + 1, max(cx - half, 0):cx + half + 1] = value


def paste_occluder(img: np.ndarray, base: np.ndarray, cx: int, cy: int, half: int, src=(7, 5)) -> None:
    """Covers the square around (cx, cy) with texture from elsewhere in the base image."""
    y0, y1 = max(cy - half, 0), min(cy + half + 1, img.shape[0])
    x0, x1 = max(cx - half, 0), min(cx + half + 1, img.shape[1])
    img[y0:y1, x0:x1] = base[src[1] + y0:src[1] + y1, src[0] + x0:src[0] + x1][::-1, ::-1]


def planted(shift, h: int = 376, w: int = 1241, seed: int = 8, n: int = 60, border: int = 100):
    """-> (img0, img1, pts): ``n`` corners of a crop and the crop ``shift`` further on.  ``border``
    100 keeps the r = 10 window of a point inside at every one of 4 levels (8 (r + 1) = 88)."""
    base = base_image(h, w, seed)
    img0 = crop(base, h, w)
    return img0, crop(base, h, w, shift), corner_points(img0, n, border)


SPECIAL_SHIFT = (3, -2)
N_OCCLUDED = 12


def special_scene(h: int, w: int, n: int = 200, seed: int = 8) -> dict:
    """A crop pair moved by SPECIAL_SHIFT with ``n`` points, the first of them special:
    N_OCCLUDED corners covered by foreign texture in the second image (the forward-backward
    check's case), then a point in a flat square, one at the left border, one whose window the
    motion pushes out at the right (for r = 15), one NaN; the rest corners, some of them near the
    border.  ``idx`` names the special points."""
    base = base_image(h, w, seed)
    img0 = crop(base, h, w).copy()
    img1 = crop(base, h, w, SPECIAL_SHIFT).copy()
    fx, fy = w // 2, h // 2
    paste_flat(img0, fx, fy, 18)
    paste_flat(img1, fx + SPECIAL_SHIFT[0], fy + SPECIAL_SHIFT[1], 18)
    occ = corner_points(img0, N_OCCLUDED, 24, min_dist=7)
    for p in occ:
        paste_occluder(img1, base, int(p[0]) + SPECIAL_SHIFT[0], int(p[1]) + SPECIAL_SHIFT[1], 22)
    extra = np.array([[fx, fy], [4.0, h / 2], [w - 18.0, h / 2 + 0.25], [np.nan, 5.0]], np.float32)
    rest = corner_points(img0, n - len(extra), 2, min_dist=3)
    rest = rest[~(rest[:, None, :] == occ[None]).all(2).any(1)][:n - N_OCCLUDED - len(extra)]
    pts = np.concatenate([occ, extra, rest]).astype(np.float32)
    assert len(pts) == n
    k = N_OCCLUDED
    return dict(img0=img0, img1=img1, pts=pts, shift=SPECIAL_SHIFT,
                idx=dict(occluded=np.arange(k), flat=k, border=k + 1, pushed=k + 2, nan=k + 3,
                         corners=np.arange(k + 4, n)))


def parity_cases() -> dict:
    """name -> dict(img0, img1, pts, kw): what the host build and the device are compared with the
    restatement on.  Odd and even extents; radii 1 (fewer pixels than lanes), 7 and 10 (a partial
    last pixel per lane) and 15 (the cap); 1, 3 and 8 (clamped) levels; each flag alone and both;
    max_err; a KITTI-size pair."""
    odd = special_scene(163, 241)
    even = special_scene(160, 240, seed=9)
    rng = np.random.default_rng(5)

    def case(sc, n, **kw):
        pts = sc["pts"][:n]
        if kw.pop("with_guess", False):
            g = pts + np.float32(sc["shift"]) + rng.uniform(-1.5, 1.5, pts.shape).astype(np.float32)
            g[::17] = np.inf  # a bad guess is a bad input
            kw["guess"] = g
        return dict(img0=sc["img0"], img1=sc["img1"], pts=pts, kw=kw)

    cases = {
        "odd_r10_l3_n200": case(odd, 200, win_radius=10, levels=3),
        "odd_r1": case(odd, 65, win_radius=1, levels=3),
        "odd_r7": case(odd, 65, win_radius=7, levels=3),
        "odd_r15": case(odd, 65, win_radius=15, levels=3),
        "odd_l1": case(odd, 65, win_radius=10, levels=1),
        "odd_l8_clamped": case(odd, 65, win_radius=10, levels=8),
        "odd_guess": case(odd, 65, win_radius=10, levels=3, with_guess=True),
        "odd_fb": case(odd, 65, win_radius=15, levels=3, fb_thresh=1.0),
        "odd_guess_fb": case(odd, 65, win_radius=7, levels=3, fb_thresh=0.5, with_guess=True),
        "odd_max_err": case(odd, 65, win_radius=15, levels=3, max_err=8.0),
        "even_r10_l3": case(even, 65, win_radius=10, levels=3),
        "even_r15_fb": case(even, 65, win_radius=15, levels=2, fb_thresh=1.0, max_iters=10, eps=0.03),
    }
    img0, img1, pts = planted((37, 11), n=300, border=6)
    cases["kitti_r10_l4_fb"] = dict(img0=img0, img1=img1, pts=pts, kw=dict(win_radius=10, levels=4, fb_thresh=1.0))
    return cases


def run_ref(case: dict, prepared: dict | None = None):
    from tests import klt_ref

    return klt_ref.track(case["img0"], case["img1"], case["pts"], prepared=prepared, **case["kw"])


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
