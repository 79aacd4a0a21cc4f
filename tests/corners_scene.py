"""Scenes and cases for the corner-detector tests: what the host build and the device are compared
with the restatement (``tests/corners_ref.py``) on."""

from __future__ import annotations

from functools import lru_cache

import numpy as np

from tests import corners_ref as R
from tests import klt_scene

QUALITY = 0.01


@lru_cache(maxsize=4)
def crop_image(h: int = 120, w: int = 160, seed: int = 8) -> np.ndarray:
    """The textured test image (shared: treat as read-only)."""
    return klt_scene.crop(klt_scene.base_image(h, w, seed), h, w)


def checkerboard(h: int = 64, w: int = 96, square: int = 8, lo: int = 20, hi: int = 220) -> np.ndarray:
    y, x = np.mgrid[:h, :w]
    return np.where(((x // square) + (y // square)) % 2 == 0, lo, hi).astype(np.uint8)


def rectangle(h: int = 60, w: int = 80, box=(20, 15, 55, 40)) -> np.ndarray:
    """A white rectangle [x0, x1) x [y0, y1) on black."""
    img = np.zeros((h, w), np.uint8)
    x0, y0, x1, y1 = box
    img[y0:y1, x0:x1] = 255
    return img


def hole_mask(h: int, w: int) -> np.ndarray:
    """Nonzero (with values other than 1) except a rectangular hole and the top rows."""
    m = np.full((h, w), 200, np.uint8)
    m[h // 3:2 * h // 3, w // 4:w // 2] = 0
    m[:5] = 0
    m[7, ::2] = 1
    return m


@lru_cache(maxsize=1)
def keep_sets() -> dict:
    """Keep-away sets for the 120 x 160 crop at d = 8: around the detector's own first corners."""
    img = crop_image()
    pts, _ = R.good_features(img, 40, QUALITY, 8.0)
    rng = np.random.default_rng(11)
    near = (pts + rng.uniform(-6, 6, pts.shape)).astype(np.float32)
    bad = near.copy()
    bad[::5, 0] = np.nan
    bad[1::7, 1] = np.inf
    bad[2::9] = -np.inf
    off = np.array([[-3.5, 10.0], [162.25, 50.0], [80.0, -4.0], [40.0, 125.5], [1e9, 1e9], [-1e30, 3.0]], np.float32)
    # exactly d from the strongest corners (not rejected), and one float32 step closer (rejected)
    exact = np.concatenate([pts[:6] + np.float32((8, 0)), pts[6:10] - np.float32((0, 8)),
                            np.nextafter(pts[10:14] + np.float32((8, 0)), np.float32(-1e9), dtype=np.float32)])
    return dict(near=near, nonfinite=bad, off_image=np.concatenate([off, near[:10]]), exact=exact.astype(np.float32),
                empty=np.zeros((0, 2), np.float32))


def cases() -> dict:
    """name -> dict(img, kw) with kw for ``corners_ref.good_features`` / ``corners.good_features``."""
    img = crop_image()
    h, w = img.shape
    ks = keep_sets()
    out = {}
    for bs in (3, 5, 7):
        out[f"crop_block{bs}"] = dict(img=img, kw=dict(min_distance=8.0, block_size=bs))
    for d in (0.0, 0.5, 1.0, 7.5, 30.0):
        out[f"crop_d{d:g}"] = dict(img=img, kw=dict(min_distance=d))
    for m in (1, 64, 65):
        out[f"crop_max{m}"] = dict(img=img, kw=dict(min_distance=8.0, max_corners=m))
    out["crop_mask_hole"] = dict(img=img, kw=dict(min_distance=8.0, mask=hole_mask(h, w)))
    out["crop_mask_zeros"] = dict(img=img, kw=dict(min_distance=8.0, mask=np.zeros((h, w), np.uint8)))
    for name, k in ks.items():
        out[f"crop_keep_{name}"] = dict(img=img, kw=dict(min_distance=8.0, keep=k))
    out["crop_keep_mask_block5_max30"] = dict(img=img, kw=dict(min_distance=7.5, keep=ks["near"], block_size=5,
                                                               mask=hole_mask(h, w), max_corners=30))
    out["checkerboard"] = dict(img=checkerboard(), kw=dict(min_distance=8.0))
    out["checkerboard_d0"] = dict(img=checkerboard(), kw=dict(min_distance=0.0))
    out["constant"] = dict(img=np.full((40, 50), 77, np.uint8), kw=dict(min_distance=8.0))
    out["rectangle"] = dict(img=rectangle(), kw=dict(min_distance=4.0, quality=0.1))
    out["odd_65x67_block7"] = dict(img=crop_image(65, 67, 9), kw=dict(min_distance=3.0, block_size=7))
    out["tiny_3x3"] = dict(img=(np.arange(9, dtype=np.uint8) * 29 % 251).reshape(3, 3), kw=dict(min_distance=1.0))
    out["thin_2x40"] = dict(img=crop_image(40, 40, 9)[:2], kw=dict(min_distance=1.0))
    return out


def kitti_case() -> dict:
    """The 376 x 1241 scene with 2000 keep-away points and room for 2000."""
    img = crop_image(376, 1241, 8)
    first, _ = R.good_features(img, 2000, QUALITY, 8.0)
    return dict(img=img, kw=dict(min_distance=8.0, keep=first, max_corners=2000))


def run_ref(case: dict, prepared: dict | None = None, key=None):
    """The restatement's result for a case -> (pts, resp), computed once per ``key`` in ``prepared``."""
    if prepared is not None and key in prepared:
        return prepared[key]
    kw = dict(case["kw"])
    kw.setdefault("quality", QUALITY)
    res = R.good_features(case["img"], **kw)
    if prepared is not None:
        prepared[key] = res
    return res


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
