"""The corner detector's restatement (``tests/corners_ref.py``) itself: the counts its prototype
found, the selection's properties, and its round-based form against the serial loop (no GPU)."""

import numpy as np
import pytest

from tests import corners_ref as R
from tests import corners_scene as S

D = 8.0


@pytest.fixture(scope="module")
def crop():
    return S.crop_image()


@pytest.fixture(scope="module")
def crop_cands(crop):
    return {bs: R.candidates(R.response(crop, bs // 2), S.QUALITY) for bs in (3, 5, 7)}


@pytest.mark.parametrize("block_size, n_cand, n_corners", [(3, 931, 173), (5, 597, 159), (7, 433, 147)])
def test_counts_on_the_crop_are_the_prototypes(crop, crop_cands, block_size, n_cand, n_corners):
    xy, r = crop_cands[block_size]
    assert len(xy) == n_cand
    pts, resp = R.good_features(crop, None, S.QUALITY, D, block_size=block_size)
    assert len(pts) == n_corners and pts.dtype == np.float32 and resp.dtype == np.float32
    assert (np.diff(resp.astype(np.float64)) <= 0).all()
    dd = ((pts[:, None].astype(np.float64) - pts[None].astype(np.float64)) ** 2).sum(2)
    dd[np.diag_indices(len(pts))] = np.inf
    assert dd.min() >= D * D


def test_order_is_response_descending_then_index(crop_cands, crop):
    xy, r = crop_cands[3]
    idx = xy[:, 1].astype(np.int64) * crop.shape[1] + xy[:, 0]
    key = list(zip((-r.astype(np.float64)).tolist(), idx.tolist()))
    assert key == sorted(key)
    assert xy[:, 0].min() >= 1 and xy[:, 0].max() <= crop.shape[1] - 2
    assert xy[:, 1].min() >= 1 and xy[:, 1].max() <= crop.shape[0] - 2


@pytest.mark.parametrize("name", ["near", "nonfinite", "off_image", "exact"])
def test_no_corner_is_within_d_of_a_keep_away_point(crop, name):
    keep = S.keep_sets()[name]
    pts, _ = R.good_features(crop, None, S.QUALITY, D, keep=keep)
    k = R.finite_keep(keep).astype(np.float64)
    dd = ((pts[:, None].astype(np.float64) - k[None]) ** 2).sum(2)
    assert len(pts) and dd.min() >= D * D
    free, _ = R.good_features(crop, None, S.QUALITY, D)
    assert len(pts) != len(free) or not np.array_equal(pts, free)


def test_a_point_exactly_d_away_does_not_reject(crop):
    free, _ = R.good_features(crop, None, S.QUALITY, D)
    at_d = free[:1] + np.float32((8, 0))
    pts, _ = R.good_features(crop, None, S.QUALITY, D, keep=at_d)
    assert (pts[0] == free[0]).all()
    closer = np.nextafter(at_d, np.float32(-1e9), dtype=np.float32)
    pts, _ = R.good_features(crop, None, S.QUALITY, D, keep=closer)
    assert not (pts == free[0]).all(1).any()


@pytest.mark.parametrize("m", [1, 64, 65, 172])
def test_prefix_property(crop, m):
    full, fr = R.good_features(crop, None, S.QUALITY, D)
    pts, r = R.good_features(crop, m, S.QUALITY, D)
    assert len(pts) == m
    np.testing.assert_array_equal(pts, full[:m])
    np.testing.assert_array_equal(r, fr[:m])


@pytest.mark.parametrize("d", [0.0, 0.5, 1.0, 1.5, 7.5, 8.0, 30.0])
@pytest.mark.parametrize("with_keep", [False, True])
def test_selection_equals_brute_force_and_rounds(crop_cands, d, with_keep):
    xy, _ = crop_cands[3]
    keep = S.keep_sets()["nonfinite"] if with_keep else None
    serial = R.select(xy, d, keep)
    np.testing.assert_array_equal(serial, R.select_brute(xy, d, keep))
    by_rounds, rounds = R.select_rounds(xy, d, keep)
    np.testing.assert_array_equal(serial, by_rounds)
    assert rounds >= 1
    if d == 0.0:
        assert len(serial) == len(xy)
    for m in (1, 17):
        np.testing.assert_array_equal(R.select(xy, d, keep, m), serial[:m])
        np.testing.assert_array_equal(R.select_rounds(xy, d, keep, m)[0], serial[:m])


def test_a_chain_takes_as_many_rounds_as_it_is_long():
    n = 64
    xy = np.stack([np.arange(n), np.zeros(n, np.int64)], 1)
    idx, rounds = R.select_rounds(xy, 1.5)
    np.testing.assert_array_equal(idx, np.arange(0, n, 2))
    np.testing.assert_array_equal(idx, R.select(xy, 1.5))
    assert rounds == n


def test_constant_image_has_no_corners():
    img = np.full((40, 50), 77, np.uint8)
    assert not R.response(img).any()
    pts, r = R.good_features(img, None, S.QUALITY, D)
    assert pts.shape == (0, 2) and r.shape == (0,)


def test_zero_mask_and_small_images_have_no_corners(crop):
    pts, _ = R.good_features(crop, None, S.QUALITY, D, mask=np.zeros(crop.shape, np.uint8))
    assert len(pts) == 0
    for shape in ((2, 40), (40, 2), (1, 1)):
        img = np.arange(shape[0] * shape[1], dtype=np.uint8).reshape(shape) * 37
        assert R.response(img).shape == shape
        assert len(R.good_features(img, None, S.QUALITY, 1.0)[0]) == 0


def test_mask_limits_the_maximum_and_the_candidates_not_the_neighbour_test(crop):
    mask = S.hole_mask(*crop.shape)
    resp = R.response(crop)
    xy, r = R.candidates(resp, S.QUALITY, mask)
    assert len(xy) and (mask[xy[:, 1], xy[:, 0]] != 0).all()
    thr = np.float64(np.float32(S.QUALITY)) * np.float64(resp[mask != 0].max())
    assert (r.astype(np.float64) > thr).all()
    # a masked-out neighbour with a larger response still suppresses
    for x, y in xy.tolist():
        assert (resp[y - 1:y + 2, x - 1:x + 2] <= resp[y, x]).all()
    assert r[0] <= resp[mask != 0].max()


def test_checkerboard_candidates_tie_and_come_in_index_order():
    img = S.checkerboard()
    xy, r = R.candidates(R.response(img), S.QUALITY)
    assert len(xy) == 308 and len(np.unique(r)) == 1
    idx = xy[:, 1].astype(np.int64) * img.shape[1] + xy[:, 0]
    assert (np.diff(idx) > 0).all()


def test_rectangle_corners_are_found_within_one_pixel():
    x0, y0, x1, y1 = 20, 15, 55, 40
    img = S.rectangle(box=(x0, y0, x1, y1))
    pts, _ = R.good_features(img, 4, 0.1, 4.0)
    assert len(pts) == 4
    want = np.array([[x0 - 0.5, y0 - 0.5], [x1 - 0.5, y0 - 0.5], [x0 - 0.5, y1 - 0.5], [x1 - 0.5, y1 - 0.5]])
    for c in want:
        assert np.abs(pts - c).max(1).min() <= 1.0, (c, pts)


def test_response_is_the_minimum_eigenvalue(crop):
    a, b, c = R.sums(crop, 1)
    resp = R.response_from_sums(a, b, c).astype(np.float64)
    M = np.stack([np.stack([a, b], -1), np.stack([b, c], -1)], -2).astype(np.float64)
    ev = np.linalg.eigvalsh(M[::7, ::5])[..., 0]
    np.testing.assert_allclose(resp[::7, ::5], ev, rtol=1e-5, atol=1e-3 * np.abs(ev).max() * 1e-3)
