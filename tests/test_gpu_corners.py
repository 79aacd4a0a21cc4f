"""vo_good_features / vo_corner_response / vo_corner_select on the MI355X against the restatement
(tests/corners_ref.py), bit for bit: response maps equal as uint32 bits, corners, responses and
counts equal.  Shapes sit below, at and above the response kernel's 64 x 16 tile; the selection is
driven through chains as long as the list, ties, one shared cell, the grid's corners and both sides
of the one-workgroup threshold (1024 candidates); the pyramid cache never changes a result."""

import numpy as np
import pytest

from tests import corners_ref as R
from tests import corners_scene as S
from visualodometry_amd import corners, klt

pytestmark = pytest.mark.gpu

CASES = S.cases()
_PREPARED = {}


def ref(name):
    return S.run_ref(CASES[name], _PREPARED, name)


def gpu(ctx, c, **extra):
    kw = dict(c["kw"])
    kw.setdefault("quality", S.QUALITY)
    kw.setdefault("max_corners", None)
    kw.update(extra)
    return corners.good_features(c["img"], ctx=ctx, **kw)


def assert_same(got, want):
    assert len(got[0]) == len(want[0])
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(S.bits(got[1]), S.bits(want[1]))
    assert got[0].dtype == np.float32 and got[0].shape == (len(want[0]), 2) and got[1].dtype == np.float32


def _image(h, w, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    if h * w > 64:  # saturated steps: the largest gradients and sums
        img[: h // 2, : w // 3] = np.where((np.add.outer(np.arange(h // 2), np.arange(w // 3)) % 2) == 0, 0, 255)
    return img


SHAPES = [(3, 3), (1, 40), (40, 2), (17, 23), (15, 63), (16, 64), (17, 65), (16, 65), (17, 64), (1, 1), (2, 2),
          (4, 129), (33, 5)]


@pytest.mark.parametrize("h, w", SHAPES)
@pytest.mark.parametrize("block_size", [3, 5, 7])
def test_response_map_bit_parity(ctx, h, w, block_size):
    img = _image(h, w, 100 * h + w)
    got = corners.response(img, block_size, ctx=ctx)
    np.testing.assert_array_equal(S.bits(got), S.bits(R.response(img, block_size // 2)))


def test_response_map_of_the_crop_and_a_saturated_image(ctx):
    img = S.crop_image()
    for bs in (3, 7):
        np.testing.assert_array_equal(S.bits(corners.response(img, bs, ctx=ctx)), S.bits(R.response(img, bs // 2)))
    sat = S.checkerboard(70, 131, 1, 0, 255)
    np.testing.assert_array_equal(S.bits(corners.response(sat, 7, ctx=ctx)), S.bits(R.response(sat, 3)))


@pytest.mark.parametrize("name", list(CASES))
def test_good_features_bit_parity(ctx, name):
    assert_same(gpu(ctx, CASES[name]), ref(name))


def test_stats_report_the_candidates_and_the_rounds(ctx):
    got = gpu(ctx, CASES["crop_block3"])
    st = corners.last_stats(ctx)
    xy, _ = R.candidates(R.response(S.crop_image()), S.QUALITY)
    assert st["candidates"] == len(xy) == 931 and st["accepted"] == len(got[0]) == 173
    assert 1 <= st["rounds"] <= R.select_rounds(xy, 8.0)[1] and st["cell_side"] == 8


def test_prefix_property(ctx):
    full = gpu(ctx, CASES["crop_block3"])
    for m in (1, 64, 65, 172, 173, 5000):
        got = gpu(ctx, CASES["crop_block3"], max_corners=m)
        assert_same(got, (full[0][:m], full[1][:m]))


def test_kitti_size_scene_with_keep_away_points(ctx):
    c = S.kitti_case()
    want = S.run_ref(c)
    assert len(want[0]) == 2000
    assert_same(gpu(ctx, c), want)
    st = corners.last_stats(ctx)
    assert st["candidates"] == 22946 and st["accepted"] == 2000


def ref_select(xy, resp, d, keep=None, m=None):
    order = np.lexsort((np.arange(len(resp)), -np.asarray(resp, np.float64)))
    return order[R.select(np.asarray(xy)[order], d, keep, m)]


def check_select(ctx, xy, resp, d, keep=None, m=None):
    got = corners.select(xy, resp, d, m, keep, ctx=ctx)
    want = ref_select(xy, resp, d, keep, m)
    np.testing.assert_array_equal(got, want)
    return got


@pytest.mark.parametrize("equal", [False, True])
def test_select_chain_as_long_as_the_list(ctx, equal):
    n = 4096
    xy = np.stack([np.arange(n), np.full(n, 7)], 1).astype(np.int32)
    resp = np.full(n, 5.0, np.float32) if equal else np.arange(n, 0, -1).astype(np.float32)
    got = check_select(ctx, xy, resp, 1.5)
    np.testing.assert_array_equal(got, np.arange(0, n, 2))
    assert corners.last_stats(ctx)["rounds"] >= 1
    np.testing.assert_array_equal(check_select(ctx, xy, resp, 1.5, m=100), np.arange(0, 200, 2))
    # the chain run from the far end: the order is the responses', not the rows'
    got = check_select(ctx, xy, resp[::-1].copy(), 1.5)
    if not equal:
        np.testing.assert_array_equal(got, np.arange(n - 1, 0, -2))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1024, 1025])
def test_select_counts_around_the_wave_and_the_workgroup(ctx, n):
    rng = np.random.default_rng(n)
    side = max(int(np.sqrt(n) * 3), 4)
    xy = rng.integers(-side, side, (n, 2)).astype(np.int32)
    resp = rng.integers(-3, 40, n).astype(np.float32) / 4  # many ties, zeros and negatives
    keep = rng.uniform(-side, side, (7, 2)).astype(np.float32)
    for d in (0.0, 1.0, 2.5, 6.0):
        check_select(ctx, xy, resp, d)
        check_select(ctx, xy, resp, d, keep)
        check_select(ctx, xy, resp, d, keep, m=max(n // 3, 1))


def test_select_many_candidates_with_keep_away_points(ctx):
    rng = np.random.default_rng(3)
    xy = rng.integers(0, 200, (3000, 2)).astype(np.int32)
    resp = rng.uniform(0.1, 10, 3000).astype(np.float32)
    keep = rng.uniform(-20, 220, (60, 2)).astype(np.float32)
    keep[::9] = np.nan
    for d in (0.5, 3.0, 5.0, 40.0):
        check_select(ctx, xy, resp, d, keep)


def test_select_candidates_sharing_one_cell_and_one_pixel(ctx):
    rng = np.random.default_rng(4)
    xy = rng.integers(10, 14, (200, 2)).astype(np.int32)  # 16 pixels, most of them several times
    resp = rng.uniform(1, 2, 200).astype(np.float32)
    assert len(check_select(ctx, xy, resp, 8.0)) == 1
    assert len(check_select(ctx, xy, resp, 0.0)) == 200
    assert len(check_select(ctx, xy, resp, 0.5)) == len(np.unique(xy, axis=0))
    check_select(ctx, xy, resp, 2.0)


def test_select_coordinates_at_the_grids_corners(ctx):
    big = 1 << 24
    corner = np.array([[-big, -big], [big, big], [-big, big], [big, -big], [0, 0]], np.int32)
    xy = np.concatenate([corner, corner - np.sign(corner) * np.int32((1, 0)),  # one pixel inwards along x
                         [[big - 2, big], [-big, -big + 3], [1, 1]]]).astype(np.int32)
    resp = np.arange(len(xy), 0, -1).astype(np.float32)
    keep = np.array([[big + 0.5, big], [-big - 900.0, -big], [3e9, 0], [0.25, 0.25]], np.float32)
    for d in (0.0, 1.0, 2.5, 1024.0):
        check_select(ctx, xy, resp, d)
        check_select(ctx, xy, resp, d, keep)
    # every cell of a small grid occupied at its corners
    g = np.array([[x, y] for y in (0, 7, 8, 15, 16) for x in (0, 7, 8, 15, 16)], np.int32)
    check_select(ctx, g, np.ones(len(g), np.float32), 8.0)
    check_select(ctx, g, np.ones(len(g), np.float32), 7.5, keep=np.array([[8.0, 8.0]], np.float32))


def test_cache_hit_gives_the_same_corners_and_leaves_the_cache_intact(ctx):
    from tests import klt_scene

    img0, img1, pts = klt_scene.planted((3, -2), h=163, w=241, seed=8, n=40, border=30)
    t0, t1 = 0x7C0FFEE0, 0x7C0FFEE1
    first = klt.track(img0, img1, pts, win_radius=7, levels=3, tags=(t0, t1), ctx=ctx)
    want = R.good_features(img1, 300, S.QUALITY, 6.0, keep=first[0])
    miss = corners.good_features(img1, 300, S.QUALITY, 6.0, keep=first[0], tag=0x7C0FFEE9, ctx=ctx)  # never cached
    hit = corners.good_features(None, 300, S.QUALITY, 6.0, keep=first[0], tag=t1, shape=img1.shape, ctx=ctx)
    hit_with_image = corners.good_features(img1, 300, S.QUALITY, 6.0, keep=first[0], tag=t1, ctx=ctx)
    for got in (miss, hit, hit_with_image):
        assert_same(got, want)
    with pytest.raises(Exception, match="not in the pyramid cache"):
        corners.good_features(None, 300, tag=0x7C0FFEE9, shape=img1.shape, ctx=ctx)  # the miss created no entry
    for im0, im1 in ((None, img1), (img0, None)):  # both entries still serve the tracker
        again = klt.track(im0, im1, pts, win_radius=7, levels=3, tags=(t0, t1), ctx=ctx)
        for a, b in zip(first, again):
            np.testing.assert_array_equal(a, b)


def test_cv2_style_call(ctx):
    img = S.crop_image()
    got = corners.goodFeaturesToTrack(img, 50, 0.01, 8, ctx=ctx)
    assert got.shape == (50, 1, 2) and got.dtype == np.float32
    np.testing.assert_array_equal(got[:, 0], ref("crop_block3")[0][:50])
    unlimited = corners.goodFeaturesToTrack(img, 0, 0.01, 8, blockSize=5, ctx=ctx)
    np.testing.assert_array_equal(unlimited[:, 0], ref("crop_block5")[0])
    masked = corners.goodFeaturesToTrack(img, -1, 0.01, 8, mask=S.hole_mask(*img.shape), ctx=ctx)
    np.testing.assert_array_equal(masked[:, 0], ref("crop_mask_hole")[0])
    none = corners.goodFeaturesToTrack(np.full((30, 30), 9, np.uint8), 10, 0.01, 8, ctx=ctx)
    assert none.shape == (0, 1, 2) and none.dtype == np.float32
