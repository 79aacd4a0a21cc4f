"""The KLT contract's restatement (tests/klt_ref.py) against planted motion and the special points of
every status code (no GPU).

The planted pairs are crops of one ``sift_scene(texture=12)`` at integer offsets, so the true
motion is known exactly and is a fixed point of the iteration (the mismatch is zero there); the
stop rule is 0.01 px, the bound on a tracked point 0.1 px.  A test cannot pass by dropping points:
at least 90 % of the points whose window stays inside both images must be tracked.  The options
are the drop-in route's (r = 10, 4 levels, forward-backward check at 1 px): without the check a
37-pixel motion leaves a few percent of the corners of this texture converged elsewhere with
status 0, which is what the check is for."""

import numpy as np
import pytest

from tests import klt_ref as R
from tests import klt_scene as S

BOUND_PX = 0.1
MIN_TRACKED = 0.9


@pytest.mark.parametrize("shift", [(0, 0), (3, -2), (37, 11)])  # the last needs the pyramid
def test_planted_shift_is_recovered(shift):
    img0, img1, pts = S.planted(shift)
    h, w = img0.shape
    p1, status, err = R.track(img0, img1, pts, win_radius=10, levels=4, fb_thresh=1.0)
    inside = S.window_inside(pts, 10, h, w) & S.window_inside(pts + np.float32(shift), 10, h, w)
    assert inside.sum() >= 50
    ok = inside & (status == R.TRACKED)
    dev = np.abs(p1 - pts - np.float32(shift)).max(1)
    print(f"shift {shift}: {ok.sum()}/{inside.sum()} tracked, max deviation {dev[ok].max():.4f} px, "
          f"max err {err[ok].max():.4f}")
    assert ok.sum() >= MIN_TRACKED * inside.sum()
    assert dev[ok].max() <= BOUND_PX
    failed = status != R.TRACKED
    np.testing.assert_array_equal(p1[failed], pts[failed])
    assert (err[failed] == 0).all()


def test_small_shifts_need_no_check_and_the_large_one_needs_the_pyramid():
    img0, img1, pts = S.planted((3, -2))
    p1, status, _ = R.track(img0, img1, pts, win_radius=10, levels=4)
    assert (status == R.TRACKED).all() and np.abs(p1 - pts - np.float32((3, -2))).max() <= BOUND_PX
    img0, img1, pts = S.planted((37, 11))
    p1, status, _ = R.track(img0, img1, pts, win_radius=10, levels=1, fb_thresh=1.0)
    good = (status == R.TRACKED) & (np.abs(p1 - pts - np.float32((37, 11))).max(1) <= BOUND_PX)
    assert good.sum() < 0.2 * len(pts)


@pytest.fixture(scope="module")
def special():
    return S.special_scene(163, 241)


def _track(sc, sel, **kw):
    sel = np.atleast_1d(sel)
    return R.track(sc["img0"], sc["img1"], sc["pts"][sel], win_radius=15, levels=3, **kw)


def test_flat_border_pushed_out_and_nan_points(special):
    ix = special["idx"]
    sel = [ix["flat"], ix["border"], ix["pushed"], ix["nan"]]
    p1, status, err = _track(special, sel)
    assert status.tolist() == [R.DEGENERATE, R.START_OUTSIDE, R.LEFT_IMAGE, R.BAD_INPUT]
    np.testing.assert_array_equal(S.bits(p1), S.bits(special["pts"][sel]))  # a failed point keeps p0, NaN included
    assert (err == 0).all()
    # the pushed-out point is a good track while the window is smaller
    p1, status, _ = R.track(special["img0"], special["img1"], special["pts"][[ix["pushed"]]], win_radius=7, levels=3)
    assert status[0] == R.TRACKED and np.abs(p1[0] - special["pts"][ix["pushed"]] - np.float32(S.SPECIAL_SHIFT)).max() <= BOUND_PX


def test_occluder_is_caught_by_the_forward_backward_check_only(special):
    occ = special["idx"]["occluded"]
    _, plain, err = _track(special, occ)
    assert (plain == R.TRACKED).all() and err.min() > 8.0  # a confident track of the wrong texture
    p1, fb, err_fb = _track(special, occ, fb_thresh=1.0)
    assert (fb == R.FB_FAILED).all()
    np.testing.assert_array_equal(p1, special["pts"][occ])
    assert (err_fb == 0).all()
    _, me, _ = _track(special, occ, max_err=8.0)
    assert (me == R.ERR_ABOVE).all()
    # the check leaves good tracks alone
    img0, img1, pts = S.planted((3, -2))
    a = R.track(img0, img1, pts[:20], win_radius=10, levels=4)
    b = R.track(img0, img1, pts[:20], win_radius=10, levels=4, fb_thresh=1.0)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_a_guess_starts_the_search_and_a_bad_one_is_bad_input(special):
    img0, img1, pts = S.planted((37, 11))
    pts = pts[:20]
    g = pts + np.float32((36, 12))
    p1, status, _ = R.track(img0, img1, pts, guess=g, win_radius=10, levels=1)  # one level: the guess alone bridges it
    assert (status == R.TRACKED).all() and np.abs(p1 - pts - np.float32((37, 11))).max() <= BOUND_PX
    g[3, 1] = np.inf
    _, status, _ = R.track(img0, img1, pts, guess=g, win_radius=10, levels=1)
    assert status[3] == R.BAD_INPUT and (np.delete(status, 3) == R.TRACKED).all()


def test_levels_clamp_to_what_the_image_allows():
    img = S.special_scene(163, 241)["img0"]
    assert R.level_sizes(163, 241, 8, 10) == [(163, 241), (82, 121), (41, 61)]  # the next would be 21 x 31 < 23
    assert R.level_sizes(163, 241, 8, 1) == [(163, 241), (82, 121), (41, 61), (21, 31), (11, 16), (6, 8)]
    assert R.level_sizes(160, 240, 2, 10) == [(160, 240), (80, 120)]
    assert R.level_sizes(20, 20, 4, 10) == [(20, 20)]  # L_eff is at least 1
    assert [lv.shape for lv in R.pyramid(img, 8, 10)] == R.level_sizes(163, 241, 8, 10)
    sc = S.special_scene(163, 241)
    a = R.track(sc["img0"], sc["img1"], sc["pts"][:30], win_radius=10, levels=8)
    b = R.track(sc["img0"], sc["img1"], sc["pts"][:30], win_radius=10, levels=3)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    # an image too small for one window: the call runs, every point is 1
    tiny = np.zeros((22, 40), np.uint8)
    _, status, _ = R.track(tiny, tiny, [[11, 20], [5, 5]], win_radius=10, levels=3)
    assert (status == R.START_OUTSIDE).all()


def test_pyramid_is_the_5x5_binomial_with_reflection():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (9, 12), dtype=np.uint8)
    k = np.array([1, 4, 6, 4, 1])
    pad = np.pad(img.astype(np.int64), 2, mode="reflect")  # numpy's reflect does not repeat the edge
    want = np.zeros((5, 6), np.int64)
    for y in range(5):
        for x in range(6):
            want[y, x] = (np.outer(k, k) * pad[2 * y:2 * y + 5, 2 * x:2 * x + 5]).sum()
    np.testing.assert_array_equal(R.pyr_down(img), (want + 128) >> 8)
    assert R.pyr_down(np.full((7, 7), 200, np.uint8)).tolist() == [[200] * 4] * 4
