"""vo_klt_track / vo_klt_pyramid on the MI355X against the restatement (tests/klt_ref.py), bit for
bit: ``status`` equal, ``pts1`` and ``err`` equal as uint32 bits, pyramids byte-equal.  The cases
(tests/klt_scene.py: parity_cases) cover odd and even extents, radii 1 / 7 / 10 / 15, 1 / 3 / 8
(clamped) levels, each flag alone and both, max_err and a KITTI-size pair; the point counts cover
one wave, a workgroup short of, at and past four waves, and many workgroups.  The pyramid cache
never changes a result."""

import numpy as np
import pytest

from tests import klt_ref as R
from tests import klt_scene as S
from visualodometry_amd import klt

pytestmark = pytest.mark.gpu

CASES = S.parity_cases()
_REF = {}
_PREPARED = {}


def ref(name):
    """The restatement's result of a case, computed once per module."""
    if name not in _REF:
        _REF[name] = S.run_ref(CASES[name], _PREPARED)
    return _REF[name]


def gpu(ctx, c, n=None, **extra):
    kw = dict(c["kw"])
    if n is not None and "guess" in kw:
        kw["guess"] = kw["guess"][:n]
    return klt.track(c["img0"], c["img1"], c["pts"][:n], ctx=ctx, **kw, **extra)


def assert_same(got, want, n=None):
    np.testing.assert_array_equal(got[1], want[1][:n])
    np.testing.assert_array_equal(S.bits(got[0]), S.bits(want[0][:n]))
    np.testing.assert_array_equal(S.bits(got[2]), S.bits(want[2][:n]))


def test_the_cases_are_informative():
    """Asserted in the restatement first: every status code occurs in at least one case, and the
    plain case tracks most of its points."""
    seen = np.zeros(7, np.int64)
    for name in CASES:
        seen += np.bincount(ref(name)[1], minlength=7)
    assert (seen > 0).all(), seen
    assert (ref("odd_r10_l3_n200")[1] == R.TRACKED).sum() >= 150


@pytest.mark.parametrize("name", list(CASES))
def test_bit_parity_with_the_restatement(ctx, name):
    assert_same(gpu(ctx, CASES[name]), ref(name))


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_point_counts_around_the_wave_and_the_workgroup(ctx, n):
    """A track does not depend on the other points of its call."""
    assert_same(gpu(ctx, CASES["odd_r10_l3_n200"], n), ref("odd_r10_l3_n200"), n)


@pytest.mark.parametrize("name", ["odd_r10_l3_n200", "odd_r1", "odd_l8_clamped", "even_r10_l3", "kitti_r10_l4_fb"])
def test_pyramid_is_byte_equal(ctx, name):
    c = CASES[name]
    want = R.pyramid(c["img0"], c["kw"]["levels"], c["kw"]["win_radius"])
    got = klt.pyramid(c["img0"], c["kw"]["levels"], c["kw"]["win_radius"], ctx=ctx)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def test_results_never_depend_on_the_pyramid_cache(ctx):
    c, want = CASES["odd_fb"], ref("odd_fb")
    other = CASES["even_r10_l3"]
    assert_same(gpu(ctx, c, tags=(101, 102)), want)            # both pyramids built and kept
    assert_same(gpu(ctx, c, tags=(101, 102)), want)            # both hit
    kw = dict(c["kw"])
    # a hit needs no pixels: garbage in place of the images changes nothing
    junk = np.zeros_like(c["img0"])
    assert_same(klt.track(junk, junk, c["pts"], tags=(101, 102), ctx=ctx, **kw), want)
    # a second image size in between, tagged and untagged
    assert_same(gpu(ctx, other, tags=(201, 0)), ref("even_r10_l3"))
    assert_same(gpu(ctx, other), ref("even_r10_l3"))
    assert_same(gpu(ctx, c, tags=(101, 102)), want)
    # the cache cycled through 5 more tags: 101 and 102 are gone and rebuilt from the pixels
    for t in range(301, 306):
        assert_same(gpu(ctx, other, tags=(t, 0)), ref("even_r10_l3"))
    assert_same(gpu(ctx, c, tags=(101, 102)), want)
    # the same tag for other extents or levels is another entry, not a stale hit
    assert_same(gpu(ctx, other, tags=(101, 102)), ref("even_r10_l3"))
    assert_same(gpu(ctx, CASES["odd_l1"], tags=(101, 102)), ref("odd_l1"))
    assert_same(gpu(ctx, c), want)


def test_a_tagged_image_may_be_none_on_a_hit(ctx):
    c, want = CASES["odd_r7"], ref("odd_r7")
    assert_same(gpu(ctx, c, tags=(401, 402)), want)
    kw = dict(c["kw"])
    assert_same(klt.track(None, c["img1"], c["pts"], tags=(401, 0), ctx=ctx, **kw), want)
    from visualodometry_amd import _lib

    with pytest.raises(_lib.VoError, match="not in the pyramid cache"):
        klt.track(None, c["img1"], c["pts"], tags=(499, 0), ctx=ctx, **kw)
    assert_same(gpu(ctx, c), want)  # the context is as usable as before


def test_cv2_style_call(ctx):
    c, want = CASES["odd_r10_l3_n200"], ref("odd_r10_l3_n200")
    p1, st, err = klt.calcOpticalFlowPyrLK(c["img0"], c["img1"], c["pts"].reshape(-1, 1, 2), None, winSize=(21, 21),
                                           maxLevel=2, ctx=ctx)
    assert p1.shape == (200, 1, 2) and st.shape == (200, 1) and err.shape == (200, 1)
    assert st.dtype == np.uint8 and p1.dtype == np.float32 and err.dtype == np.float32
    np.testing.assert_array_equal(st[:, 0], (want[1] == R.TRACKED).astype(np.uint8))
    np.testing.assert_array_equal(S.bits(p1[:, 0]), S.bits(want[0]))


def test_image_too_small_for_a_window_and_no_points(ctx):
    tiny = np.full((22, 40), 7, np.uint8)
    _, status, _ = klt.track(tiny, tiny, [[11, 20], [5, 5]], win_radius=10, levels=3, ctx=ctx)
    assert status.tolist() == [R.START_OUTSIDE, R.START_OUTSIDE]
    p1, status, err = klt.track(tiny, tiny, np.zeros((0, 2)), ctx=ctx)
    assert p1.shape == (0, 2) and status.shape == (0,) and err.shape == (0,)
