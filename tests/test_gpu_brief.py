"""vo_brief_describe on the MI355X against the restatement (tests/brief_ref.py), bit for bit:
descriptors, bins and status.  Images from one pixel to a few workgroups' worth of points; points on
the border (the reflection), at halves (rounding to even), just off the image and not finite; point
counts below, at and above the four waves of a workgroup; the pyramid cache never changes a bit; a
quarter turn of the image keeps the descriptor."""

import numpy as np
import pytest

from tests import brief_ref as R
from visualodometry_amd import brief, klt

pytestmark = pytest.mark.gpu

H, W = 96, 128
_REF = {}


def images():
    return {
        "one_pixel": np.array([[200]], np.uint8),
        "tiny_5x7": R.texture(5, 7, seed=1, smooth=0),
        "odd_40x33": R.texture(40, 33, seed=2, smooth=1),
        "flat": R.flat(40, 33),
        "step_edge": R.step_edge(40, 33),
        "texture": R.texture(H, W, seed=3),
    }


IMAGES = images()


def points(name, n=None):
    """The edge points of the image, then uniform random positions on and just off it, n in all."""
    h, w = IMAGES[name].shape
    p = R.edge_points(h, w)
    if n is not None:
        if n > len(p):
            rng = np.random.default_rng(n)
            extra = np.stack([rng.uniform(-1.0, w, n - len(p)), rng.uniform(-1.0, h, n - len(p))], 1).astype(np.float32)
            p = np.concatenate([p, extra])
        p = p[:n]
    return np.ascontiguousarray(p, np.float32)


def ref(name, n=None):
    key = (name, n)
    if key not in _REF:
        _REF[key] = R.describe(IMAGES[name], points(name, n))
    return _REF[key]


def assert_same(got, want):
    assert got[0].dtype == np.uint32 and got[0].shape == want[0].shape
    assert got[1].dtype == np.int32 and got[2].dtype == np.uint8
    np.testing.assert_array_equal(got[2], want[2])
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[0], want[0])


@pytest.mark.parametrize("name", list(IMAGES))
def test_bit_parity_on_every_image(ctx, name):
    got = brief.describe(IMAGES[name], points(name), ctx=ctx)
    want = ref(name)
    assert_same(got, want)
    assert (want[2] == 1).sum() >= 10 and (want[2] == 0).sum() >= 3  # both kinds of point are present


def test_flat_image_gives_bin_zero_and_no_bits_and_a_step_edge_gives_some(ctx):
    des, bins, status = brief.describe(IMAGES["flat"], points("flat"), ctx=ctx)
    assert not des.any() and not bins.any() and (status == 0).sum() >= 16
    pts = np.concatenate([points("step_edge"), R.interior_points(40, 33, 24, margin=2)])
    got = brief.describe(IMAGES["step_edge"], pts, ctx=ctx)
    want = R.describe(IMAGES["step_edge"], pts)
    assert_same(got, want)
    ok = want[2] == 0
    bits = np.unpackbits(want[0][ok].view(np.uint8), axis=1)
    assert 0 < bits.mean() < 0.5  # many box sums are equal: the strict < decides


@pytest.mark.parametrize("n", [1, 3, 4, 5, 64, 257])
def test_partial_workgroups(ctx, n):
    got = brief.describe(IMAGES["texture"], points("texture", n), ctx=ctx)
    assert_same(got, ref("texture", n))
    assert len(got[0]) == n


def test_repeated_calls_and_optional_outputs(ctx):
    pts = points("texture", 64)
    first = brief.describe(IMAGES["texture"], pts, ctx=ctx)
    for _ in range(2):
        again = brief.describe(IMAGES["texture"], pts, ctx=ctx)
        for a, b in zip(first, again):
            np.testing.assert_array_equal(a, b)
    # a smaller call after a larger one reuses the workspace
    assert_same(brief.describe(IMAGES["odd_40x33"], points("odd_40x33"), ctx=ctx), ref("odd_40x33"))
    des = np.zeros((64, 8), np.uint32)
    rc = ctx.lib.vo_brief_describe(ctx.handle, IMAGES["texture"].ctypes.data, 0, H, W, pts.ctypes.data, 64, 0,
                                   des.ctypes.data, None, None)
    assert rc == 0
    np.testing.assert_array_equal(des, first[0])


def test_tag_hit_tag_miss_and_image_passed_agree(ctx):
    img0 = IMAGES["texture"]
    img1 = np.ascontiguousarray(np.roll(img0, (2, -3), (0, 1)))
    seeds = R.interior_points(H, W, 20, seed=9, margin=30)
    t0, t1 = 0x7B21EF00, 0x7B21EF01
    first = klt.track(img0, img1, seeds, win_radius=7, levels=3, tags=(t0, t1), ctx=ctx)
    pts = points("texture", 64)
    want = R.describe(img1, pts)
    miss = brief.describe(img1, pts, tag=0x7B21EF09, ctx=ctx)  # never cached
    hit = brief.describe(None, pts, tag=t1, shape=img1.shape, ctx=ctx)
    hit_with_image = brief.describe(img1, pts, tag=t1, ctx=ctx)
    plain = brief.describe(img1, pts, ctx=ctx)
    for got in (miss, hit, hit_with_image, plain):
        assert_same(got, want)
    assert_same(brief.describe(None, points("texture", 64), tag=t0, shape=img0.shape, ctx=ctx), ref("texture", 64))
    with pytest.raises(Exception, match="not in the pyramid cache"):
        brief.describe(None, pts, tag=0x7B21EF09, shape=img1.shape, ctx=ctx)  # the miss created no entry
    with pytest.raises(Exception, match="not in the pyramid cache"):
        brief.describe(None, pts, tag=t1, shape=(H, W + 1), ctx=ctx)  # another shape is another image
    again = klt.track(img0, None, seeds, win_radius=7, levels=3, tags=(t0, t1), ctx=ctx)  # the cache was only read
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b)


def test_quarter_turn_identity_on_the_device(ctx):
    img = IMAGES["texture"]
    pts = R.interior_points(H, W, 60, seed=4)
    des, bins, status = brief.describe(img, pts, ctx=ctx)
    rot = np.ascontiguousarray(np.rot90(img))
    rpts = np.stack([pts[:, 1], W - 1 - pts[:, 0]], 1)
    rdes, rbins, rstatus = brief.describe(rot, rpts, ctx=ctx)
    assert not status.any() and not rstatus.any() and len(set(bins.tolist())) > 8
    np.testing.assert_array_equal(rdes, des)
    np.testing.assert_array_equal(rbins, (bins + 24) % 32)
