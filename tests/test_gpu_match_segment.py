"""GPU parity of the segment-gated matcher (``matcher.match_segment`` / ``vo_match_segment``) against
the oracle composition in ``tests/segment_ref.py``: pairs compared by ``assert_array_equal``,
distances by their ``uint32`` bits.

Every scene case first asserts in the restatement alone that it shows something (the conditions of
``gated_ref.informative``): some queries have no candidate, some exactly one, some three or more;
``max_dist`` rejects some kept pairs and not all; the unique rule removes some pairs and not all.
"""

import functools

import numpy as np
import pytest

from oracle import match_ref
from tests import gated_ref as G
from tests import segment_ref as S
from visualodometry_amd import _lib, matcher
from visualodometry_amd._lib import C, ptr

pytestmark = pytest.mark.gpu

RATIO = 0.8
HINTS = ((1241, 376), None, (0, 0), (17, 5), (100000, 3), (376, 1241), (2 ** 31 - 1, 2 ** 31 - 1))


def max_dist_for(kind, dim):
    """Between a noisy copy (8 sqrt(dim) for the integer scenes' sigma 8, 0.02 sqrt(dim) for the unit
    rows) and an unrelated row (about 104 sqrt(dim), sqrt(2)): 300 at the SIFT shape, 0.9 for floats."""
    return 300.0 * np.sqrt(dim / 128.0) if kind == "sift" else 0.9


@functools.lru_cache(maxsize=None)
def _scene(kind, n0, n1, dim=None, radius=3.0):
    return S.scene(kind, n0, n1, 1, dim=dim, radius=radius)


@functools.lru_cache(maxsize=None)
def _scene_ref(kind, n0, n1, dim=None, radius=3.0):
    s = _scene(kind, n0, n1, dim, radius)
    return S.segmented(s.d0, s.seg, s.radius, s.d1, s.kp1, RATIO, max_dist_for(kind, s.d0.shape[1]), True)


def _same(got, ref: G.Gated):
    pairs, dist = got
    assert pairs.dtype == np.int64 and pairs.ndim == 2 and pairs.shape[1] == 2 and dist.dtype == np.float32
    np.testing.assert_array_equal(pairs, ref.pairs)
    np.testing.assert_array_equal(dist.view(np.uint32), ref.dist.view(np.uint32))


def _check(ctx, d0, seg, radius, d1, kp1, ratio=RATIO, max_dist=0.0, unique=True, image_size=None):
    ref = S.segmented(d0, seg, radius, d1, kp1, ratio, max_dist, unique)
    got = matcher.match_segment(d0, seg, radius, d1, kp1, ratio, max_dist, unique, image_size, True, ctx)
    _same(got, ref)
    if unique:
        assert len(set(got[0][:, 1].tolist())) == len(got[0])
    return ref


def _check_scene(ctx, kind, n0, n1, dim=None, radius=3.0):
    s, ref = _scene(kind, n0, n1, dim, radius), _scene_ref(kind, n0, n1, dim, radius)
    assert S.informative(ref), (np.bincount(np.minimum(ref.n_cand, 3)), ref.n_ratio, ref.n_near, ref.n_final)
    got = matcher.match_segment(s.d0, s.seg, s.radius, s.d1, s.kp1, RATIO, max_dist_for(kind, s.d0.shape[1]), True,
                                s.size, True, ctx)
    _same(got, ref)
    assert len(set(got[0][:, 1].tolist())) == len(got[0])  # one-to-one
    return s, ref, got


# ---- scenes ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sift", "float"])
@pytest.mark.parametrize("n0,n1", [(300, 400), (700, 900)])  # neither n1 is a multiple of 64
def test_scenes(ctx, kind, n0, n1):
    s, _, _ = _check_scene(ctx, kind, n0, n1)
    length = np.hypot(s.seg[:, 2] - s.seg[:, 0], s.seg[:, 3] - s.seg[:, 1])
    assert np.nanmax(np.where(np.isfinite(length), length, 0)) > 350  # capsules across many grid rows


@pytest.mark.parametrize("kind", ["sift", "float"])
@pytest.mark.parametrize("dim", [64, 100, 128, 256, 320])  # 100: no float4 rows; 320: past the int8 path's 256
def test_dims(ctx, kind, dim):
    _check_scene(ctx, kind, 300, 400, dim)


@pytest.mark.parametrize("kind", ["sift", "float"])
def test_radius_8_walks_several_cells_across(ctx, kind):
    _, ref, _ = _check_scene(ctx, kind, 300, 400, None, 8.0)
    assert ref.n_cand.max() >= 8 and np.median(ref.n_cand) >= 2


def test_without_unique_and_without_max_dist(ctx):
    s = _scene("sift", 300, 400)
    a = _check(ctx, s.d0, s.seg, s.radius, s.d1, s.kp1, unique=False, max_dist=300.0, image_size=s.size)
    b = _check(ctx, s.d0, s.seg, s.radius, s.d1, s.kp1, unique=True, max_dist=0.0, image_size=s.size)
    c = _check(ctx, s.d0, s.seg, s.radius, s.d1, s.kp1, unique=False, max_dist=0.0, image_size=s.size)
    assert len(a.pairs) > _scene_ref("sift", 300, 400).n_final and len(c.pairs) > len(b.pairs)


def test_inactive_queries_of_each_kind(ctx):
    s, ref = _scene("sift", 300, 400), _scene_ref("sift", 300, 400)
    assert s.radius[s.quiet[0]] == -1 and np.isnan(s.radius[s.quiet[1]]) and np.isnan(s.seg[s.quiet[2], 0]) and \
        np.isinf(s.seg[s.quiet[3], 3])
    clean_seg, clean_rad = matcher.epipolar_segments(s.kp0, s.T_cw0, s.T_cw1, s.K, s.size, S.Z_MIN, S.Z_MAX)[0], 3.0
    clean = _check(ctx, s.d0, clean_seg, clean_rad, s.d1, s.kp1, max_dist=300.0, unique=False, image_size=s.size)
    part = _check(ctx, s.d0, s.seg, s.radius, s.d1, s.kp1, max_dist=300.0, unique=False, image_size=s.size)
    assert (clean.n_cand[s.quiet] > 0).sum() >= 2 and (part.n_cand[s.quiet] == 0).all()
    assert not np.isin(s.quiet, part.pairs[:, 0]).any()
    assert (ref.n_cand[s.quiet] == 0).all() and (ref.n_cand[~s.valid] == 0).all()  # NaN rows of epipolar_segments
    for coord in range(4):
        for bad in (np.nan, np.inf, -np.inf):
            seg = clean_seg[:8].copy()
            seg[:, coord] = bad
            assert len(_check(ctx, s.d0[:8], seg, 1e9, s.d1, s.kp1).pairs) == 0


# ---- edge sizes --------------------------------------------------------------------------
def test_edge_sizes(ctx):
    s = _scene("sift", 300, 400)
    ref = _scene_ref("sift", 300, 400)
    i = int(ref.pairs[0, 0])
    one = _check(ctx, s.d0[i:i + 1], s.seg[i:i + 1], 3.0, s.d1, s.kp1, max_dist=300.0)  # n0 == 1
    assert one.pairs.tolist() == [[0, int(ref.pairs[0, 1])]]
    j = int(ref.pairs[0, 1])
    lone = _check(ctx, s.d0, s.seg, s.radius, s.d1[j:j + 1], s.kp1[j:j + 1], max_dist=300.0)  # n1 == 1
    assert len(lone.pairs) == 1 and lone.pairs[0, 1] == 0
    e_d, e_seg, e_xy = np.zeros((0, 128), np.float32), np.zeros((0, 4), np.float32), np.zeros((0, 2), np.float32)
    for a in ((e_d, e_seg, 3.0, s.d1, s.kp1), (s.d0, s.seg, s.radius, e_d, e_xy), (e_d, e_seg, 3.0, e_d, e_xy)):
        pairs, dist = matcher.match_segment(*a, return_dist=True, ctx=ctx)
        assert pairs.shape == (0, 2) and pairs.dtype == np.int64 and dist.shape == (0,)
        assert matcher.match_segment(*a, ctx=ctx).shape == (0, 2)


def test_64_and_65_candidates_along_one_segment(ctx):
    """More candidates than lanes, on both sides of a full wave's worth: the lane loop's further trips."""
    rng = np.random.default_rng(5)

    def along(a, b, n):
        t, off = rng.uniform(0, 1, n), rng.uniform(-2.0, 2.0, n)
        d = np.subtract(b, a) / np.hypot(*np.subtract(b, a))
        return np.add(a, t[:, None] * np.subtract(b, a)) + off[:, None] * np.array([-d[1], d[0]])

    seg = np.array([[100, 40, 500, 300], [600, 350, 1200, 20], [50, 300, 400, 310], [700, 20, 900, 20]], np.float32)
    kp = np.concatenate([along(seg[0, :2], seg[0, 2:], 64), along(seg[1, :2], seg[1, 2:], 65),
                         along(seg[2, :2], seg[2, 2:], 30),
                         np.stack([rng.uniform(0, 90, 200), rng.uniform(0, 30, 200)], axis=1)]).astype(np.float32)
    kp = kp[rng.permutation(len(kp))]
    d1 = rng.integers(0, 256, (len(kp), 128)).astype(np.float32)
    d0 = rng.integers(0, 256, (4, 128)).astype(np.float32)
    ref = _check(ctx, d0, seg, 2.5, d1, kp, ratio=2.0, image_size=(1241, 376))
    assert ref.n_cand.tolist() == [64, 65, 30, 0] and len(ref.pairs) == 3


# ---- ties to the circular gate and to the dense matcher ------------------------------------
@pytest.mark.parametrize("kind", ["sift", "float"])
def test_zero_length_segment_is_match_gated(ctx, kind):
    s = G.scene(kind, 300, 400, 1)
    md = max_dist_for(kind, s.d0.shape[1])
    seg = np.concatenate([s.pred, s.pred], axis=1)
    ref = G.gated(s.d0, s.pred, s.radius, s.d1, s.kp1, RATIO, md, True)
    assert G.informative(ref)
    for size in (s.size, None, (17, 5)):
        circle = matcher.match_gated(s.d0, s.pred, s.radius, s.d1, s.kp1, RATIO, md, True, size, True, ctx)
        capsule = matcher.match_segment(s.d0, seg, s.radius, s.d1, s.kp1, RATIO, md, True, size, True, ctx)
        _same(circle, ref)
        _same(capsule, ref)


@pytest.mark.parametrize("kind", ["sift", "float"])
def test_infinite_radius_is_the_dense_matcher(ctx, kind):
    """radius = +inf with any segment, max_dist = 0, no unique: every finite keypoint is a candidate of
    every query, so the result is knn-2 + ratio test over all rows -- the pinned path's and the oracle's."""
    s = _scene(kind, 300, 400)
    seg = np.nan_to_num(s.seg, nan=5.0, posinf=7.0)
    ref = _check(ctx, s.d0, seg, np.inf, s.d1, s.kp1, ratio=0.75, unique=False, image_size=s.size)
    dense = match_ref.match_int(s.d0, s.d1, 0.75) if kind == "sift" else match_ref.match_c(s.d0, s.d1, 0.75, nthreads=8)
    assert 0 < len(dense) < len(s.d0)
    np.testing.assert_array_equal(ref.pairs, dense)
    np.testing.assert_array_equal(matcher.match_knn2_ratio(s.d0, s.d1, 0.75, ctx=ctx), dense)
    np.testing.assert_array_equal(matcher.match_segment(s.d0, seg, np.inf, s.d1, s.kp1, 0.75, unique=False, ctx=ctx),
                                  dense)


# ---- directions, borders, hints --------------------------------------------------------------
def _lattice():
    """Keypoints on cell borders (multiples of 16), at negative coordinates and beyond the image."""
    rng = np.random.default_rng(11)
    xs = np.array([-40, -16, -0.0, 0, 15.999, 16, 16.001, 32, 48, 63.999, 64, 80, 96, 111.5, 112, 130, 1e6], np.float32)
    ys = np.array([-1e6, -20, 0, 16, 31.999, 32, 47, 48, 64, 70], np.float32)
    kp = np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2).astype(np.float32)
    kp = kp[rng.permutation(len(kp))]
    return kp, rng.integers(0, 256, (len(kp), 64)).astype(np.float32)


SEGMENTS = np.float32([
    [16, 16, 96, 16],          # horizontal, on a cell border
    [32, 0, 32, 64],           # vertical, on a cell border
    [0, 0, 64, 64],            # 45 degrees through cell corners
    [64, 64, 0, 0],            # the same reversed
    [96, 16, 16, 16],          # the horizontal one reversed
    [-500, 20, 2000, 50],      # longer than the image, starting and ending outside
    [-30, -30, 40, 40],        # starting outside the image
    [130, 100, 100, 40],       # starting outside, steep
    [8, 70, 120, -20],         # descending across every row
    [48, 32, 48, 32],          # zero length on a lattice point
    [10, 5, 10.5, 5.25],       # shorter than a pixel
    [1e6, 0, -1e6, 70],        # far beyond both sides
    [0, -1e6, 112, 1e6],       # far beyond top and bottom
    [40, 24, 41, 1e5],         # leaving through the last row
])


def test_directions_borders_radii_and_hints(ctx):
    kp, d1 = _lattice()
    d0 = np.random.default_rng(12).integers(0, 256, (len(SEGMENTS), 64)).astype(np.float32)
    for radius in (0.0, 3.0, 15.999, 16.0, 40.0, 1e7):
        ref = S.segmented(d0, SEGMENTS, radius, d1, kp, 2.0, 0.0, False)
        assert radius == 0.0 or (ref.n_cand > 0).sum() >= 10
        # a and b swapped: the same candidates, wherever the float32 differences are exact (every
        # segment but the three that reach 1e5 and beyond: there a keypoint within a rounding of the
        # boundary may fall on either side, and the device is held to the restatement both ways round)
        swapped = S.candidates(SEGMENTS[:, [2, 3, 0, 1]], radius, kp)
        for i, (x, y) in enumerate(zip(swapped, S.candidates(SEGMENTS, radius, kp))):
            if np.abs(SEGMENTS[i]).max() < 1e4:
                np.testing.assert_array_equal(x, y)
        back = S.segmented(d0, SEGMENTS[:, [2, 3, 0, 1]], radius, d1, kp, 2.0, 0.0, False)
        for size in HINTS + ((112, 64), (113, 65)):
            got = matcher.match_segment(d0, SEGMENTS, radius, d1, kp, 2.0, 0.0, False, size, True, ctx)
            _same(got, ref)
            got = matcher.match_segment(d0, SEGMENTS[:, [2, 3, 0, 1]], radius, d1, kp, 2.0, 0.0, False, size, True, ctx)
            _same(got, back)
    # keypoints at distance exactly r: from the interior (16 above the horizontal segment), from each end
    c16, c15 = S.candidates(SEGMENTS, 16.0, kp), S.candidates(SEGMENTS, np.float32(15.999), kp)

    def at(x, y):
        return int(np.flatnonzero((kp[:, 0] == x) & (kp[:, 1] == y))[0])

    for j in (at(48, 32), at(48, 0), at(0, 16), at(112, 16)):
        assert j in c16[0] and j not in c15[0]
    assert at(64, 16) in S.candidates(SEGMENTS, 0.0, kp)[0]  # on the segment
    assert S.segmented(d0, SEGMENTS, 0.0, d1, kp, 2.0, 0.0, False).n_cand[9] == 1


@pytest.mark.parametrize("kind", ["sift", "float"])
def test_image_size_never_changes_the_result(ctx, kind):
    s, ref = _scene(kind, 700, 900), _scene_ref(kind, 700, 900)
    md = max_dist_for(kind, s.d0.shape[1])
    for size in HINTS + ((-4, -4),):
        _same(matcher.match_segment(s.d0, s.seg, s.radius, s.d1, s.kp1, RATIO, md, True, size, True, ctx), ref)


def test_keypoints_outside_the_hinted_extent(ctx):
    """The scene's keypoints binned under hints far smaller than their extent, and shifted so that many
    lie at negative coordinates: the border rows and columns stand for unbounded bands."""
    s = _scene("sift", 700, 900)
    shift = np.float32([-600.0, -200.0])
    seg = s.seg + np.concatenate([shift, shift])
    kp = s.kp1 + shift
    ref = S.segmented(s.d0, seg, s.radius, s.d1, kp, RATIO, 300.0, True)
    assert S.informative(ref)
    for size in ((1241, 376), (17, 5), (100, 100), (640, 3), None):
        _same(matcher.match_segment(s.d0, seg, s.radius, s.d1, kp, RATIO, 300.0, True, size, True, ctx), ref)


# ---- radius array ------------------------------------------------------------------------------
def test_radius_array_against_the_scalar(ctx):
    s = _scene("float", 300, 400)
    seg = np.nan_to_num(s.seg, nan=5.0, posinf=7.0)
    a = matcher.match_segment(s.d0, seg, np.full(300, 3.0, np.float32), s.d1, s.kp1, RATIO, 0.9, True, s.size, True, ctx)
    b = matcher.match_segment(s.d0, seg, 3.0, s.d1, s.kp1, RATIO, 0.9, True, s.size, True, ctx)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    rad = np.random.default_rng(3).choice(np.float32([-1, 0, 1, 3, 8, 25, np.inf, np.nan]), 300)
    ref = _check(ctx, s.d0, seg, rad, s.d1, s.kp1, max_dist=0.9, image_size=s.size)
    assert 0 < len(ref.pairs) and not np.array_equal(ref.pairs, b[0])
    for scalar in (-1.0, float("nan")):  # an inactive scalar: nothing
        assert len(_check(ctx, s.d0, seg, scalar, s.d1, s.kp1).pairs) == 0


# ---- non-finite descriptors ----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sift", "float"])
def test_nan_train_row_and_inf_query_row(ctx, kind):
    s, clean = _scene(kind, 300, 400), _scene_ref(kind, 300, 400)
    j = int(clean.pairs[len(clean.pairs) // 2, 1])
    d1 = s.d1.copy()
    d1[j, 17] = np.nan
    md = max_dist_for(kind, s.d0.shape[1])
    ref = _check(ctx, s.d0, s.seg, s.radius, d1, s.kp1, max_dist=md, image_size=s.size)
    assert j in clean.pairs[:, 1] and j not in ref.pairs[:, 1]
    d0 = s.d0.copy()
    i = int(clean.pairs[3, 0])
    d0[i, 0] = np.inf  # every distance of this query is not < FLT_MAX
    ref = _check(ctx, d0, s.seg, s.radius, s.d1, s.kp1, max_dist=md, image_size=s.size)
    assert i not in ref.pairs[:, 0]
    kp = s.kp1.copy()
    kp[j, 1] = np.nan  # a keypoint with a non-finite coordinate is never a candidate
    ref = _check(ctx, s.d0, s.seg, s.radius, s.d1, kp, max_dist=md, image_size=s.size)
    assert j not in ref.pairs[:, 1]


# ---- the C entry: device pointers, profiler ids ------------------------------------------------
def _raw(ctx, s, flags, p_des1=None, p_kp1=None, n1=None):
    n0, dim = s.d0.shape
    n1 = len(s.d1) if n1 is None else n1
    opt = _lib.MatchSegmentOptionsC(seg=s.seg.ctypes.data, radius=s.radius.ctypes.data,
                                    kp1=s.kp1.ctypes.data if p_kp1 is None else p_kp1, radius0=0.0, width=s.size[0],
                                    height=s.size[1], ratio=RATIO, max_dist=300.0, flags=flags, reserved=0)
    out = np.empty((n0, 2), np.int32)
    dist = np.empty(n0, np.float32)
    cnt = np.zeros(1, np.int32)
    rc = ctx.lib.vo_match_segment(ctx.handle, C.c_void_p(s.d0.ctypes.data), n0,
                                  C.c_void_p(s.d1.ctypes.data if p_des1 is None else p_des1), n1, dim, C.byref(opt),
                                  ptr(out, C.c_int32), ptr(dist, C.c_float), ptr(cnt, C.c_int32))
    return rc, out[:cnt[0]].astype(np.int64), dist[:cnt[0]]


def test_device_pointer_route_equals_the_host_route(ctx):
    s, ref = _scene("sift", 300, 400), _scene_ref("sift", 300, 400)
    U, D = _lib.VO_MATCH_GATE_UNIQUE, _lib.VO_MATCH_DEVICE_PTRS
    rc, pairs, dist = _raw(ctx, s, U)
    assert rc == _lib.VO_OK
    _same((pairs, dist), ref)
    rc, _, _ = _raw(ctx, s, U | D)  # host memory under the flag: refused before any launch
    assert rc == _lib.VO_ERR_ARG
    b = _lib.DeviceArray.from_numpy(ctx, s.d1)
    k = _lib.DeviceArray.from_numpy(ctx, s.kp1)
    for _ in range(2):
        rc, pairs, dist = _raw(ctx, s, U | D, b.ptr, k.ptr)
        assert rc == _lib.VO_OK
        _same((pairs, dist), ref)
    rc, _, _ = _raw(ctx, s, U | D, b.ptr, k.ptr, n1=400 + 4096)  # rows far past the allocations
    assert rc == _lib.VO_ERR_ARG
    rc, _, _ = _raw(ctx, s, U | D, b.ptr, s.kp1.ctypes.data)  # one host array among device pointers
    assert rc == _lib.VO_ERR_ARG
    rc, _, _ = _raw(ctx, s, U | D, s.d1.ctypes.data, k.ptr)
    assert rc == _lib.VO_ERR_ARG
    # rows that are not 16-byte aligned (a view into a larger tensor): the scalar-load kernel
    shifted = _lib.DeviceArray.from_numpy(ctx, np.concatenate([np.zeros(1, np.float32), s.d1.reshape(-1)]))
    rc, pairs, dist = _raw(ctx, s, U | D, shifted.ptr + 4, k.ptr)
    assert rc == _lib.VO_OK
    _same((pairs, dist), ref)


def test_launches_count_under_the_existing_profiler_ids(ctx):
    s, ref = _scene("sift", 300, 400), _scene_ref("sift", 300, 400)
    _lib.profile_enable(ctx, True)
    try:
        _same(matcher.match_segment(s.d0, s.seg, s.radius, s.d1, s.kp1, RATIO, 300.0, True, s.size, True, ctx), ref)
        prof = _lib.profile_read(ctx)
    finally:
        _lib.profile_enable(ctx, False)
    assert set(prof) == {"match_pack", "match_f32"}
    assert prof["match_pack"][1] == 1 and prof["match_f32"][1] == 1


def test_match_gated_is_unchanged_by_a_segment_call_in_between(ctx):
    """The two share the gate workspace: the circular matcher on its own scene stays bit-identical to
    ``gated_ref`` before and after a segment call of another shape, and so does the segment matcher."""
    g = G.scene("sift", 300, 400, 1)
    gref = G.gated(g.d0, g.pred, g.radius, g.d1, g.kp1, RATIO, 300.0, True)
    assert G.informative(gref)
    s, sref = _scene("sift", 700, 900), _scene_ref("sift", 700, 900)
    for _ in range(2):
        _same(matcher.match_gated(g.d0, g.pred, g.radius, g.d1, g.kp1, RATIO, 300.0, True, g.size, True, ctx), gref)
        _same(matcher.match_segment(s.d0, s.seg, s.radius, s.d1, s.kp1, RATIO, 300.0, True, s.size, True, ctx), sref)
    _same(matcher.match_gated(g.d0, g.pred, g.radius, g.d1, g.kp1, RATIO, 300.0, True, g.size, True, ctx), gref)
