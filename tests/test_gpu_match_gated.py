"""GPU parity of the projection-gated matcher (``matcher.match_gated`` / ``vo_match_gated``) against
the oracle composition in ``tests/gated_ref.py``: pairs and distances compared bit for bit.

Every scene case first asserts in the restatement alone that it shows something: some queries have
no candidate, some exactly one, some three or more; ``max_dist`` rejects some kept pairs and not
all; the unique rule removes some pairs and not all.
"""

import functools

import numpy as np
import pytest

from oracle import match_ref
from tests import gated_ref as G
from visualodometry_amd import _lib, matcher
from visualodometry_amd._lib import C, ptr

pytestmark = pytest.mark.gpu

RATIO = 0.8


def max_dist_for(kind, dim):
    """Between a noisy copy (8 sqrt(dim) for the integer scenes' sigma 8, 0.02 sqrt(dim) for the unit
    rows) and an unrelated row (about 104 sqrt(dim), sqrt(2)): 300 at the SIFT shape, 0.9 for floats."""
    return 300.0 * np.sqrt(dim / 128.0) if kind == "sift" else 0.9


@functools.lru_cache(maxsize=None)
def _scene(kind, n0, n1, dim=None, radius=12.0):
    return G.scene(kind, n0, n1, 1, dim=dim, radius=radius)


@functools.lru_cache(maxsize=None)
def _scene_ref(kind, n0, n1, dim=None, radius=12.0):
    s = _scene(kind, n0, n1, dim, radius)
    return G.gated(s.d0, s.pred, s.radius, s.d1, s.kp1, RATIO, max_dist_for(kind, s.d0.shape[1]), True)


def _same(got, ref: G.Gated):
    pairs, dist = got
    assert pairs.dtype == np.int64 and pairs.ndim == 2 and pairs.shape[1] == 2 and dist.dtype == np.float32
    np.testing.assert_array_equal(pairs, ref.pairs)
    np.testing.assert_array_equal(dist.view(np.uint32), ref.dist.view(np.uint32))


def _check(ctx, d0, pred, radius, d1, kp1, ratio=RATIO, max_dist=0.0, unique=True, image_size=None):
    ref = G.gated(d0, pred, radius, d1, kp1, ratio, max_dist, unique)
    got = matcher.match_gated(d0, pred, radius, d1, kp1, ratio, max_dist, unique, image_size, True, ctx)
    _same(got, ref)
    if unique:
        assert len(set(got[0][:, 1].tolist())) == len(got[0])
    return ref


def _check_scene(ctx, kind, n0, n1, dim=None, radius=12.0):
    s, ref = _scene(kind, n0, n1, dim, radius), _scene_ref(kind, n0, n1, dim, radius)
    assert G.informative(ref), (np.bincount(np.minimum(ref.n_cand, 3)), ref.n_ratio, ref.n_near, ref.n_final)
    got = matcher.match_gated(s.d0, s.pred, s.radius, s.d1, s.kp1, RATIO, max_dist_for(kind, s.d0.shape[1]), True,
                              s.size, True, ctx)
    _same(got, ref)
    assert len(set(got[0][:, 1].tolist())) == len(got[0])  # one-to-one
    return s, ref, got


# ---- scenes ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sift", "float"])
@pytest.mark.parametrize("n0,n1", [(300, 400), (700, 900)])  # neither n1 is a multiple of 64
def test_scenes(ctx, kind, n0, n1):
    _check_scene(ctx, kind, n0, n1)


@pytest.mark.parametrize("kind", ["sift", "float"])
@pytest.mark.parametrize("dim", [64, 100, 128, 256, 320])  # 100: no float4 rows; 320: past the int8 path's 256
def test_dims(ctx, kind, dim):
    _check_scene(ctx, kind, 300, 400, dim)


@pytest.mark.parametrize("kind", ["sift", "float"])
def test_radius_40_walks_several_cells(ctx, kind):
    _, ref, _ = _check_scene(ctx, kind, 300, 400, None, 40.0)
    assert ref.n_cand.max() >= 8 and np.median(ref.n_cand) >= 3


def test_without_unique_and_without_max_dist(ctx):
    s = _scene("sift", 300, 400)
    a = _check(ctx, s.d0, s.pred, s.radius, s.d1, s.kp1, unique=False, max_dist=300.0, image_size=s.size)
    b = _check(ctx, s.d0, s.pred, s.radius, s.d1, s.kp1, unique=True, max_dist=0.0, image_size=s.size)
    c = _check(ctx, s.d0, s.pred, s.radius, s.d1, s.kp1, unique=False, max_dist=0.0, image_size=s.size)
    assert len(a.pairs) > _scene_ref("sift", 300, 400).n_final and len(c.pairs) > len(b.pairs)


# ---- edge sizes --------------------------------------------------------------------------
def test_edge_sizes(ctx):
    s = _scene("sift", 300, 400)
    ref = _scene_ref("sift", 300, 400)
    i = int(ref.pairs[0, 0])
    one = _check(ctx, s.d0[i:i + 1], s.pred[i:i + 1], 12.0, s.d1, s.kp1, max_dist=300.0)  # n0 == 1
    assert one.pairs.tolist() == [[0, int(ref.pairs[0, 1])]]
    j = int(ref.pairs[0, 1])
    lone = _check(ctx, s.d0, s.pred, s.radius, s.d1[j:j + 1], s.kp1[j:j + 1], max_dist=300.0)  # n1 == 1
    assert len(lone.pairs) == 1 and lone.pairs[0, 1] == 0
    e_d, e_xy = np.zeros((0, 128), np.float32), np.zeros((0, 2), np.float32)
    for a in ((e_d, e_xy, 12.0, s.d1, s.kp1), (s.d0, s.pred, s.radius, e_d, e_xy), (e_d, e_xy, 12.0, e_d, e_xy)):
        pairs, dist = matcher.match_gated(*a, return_dist=True, ctx=ctx)
        assert pairs.shape == (0, 2) and pairs.dtype == np.int64 and dist.shape == (0,)
        assert matcher.match_gated(*a, ctx=ctx).shape == (0, 2)


def test_64_and_65_candidates(ctx):
    """More candidates than lanes, on both sides of a full wave's worth: the lane loop's further trips."""
    rng = np.random.default_rng(5)

    def cluster(cx, cy, n):
        ang, rad = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 4.0, n)
        return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1)

    kp = np.concatenate([cluster(100, 100, 64), cluster(300, 200, 65), cluster(700, 50, 30),
                         np.stack([rng.uniform(0, 1241, 200), rng.uniform(330, 376, 200)], axis=1)]).astype(np.float32)
    order = rng.permutation(len(kp))
    kp = kp[order]
    d1 = rng.integers(0, 256, (len(kp), 128)).astype(np.float32)
    pred = np.array([[100, 100], [300, 200], [700, 50], [600, 200]], np.float32)
    d0 = rng.integers(0, 256, (4, 128)).astype(np.float32)
    ref = _check(ctx, d0, pred, 5.0, d1, kp, ratio=2.0, image_size=(1241, 376))
    assert ref.n_cand.tolist() == [64, 65, 30, 0] and len(ref.pairs) == 3


# ---- tie to the dense matcher ----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sift", "float"])
def test_infinite_radius_is_the_dense_matcher(ctx, kind):
    """radius = +inf, max_dist = 0, no unique: every finite keypoint is a candidate of every query, so
    the result is knn-2 + ratio test over all rows -- the pinned path's and the oracle's."""
    s = _scene(kind, 300, 400)
    pred = np.nan_to_num(s.pred, nan=5.0, posinf=7.0)
    ref = _check(ctx, s.d0, pred, np.inf, s.d1, s.kp1, ratio=0.75, unique=False, image_size=s.size)
    dense = match_ref.match_int(s.d0, s.d1, 0.75) if kind == "sift" else match_ref.match_c(s.d0, s.d1, 0.75, nthreads=8)
    assert 0 < len(dense) < len(s.d0)
    np.testing.assert_array_equal(ref.pairs, dense)
    np.testing.assert_array_equal(matcher.match_knn2_ratio(s.d0, s.d1, 0.75, ctx=ctx), dense)
    np.testing.assert_array_equal(matcher.match_gated(s.d0, pred, np.inf, s.d1, s.kp1, 0.75, unique=False, ctx=ctx),
                                  dense)


# ---- the grid's borders -------------------------------------------------------------------------
def test_cell_borders_negative_and_outside_coordinates(ctx):
    """Keypoints on cell borders (multiples of 16), at negative coordinates and beyond the image;
    predictions on the lattice and outside the image whose circle reaches in; radius 16 puts
    lattice neighbours at distance exactly r."""
    rng = np.random.default_rng(11)
    xs = np.array([-40, -16, -0.0, 0, 15.999, 16, 16.001, 32, 48, 63.999, 64, 80, 96, 111.5, 112, 130, 1e6], np.float32)
    ys = np.array([-1e6, -20, 0, 16, 31.999, 32, 47, 48, 64, 70], np.float32)
    kp = np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2).astype(np.float32)
    kp = kp[rng.permutation(len(kp))]
    d1 = rng.integers(0, 256, (len(kp), 64)).astype(np.float32)
    pred = np.array([[16, 16], [0, 0], [-10, -10], [32, 32], [112, 48], [120, 60], [-30, 8], [64, -12], [128, 80],
                     [48, 32], [1e6, 3], [5, -1e6], [63.9995, 31.9995]], np.float32)
    d0 = rng.integers(0, 256, (len(pred), 64)).astype(np.float32)
    for size in ((112, 64), (113, 65), None):
        for radius in (16.0, 0.0, 15.999, 40.0, 1e7):
            ref = _check(ctx, d0, pred, radius, d1, kp, ratio=2.0, unique=False, image_size=size)
            assert radius == 0.0 or (ref.n_cand > 0).sum() >= 9
    east = int(np.flatnonzero((kp[:, 0] == 32) & (kp[:, 1] == 16))[0])  # at exactly r from prediction 0
    assert east in G.candidates(pred, 16.0, kp)[0] and east not in G.candidates(pred, np.float32(15.999), kp)[0]
    assert G.gated(d0, pred, 0.0, d1, kp, 2.0, 0.0, False).n_cand[:2].tolist() == [1, 2]  # (0, 0) and (-0.0, 0)


# ---- radius array, image size ----------------------------------------------------------------
def test_radius_array_against_the_scalar(ctx):
    s = _scene("float", 300, 400)
    pred = np.nan_to_num(s.pred, nan=5.0, posinf=7.0)
    a = matcher.match_gated(s.d0, pred, np.full(300, 12.0, np.float32), s.d1, s.kp1, RATIO, 0.9, True, s.size, True, ctx)
    b = matcher.match_gated(s.d0, pred, 12.0, s.d1, s.kp1, RATIO, 0.9, True, s.size, True, ctx)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    rad = np.random.default_rng(3).choice(np.float32([-1, 0, 3, 12, 25, 60, np.inf, np.nan]), 300)
    ref = _check(ctx, s.d0, pred, rad, s.d1, s.kp1, max_dist=0.9, image_size=s.size)
    assert 0 < len(ref.pairs) and not np.array_equal(ref.pairs, b[0])
    for scalar in (-1.0, float("nan")):  # an inactive scalar: nothing
        assert len(_check(ctx, s.d0, pred, scalar, s.d1, s.kp1).pairs) == 0


@pytest.mark.parametrize("kind", ["sift", "float"])
def test_image_size_never_changes_the_result(ctx, kind):
    s, ref = _scene(kind, 700, 900), _scene_ref(kind, 700, 900)
    md = max_dist_for(kind, s.d0.shape[1])
    for size in (s.size, None, (0, 0), (17, 5), (100000, 3), (-4, -4), (2 ** 31 - 1, 2 ** 31 - 1), (376, 1241)):
        _same(matcher.match_gated(s.d0, s.pred, s.radius, s.d1, s.kp1, RATIO, md, True, size, True, ctx), ref)


def test_hint_and_repeated_calls_never_change_the_result(ctx):
    s, ref = _scene("sift", 300, 400), _scene_ref("sift", 300, 400)
    prior = getattr(ctx, "desc_kind", matcher.DESC_AUTO)
    try:
        for kind in (matcher.DESC_FLOAT, matcher.DESC_SIFT, matcher.DESC_AUTO):
            matcher.set_descriptor_kind(kind, ctx)
            for _ in range(2):
                _same(matcher.match_gated(s.d0, s.pred, s.radius, s.d1, s.kp1, RATIO, 300.0, True, s.size, True, ctx),
                      ref)
            matcher.match_knn2_ratio(s.d0, s.d1, ctx=ctx)  # the dense matcher's workspace in between
    finally:
        matcher.set_descriptor_kind(prior, ctx)


# ---- non-finite descriptors ----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sift", "float"])
def test_nan_train_row_is_never_selected(ctx, kind):
    s, clean = _scene(kind, 300, 400), _scene_ref(kind, 300, 400)
    j = int(clean.pairs[len(clean.pairs) // 2, 1])
    d1 = s.d1.copy()
    d1[j, 17] = np.nan
    md = max_dist_for(kind, s.d0.shape[1])
    ref = _check(ctx, s.d0, s.pred, s.radius, d1, s.kp1, max_dist=md, image_size=s.size)
    assert j in clean.pairs[:, 1] and j not in ref.pairs[:, 1]
    d0 = s.d0.copy()
    i = int(clean.pairs[3, 0])
    d0[i, 0] = np.inf  # every distance of this query is not < FLT_MAX
    ref = _check(ctx, d0, s.pred, s.radius, s.d1, s.kp1, max_dist=md, image_size=s.size)
    assert i not in ref.pairs[:, 0]


# ---- the C entry: device pointers, profiler ids ------------------------------------------------
def _raw(ctx, s, flags, p_des1=None, p_kp1=None, n1=None):
    n0, dim = s.d0.shape
    n1 = len(s.d1) if n1 is None else n1
    opt = _lib.MatchGateOptionsC(pred=s.pred.ctypes.data, radius=s.radius.ctypes.data,
                                 kp1=s.kp1.ctypes.data if p_kp1 is None else p_kp1, radius0=0.0, width=s.size[0],
                                 height=s.size[1], ratio=RATIO, max_dist=300.0, flags=flags, reserved=0)
    out = np.empty((n0, 2), np.int32)
    dist = np.empty(n0, np.float32)
    cnt = np.zeros(1, np.int32)
    rc = ctx.lib.vo_match_gated(ctx.handle, C.c_void_p(s.d0.ctypes.data), n0,
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
    # rows that are not 16-byte aligned (a view into a larger tensor): the scalar-load kernel
    shifted = _lib.DeviceArray.from_numpy(ctx, np.concatenate([np.zeros(1, np.float32), s.d1.reshape(-1)]))
    rc, pairs, dist = _raw(ctx, s, U | D, shifted.ptr + 4, k.ptr)
    assert rc == _lib.VO_OK
    _same((pairs, dist), ref)


def test_launches_count_under_the_existing_profiler_ids(ctx):
    s, ref = _scene("sift", 300, 400), _scene_ref("sift", 300, 400)
    _lib.profile_enable(ctx, True)
    try:
        _same(matcher.match_gated(s.d0, s.pred, s.radius, s.d1, s.kp1, RATIO, 300.0, True, s.size, True, ctx), ref)
        prof = _lib.profile_read(ctx)
    finally:
        _lib.profile_enable(ctx, False)
    assert set(prof) == {"match_pack", "match_f32"}
    assert prof["match_pack"][1] == 1 and prof["match_f32"][1] == 1
