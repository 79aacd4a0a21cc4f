"""GPU parity of the mutual-check matcher (``cross_check=True`` / ``vo_match_mutual*``) against
the oracle composition in ``tests/mutual_ref.py`` -- bit-exact array equality.

Every case first asserts that the cross check removes some of the forward pairs and not all
of them in the reference (``0 < kept < forward``): a case where it removes nothing, or
everything, shows nothing.
"""

import numpy as np
import pytest

from oracle import match_ref
from tests import mutual_ref
from visualodometry_amd import _lib, matcher
from visualodometry_amd._lib import C, ptr
from visualodometry_amd.synthetic import sift_like_pair, superpoint_like_pair

pytestmark = pytest.mark.gpu


def _check(d0, d1, ctx, ratio, oracle="int", exempt=False, **kw):
    ref, n_forward = mutual_ref.mutual(d0, d1, ratio, oracle)
    if not exempt:
        assert mutual_ref.informative(ref, n_forward), (len(ref), n_forward)
    got = matcher.match_knn2_ratio(d0, d1, ratio=ratio, ctx=ctx, cross_check=True, **kw)
    assert got.dtype == np.int64 and got.ndim == 2 and got.shape[1] == 2
    np.testing.assert_array_equal(got, ref)
    assert len(set(got[:, 1].tolist())) == len(got)  # one-to-one
    return got


# ---- int8 path -----------------------------------------------------------------
@pytest.mark.parametrize("n0,n1", [(37, 5), (300, 17), (700, 800), (1000, 1200), (5, 37)])
def test_sift_like_ratio_one(ctx, n0, n1):
    _check(*sift_like_pair(n0, n1, 3), ctx, 1.0)


def test_single_query_row_is_legal(ctx):
    """n0 == 1: the reverse nearest of every train row is row 0 (exempt from the condition)."""
    d0, d1 = sift_like_pair(1, 64, 3)
    got = _check(d0, d1, ctx, 1.0, exempt=True)
    np.testing.assert_array_equal(got, match_ref.match_int(d0, d1, 1.0))


@pytest.mark.parametrize("dim", [64, 100, 192, 256])
def test_int_dims(ctx, dim):
    _check(*sift_like_pair(333, 444, 3, dim=dim), ctx, 1.0)
    _check(*mutual_ref.sift_near_duplicates(333, 444, 3, 150, dim), ctx, 0.75)


def test_sift_near_duplicate_keyframe_rows(ctx):
    _check(*mutual_ref.sift_near_duplicates(), ctx, 0.75)


# ---- float path ----------------------------------------------------------------
@pytest.mark.parametrize("n0,n1", [(37, 5), (333, 517), (700, 900)])
def test_superpoint_like_ratio_one(ctx, n0, n1):
    _check(*superpoint_like_pair(n0, n1, 3), ctx, 1.0, oracle="c")


@pytest.mark.parametrize("dim", [32, 100, 256])
def test_float_dims(ctx, dim):
    _check(*superpoint_like_pair(333, 517, 3, dim=dim), ctx, 1.0, oracle="c")


def test_superpoint_near_duplicate_keyframe_rows(ctx):
    _check(*mutual_ref.superpoint_near_duplicates(), ctx, 0.75, oracle="c")


def test_dim_over_256_takes_the_fp32_sweep(ctx):
    _check(*sift_like_pair(200, 300, 3, dim=320), ctx, 1.0, oracle="c")


@pytest.mark.parametrize("side", [0, 1])
def test_one_non_integer_value_switches_both_passes(ctx, side):
    d = [x.copy() for x in sift_like_pair(300, 400, 3)]
    d[side][7, 3] += 0.5
    _check(d[0], d[1], ctx, 1.0, oracle="c")


# ---- reverse ties ----------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", [("int", 128), ("float", 256)])
def test_equal_reverse_distances_keep_the_lower_query_index(ctx, kind, dim):
    """200 distinct rows, each 4 times at shuffled positions among 800 query rows: a train
    row's 4 equal reverse distances (inside a 16-lane group, across tiles, across splits)."""
    d0, d1 = mutual_ref.repeated_queries(kind, dim=dim)
    got = _check(d0, d1, ctx, 0.75, oracle="int" if kind == "int" else "c")
    assert len(got) == 200


def test_sqrt_collision_on_the_reverse_pass(ctx):
    """test_sqrt_collision_rescan's construction with the roles swapped: query rows 1 and 3 are
    at d2 = n + 1 and n (>= 2^22) from train row 0 and sqrtf maps both to one float, so the
    reverse key (dist, i') keeps query 1 although its d2 is larger."""
    n = None
    for cand in range(4_200_000, 8_000_000, 7):
        if np.sqrt(np.float32(cand)) == np.sqrt(np.float32(cand + 1)):
            n = cand
            break
    assert n is not None

    def vec_with_d2(target):  # values 0..255 on the leading coordinates, sum of squares == target
        v = np.zeros(128, np.float32)
        rem, k = target, 0
        while rem > 0:
            x = int(min(255, np.floor(np.sqrt(rem))))
            v[k] = x
            rem -= x * x
            k += 1
        assert rem == 0 and k <= 72
        return v

    far = vec_with_d2(n + 4000)
    d0 = np.stack([far, vec_with_d2(n + 1), far, vec_with_d2(n), far])
    d1 = np.zeros((2, 128), np.float32)
    d1[1, 72:] = 255.0  # the second neighbour every query needs: off the queries' support, far away
    ref, n_forward = mutual_ref.mutual(d0, d1, 0.9)
    assert n_forward == 5
    np.testing.assert_array_equal(ref, [[1, 0]])
    _check(d0, d1, ctx, 0.9)


# ---- hints, non-finite values ------------------------------------------------------
@pytest.mark.parametrize("oracle", ["int", "c"])
def test_hints_do_not_change_the_result(ctx, oracle):
    d0, d1 = mutual_ref.sift_near_duplicates() if oracle == "int" else mutual_ref.superpoint_near_duplicates()
    outs = [_check(d0, d1, ctx, 0.75, oracle=oracle, kind=k)
            for k in (matcher.DESC_AUTO, matcher.DESC_SIFT, matcher.DESC_FLOAT)]
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(outs[0], outs[2])


def test_non_finite_values(ctx):
    """A NaN in a query row and an inf in a train row: the exact sweep (no hint) and the re-rank
    kernel's exact scan (float hint) answer both passes."""
    f0, f1 = [x.copy() for x in superpoint_like_pair(333, 517, 3)]
    f0[5, 7] = np.nan
    f1[9, 3] = np.inf
    a = _check(f0, f1, ctx, 1.0, oracle="c")
    b = _check(f0, f1, ctx, 1.0, oracle="c", kind=matcher.DESC_FLOAT)
    np.testing.assert_array_equal(a, b)


# ---- edge sizes ------------------------------------------------------------------------
def test_edge_sizes(ctx):
    d = sift_like_pair(10, 10, 1)[0]
    e = np.zeros((0, 128), np.float32)
    for a, b in ((e, d), (d, e), (d, d[:1]), (e, e)):
        got = matcher.match_knn2_ratio(a, b, ctx=ctx, cross_check=True)
        assert got.shape == (0, 2) and got.dtype == np.int64


def test_cross_check_off_is_todays_result(ctx):
    d0, d1 = mutual_ref.sift_near_duplicates()
    np.testing.assert_array_equal(matcher.match_knn2_ratio(d0, d1, ctx=ctx, cross_check=False),
                                  match_ref.match_int(d0, d1))
    np.testing.assert_array_equal(matcher.match_knn2_ratio(d0, d1, ctx=ctx), match_ref.match_int(d0, d1))
    f0, f1 = mutual_ref.superpoint_near_duplicates()
    np.testing.assert_array_equal(matcher.match_knn2_ratio(f0, f1, ctx=ctx, cross_check=False),
                                  match_ref.match_c(f0, f1, nthreads=8))


# ---- batch ---------------------------------------------------------------------------
def test_batch_matches_single(ctx):
    B, n0, n1 = 3, 500, 600
    pairs = [sift_like_pair(n0, n1, 100 + b) for b in range(B)]
    a = _lib.DeviceArray.from_numpy(ctx, np.stack([p[0] for p in pairs]))
    b = _lib.DeviceArray.from_numpy(ctx, np.stack([p[1] for p in pairs]))
    best = matcher.match_batch_device(a, b, ratio=1.0, ctx=ctx, cross_check=True)
    matcher.synchronize(ctx)
    best = best.numpy()
    plain = matcher.match_batch_device(a, b, ratio=1.0, ctx=ctx)
    matcher.synchronize(ctx)
    plain = plain.numpy()
    for k in range(B):
        single = _check(*pairs[k], ctx, 1.0)
        got = np.nonzero(best[k] >= 0)[0]
        np.testing.assert_array_equal(np.stack([got, best[k][got]], 1), single)
        fwd = np.nonzero(plain[k] >= 0)[0]
        np.testing.assert_array_equal(np.stack([fwd, plain[k][fwd]], 1), match_ref.match_int(*pairs[k], 1.0))


def test_float_batch_matches_single(ctx):
    B, n0, n1 = 2, 300, 400
    pairs = [superpoint_like_pair(n0, n1, 200 + b) for b in range(B)]
    a = _lib.DeviceArray.from_numpy(ctx, np.stack([p[0] for p in pairs]))
    b = _lib.DeviceArray.from_numpy(ctx, np.stack([p[1] for p in pairs]))
    best = matcher.match_batch_device(a, b, ratio=1.0, ctx=ctx, cross_check=True)
    matcher.synchronize(ctx)
    best = best.numpy()
    for k in range(B):
        single = _check(*pairs[k], ctx, 1.0, oracle="c")
        got = np.nonzero(best[k] >= 0)[0]
        np.testing.assert_array_equal(np.stack([got, best[k][got]], 1), single)


# ---- query cache ---------------------------------------------------------------------
def test_query_cache_torch_cpu_tensors(ctx):
    """cache_query=True: the keyframe side stays packed across calls -- for both roles it plays --
    while the same unmodified torch tensor comes back; an in-place write repacks it."""
    torch = pytest.importorskip("torch")
    d0, d1 = mutual_ref.sift_near_duplicates(700, 800, 21, 150)
    d2 = np.ascontiguousarray(d1[::-1][:650])  # another frame seeing the same keyframe
    t0 = torch.from_numpy(d0.copy())[None]
    for other in (d1, d2, d1):
        _check(t0[0].numpy(), other, ctx, 0.75)  # the reference is informative for this pair
        got = matcher.match_knn2_ratio(t0, other, ctx=ctx, kind=matcher.DESC_SIFT, cache_query=True,
                                       cross_check=True)
        np.testing.assert_array_equal(got, mutual_ref.mutual(d0, other)[0])
    t0[0, 5, :] = t0[0, 9, :]  # in place: the cached rows (and column constants) are stale now
    m0 = t0[0].numpy().copy()
    got = matcher.match_knn2_ratio(t0, d1, ctx=ctx, kind=matcher.DESC_SIFT, cache_query=True, cross_check=True)
    np.testing.assert_array_equal(got, mutual_ref.mutual(m0, d1)[0])
    # a forward-only call on the same cached keyframe, then the cross check again
    got = matcher.match_knn2_ratio(t0, d2, ctx=ctx, kind=matcher.DESC_SIFT, cache_query=True)
    np.testing.assert_array_equal(got, match_ref.match_int(m0, d2))
    got = matcher.match_knn2_ratio(t0, d2, ctx=ctx, kind=matcher.DESC_SIFT, cache_query=True, cross_check=True)
    np.testing.assert_array_equal(got, mutual_ref.mutual(m0, d2)[0])
    # a float keyframe behind the cache
    f0, f1 = mutual_ref.superpoint_near_duplicates()
    tf = torch.from_numpy(f0.copy())[None]
    for _ in range(2):
        got = matcher.match_knn2_ratio(tf, f1, ctx=ctx, kind=matcher.DESC_FLOAT, cache_query=True, cross_check=True)
        np.testing.assert_array_equal(got, mutual_ref.mutual(f0, f1, oracle="c")[0])


def _raw_mutual(ctx, a, b, tag, flags=0, pa=None, pb=None, n0=None):
    n0 = a.shape[0] if n0 is None else n0
    out = np.empty((max(n0, 1), 2), dtype=np.int32)
    cnt = np.zeros(1, dtype=np.int32)
    rc = ctx.lib.vo_match_mutual(ctx.handle, C.c_void_p(a.ctypes.data if pa is None else pa), n0, C.c_uint64(tag),
                                 C.c_void_p(b.ctypes.data if pb is None else pb), b.shape[0], a.shape[1], 0.75,
                                 flags, ptr(out, C.c_int32), ptr(cnt, C.c_int32))
    return rc, out[: cnt[0]]


def test_query_cache_tag_and_pointer_keyed(ctx):
    """The C-level cache key: (pointer, n0, dim, tag).  The same tag with another pointer or
    size is a miss."""
    d0, d1 = mutual_ref.sift_near_duplicates(700, 900, 31, 150)
    e0 = np.roll(d0, 17, axis=0)  # other contents at another address, the same size
    for a in (d0, d0, e0, d0[:800].copy()):
        ref, n_forward = mutual_ref.mutual(a, d1)
        assert mutual_ref.informative(ref, n_forward)
        rc, got = _raw_mutual(ctx, a, d1, 7)
        assert rc == _lib.VO_OK
        np.testing.assert_array_equal(got, ref)


def test_device_pointer_flag(ctx):
    """VO_MATCH_DEVICE_PTRS: host memory is VO_ERR_ARG before any launch; the library's own
    device memory is accepted."""
    d0, d1 = mutual_ref.sift_near_duplicates(64, 64, 41, 32)
    ref, n_forward = mutual_ref.mutual(d0, d1)
    assert mutual_ref.informative(ref, n_forward)
    rc, _ = _raw_mutual(ctx, d0, d1, 0, _lib.VO_MATCH_DEVICE_PTRS)
    assert rc == _lib.VO_ERR_ARG
    a = _lib.DeviceArray.from_numpy(ctx, d0)
    b = _lib.DeviceArray.from_numpy(ctx, d1)
    for tag in (0, 9, 9):
        rc, got = _raw_mutual(ctx, d0, d1, tag, _lib.VO_MATCH_DEVICE_PTRS, a.ptr, b.ptr)
        assert rc == _lib.VO_OK
        np.testing.assert_array_equal(got, ref)
    rc, _ = _raw_mutual(ctx, d0, d1, 0, _lib.VO_MATCH_DEVICE_PTRS, a.ptr, b.ptr, n0=96 + 4096)
    assert rc == _lib.VO_ERR_ARG  # rows far past the allocation
    rc, _ = _raw_mutual(ctx, d0, d1, 0, 2)
    assert rc == _lib.VO_ERR_ARG  # an unknown flag bit
