"""vo_match_hamming on the MI355X against a numpy restatement of its contract (include/vo_hip.h):
top-2 under keys (d, j), the keep rule, the cross check under keys (d, i), ascending output.  Sizes
sit below, at and above a wave and a workgroup and span several train slices and tiles; rows drawn
from a small pool make distances tie constantly, so both tie rules decide the result; host arrays
and device pointers agree; the existing float matcher on the unpacked bits agrees."""

import numpy as np
import pytest

from tests import brief_ref as R
from visualodometry_amd import _lib, brief, matcher

pytestmark = pytest.mark.gpu

INT_MAX = np.iinfo(np.int32).max
RATIOS = (0.0, 0.75, 1.0, 2.0)
MAX_DISTS = (0, 1, 40)


def rows(kind, n, words, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 1 << 32, (n, words), dtype=np.uint64).astype(np.uint32)
    # a pool of 16 distinct rows a few bits apart: distances tie constantly
    base = rng.integers(0, 1 << 32, words, dtype=np.uint64).astype(np.uint32)
    pool = np.tile(base, (16, 1))
    for k in range(16):
        pool[k, k % words] ^= np.uint32((k + 1) * 0x01010101 & 0xFFFFFFFF) if k else np.uint32(0)
    assert len({p.tobytes() for p in pool}) == 16
    return pool[rng.integers(0, 16, n)]


def ref_knn(d):
    """Top-2 of every row of the distance matrix under keys (d, j)."""
    n0, n1 = d.shape
    idx = np.full((n0, 2), -1, np.int32)
    dist = np.full((n0, 2), INT_MAX, np.int32)
    if n1:
        key = d * (1 << 32) + np.arange(n1)[None, :]
        order = np.argsort(key, axis=1, kind="stable")[:, :2]
        k = order.shape[1]
        idx[:, :k] = order
        dist[:, :k] = np.take_along_axis(d, order, 1)
    return idx, dist


def ref_match(d, idx, dist, ratio, max_dist, mutual):
    n0, n1 = d.shape
    pairs, dists = [], []
    if n1 >= 2 and n0:
        rev = np.argmin(d * (1 << 32) + np.arange(n0)[:, None], axis=0)  # smallest key (d(i', j), i') per j
        for i in range(n0):
            d1, d2, j1 = int(dist[i, 0]), int(dist[i, 1]), int(idx[i, 0])
            keep = (max_dist == 0 or d1 <= max_dist) and float(d1) < float(ratio) * float(d2)
            if keep and mutual:
                keep = rev[j1] == i
            if keep:
                pairs.append((i, j1))
                dists.append(d1)
    return np.array(pairs, np.int64).reshape(-1, 2), np.array(dists, np.int32)


def check_all(ctx, a, b, ratios=RATIOS, max_dists=MAX_DISTS, wrap=lambda x: x):
    d = R.hamming(a, b) if len(a) and len(b) else np.zeros((len(a), len(b)), np.int64)
    idx, dist = ref_knn(d)
    da, db = wrap(a), wrap(b)
    counts = []
    for ratio in ratios:
        for max_dist in max_dists:
            for mutual in (False, True):
                pairs, pd, (kidx, kdist) = matcher.match_hamming(da, db, ratio=ratio, max_dist=max_dist,
                                                                 cross_check=mutual, return_dist=True, return_knn=True,
                                                                 ctx=ctx)
                want, wd = ref_match(d, idx, dist, ratio, max_dist, mutual)
                what = f"ratio {ratio} max_dist {max_dist} mutual {mutual}"
                np.testing.assert_array_equal(kidx, idx, what)
                np.testing.assert_array_equal(kdist, dist, what)
                np.testing.assert_array_equal(pairs, want, what)
                np.testing.assert_array_equal(pd, wd, what)
                assert pairs.dtype == np.int64 and pd.dtype == np.int32
                if mutual:
                    assert len(set(pairs[:, 1].tolist())) == len(pairs)
                counts.append(len(want))
    return counts


SIZES = [(0, 5), (5, 0), (1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (63, 64), (64, 63), (65, 65), (64, 257), (257, 64),
         (257, 257), (3, 1000), (1000, 3), (1000, 1000)]


@pytest.mark.parametrize("n0, n1", SIZES)
@pytest.mark.parametrize("kind", ["random", "pool"])
def test_parity_with_the_restatement(ctx, n0, n1, kind):
    for words in (1, 8, 16):
        a, b = rows(kind, n0, words, 100 + n0), rows(kind, n1, words, 200 + n1)
        big = n0 * n1 >= 250000
        counts = check_all(ctx, a, b, ratios=(0.75, 2.0) if big else RATIOS, max_dists=(0, 40) if big else MAX_DISTS)
        if n0 >= 63 and n1 >= 63:
            assert max(counts) > 0 and min(counts) < max(counts)  # (the two pools differ: tied distances above 0)


def test_identical_sets_match_themselves(ctx):
    a = rows("random", 257, 8, 7)
    counts = check_all(ctx, a, a.copy())
    pairs = matcher.match_hamming(a, a, ratio=0.75, max_dist=1, cross_check=True, ctx=ctx)
    np.testing.assert_array_equal(pairs, np.stack([np.arange(257)] * 2, 1))
    assert max(counts) == 257
    # uint8 rows are the same rows
    p8 = matcher.match_hamming(a.view(np.uint8), a.view(np.uint8), ratio=0.75, max_dist=1, cross_check=True, ctx=ctx)
    np.testing.assert_array_equal(p8, pairs)


@pytest.mark.parametrize("words", [1, 3, 8, 11, 16])
def test_every_register_width_and_its_zero_padding(ctx, words):
    a, b = rows("random", 130, words, 11), rows("random", 70, words, 12)
    b[:35] = a[:35] ^ np.uint32(1)
    check_all(ctx, a, b, ratios=(0.75,), max_dists=(0, 40))


def test_several_train_slices_and_tiles(ctx):
    # 3 queries: one workgroup column, so the train rows are cut into the most slices; 16500 rows
    # make a slice longer than one LDS tile
    a = rows("random", 3, 8, 21)
    b = rows("pool", 16500, 8, 22)
    b[[5, 9000, 16499]] = a ^ np.uint32(2)
    b[[9001, 16400]] = a[1] ^ np.uint32(2)  # the tie on the second neighbour goes to the lower row
    counts = check_all(ctx, a, b, ratios=(0.75, 1.0), max_dists=(0, 40))
    assert max(counts) >= 2
    check_all(ctx, b[:9000], a, ratios=(2.0,), max_dists=(0,))  # and the reverse pass over many query rows


def test_device_pointers_agree_with_host_arrays(ctx):
    a, b = rows("pool", 257, 8, 31), rows("pool", 1000, 8, 32)
    keep = []

    def wrap(x):
        keep.append(_lib.DeviceArray.from_numpy(ctx, x))
        return keep[-1]

    host = check_all(ctx, a, b, ratios=(0.75, 2.0), max_dists=(0, 40))
    dev = check_all(ctx, a, b, ratios=(0.75, 2.0), max_dists=(0, 40), wrap=wrap)
    assert host == dev
    import torch

    # tensors torch holds on the host take the host path (this process gives torch no GPU)
    ta, tb = (torch.from_numpy(x.view(np.int32).copy()) for x in (a, b))
    got = matcher.match_hamming(ta, tb, ratio=0.75, max_dist=40, cross_check=True, ctx=ctx)
    np.testing.assert_array_equal(got, matcher.match_hamming(a, b, ratio=0.75, max_dist=40, cross_check=True, ctx=ctx))
    # a host pointer passed as a device pointer is refused before any launch
    opt = _lib.MatchHammingOptionsC(ratio=0.75, max_dist=0, flags=_lib.VO_MATCH_DEVICE_PTRS, reserved=0)
    out, cnt = np.zeros((257, 2), np.int32), np.zeros(1, np.int32)
    rc = ctx.lib.vo_match_hamming(ctx.handle, a.ctypes.data, 257, b.ctypes.data, 1000, 8, _lib.C.byref(opt),
                                  out.ctypes.data, None, _lib.ptr(cnt, _lib.C.c_int32), None, None)
    assert rc == _lib.VO_ERR_ARG


@pytest.mark.parametrize("kind", ["random", "pool"])
def test_the_float_matcher_on_the_unpacked_bits_agrees(ctx, kind):
    a, b = rows(kind, 130, 8, 41), rows(kind, 257, 8, 42)
    _, _, (kidx, kdist) = matcher.match_hamming(a, b, ratio=0.75, return_dist=True, return_knn=True, ctx=ctx)
    fidx, fdist = matcher.match_knn2(brief.unpack(a), brief.unpack(b), ctx=ctx)
    np.testing.assert_array_equal(fidx, kidx)
    np.testing.assert_array_equal(fdist, np.sqrt(kdist.astype(np.float32)))
