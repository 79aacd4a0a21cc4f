"""``oracle/sift_ref.select_keypoints`` (the sort, removeDuplicatedSorted and retainBest of the
SIFT oracle) against an independent restatement, on the cases of tests/sift_select_cases.py, and
the shape of every case against what it claims to be (no GPU).

The restatement sorts record indices with ``functools.cmp_to_key`` over a literal
KeyPoint12_LessThan (OpenCV ``modules/features2d/src/keypoint.cpp``: x, y ascending, size
descending, angle ascending, response, octave descending, then ``i < j``), drops a record that
equals its predecessor in x, y, size and angle, and cuts at the nfeatures-th largest response,
keeping ties.  The shape assertions keep a later edit of a generator from emptying a GPU test
(tests/test_gpu_sift_select.py runs the same cases).
"""

import collections
import functools

import numpy as np
import pytest

from oracle import sift_ref
from tests import sift_select_cases as G


def restated_select(okp_img, n, nfeatures):
    rows = [tuple(r[:5].tolist()) + (int(r[5:6].view(np.int32)[0]),) for r in np.ascontiguousarray(okp_img[:n])]

    def less(i, j):  # KeyPoint12_LessThan
        a, b = rows[i], rows[j]
        if a[0] != b[0]:
            return a[0] < b[0]
        if a[1] != b[1]:
            return a[1] < b[1]
        if a[2] != b[2]:
            return a[2] > b[2]
        if a[3] != b[3]:
            return a[3] < b[3]
        if a[4] != b[4]:
            return a[4] > b[4]
        if a[5] != b[5]:
            return a[5] > b[5]
        return i < j

    order = sorted(range(n), key=functools.cmp_to_key(lambda i, j: -1 if less(i, j) else (1 if less(j, i) else 0)))
    kept = []
    for i in order:
        if kept and rows[kept[-1]][:4] == rows[i][:4]:
            continue
        kept.append(i)
    if nfeatures > 0 and len(kept) > nfeatures:
        thr = sorted((rows[i][4] for i in kept), reverse=True)[nfeatures - 1]
        kept = [i for i in kept if rows[i][4] >= thr]
    return kept


@pytest.mark.parametrize("name", G.NAMES)
def test_select_keypoints_equals_restatement(name):
    okp, counts, nfeatures, cap_img = G.case(name)
    ref = G.reference(name)
    for b in range(len(counts)):
        n = int(counts[b])
        kps = G.records(okp[b], n)
        out, idx = sift_ref.select_keypoints(kps, nfeatures)
        assert list(ref[b]) == idx == restated_select(okp[b], n, nfeatures), f"image {b}"
        assert all(o is kps[i] for o, i in zip(out, idx))


def _per_image(claim, batch):
    return claim if isinstance(claim, list) else [claim] * batch


@pytest.mark.parametrize("name", G.NAMES)
def test_case_has_the_shape_it_claims(name):
    okp, counts, nfeatures, cap_img = G.case(name)
    facts, claims = G.facts(name), G.CLAIMS[name]
    batch = len(counts)
    assert okp.shape == (batch, cap_img, 8) and okp.dtype == np.float32 and 16 <= cap_img <= 8192
    for b, f in enumerate(facts):
        r = okp[b, :f["n"]]
        # inside the key range, positive normal responses, positive octave words, zero padding
        assert ((r[:, :2] >= G.XY_LO) & (r[:, :2] < G.XY_HI)).all()
        assert (r[:, 4] >= np.finfo(np.float32).tiny).all() and np.isfinite(r[:, 4]).all()
        assert (r[:, 5].view(np.int32) > 0).all() and (r[:, 6:] == 0).all()
        # the queue of long runs overflows only where the case says so
        if "nlong" not in claims:
            assert f["nlong"] <= G.K_LONG_QUEUE
        assert f["kept"] == len(restated_select(okp[b], f["n"], 0))
    for key in ("n", "nlong", "longest", "dups", "kept", "tie", "sep_byte"):
        if key in claims:
            assert [f[key] for f in facts] == _per_image(claims[key], batch), key
    if "lengths" in claims:
        assert [set(f["lengths"].tolist()) for f in facts] == _per_image(claims["lengths"], batch)
    if "digit" in claims:
        for f, (p, d) in zip(facts, claims["digit"]):
            assert (f["thr_bits"] >> (8 * p)) & 255 == d and f["tie"] >= 1
    if "last_runs" in claims:
        for f, (L, t) in zip(facts, claims["last_runs"]):
            assert f["lengths"][-1 - t] == L and (f["lengths"][len(f["lengths"]) - t:] == 1).all()
            assert f["starts"][-1 - t] == f["n"] - L - t
    if "placed" in claims:
        for f, placed in zip(facts, claims["placed"]):
            runs = dict(zip(f["starts"].tolist(), f["lengths"].tolist()))
            assert all(runs.get(s) == L for s, L in placed.items())
    for b in claims.get("zero_images", []):
        assert counts[b] == 0
    for b in claims.get("full_images", []):
        assert counts[b] == cap_img
    if claims.get("shared_xy"):
        seen = collections.Counter(p for b, f in enumerate(facts) for p in set(map(tuple, okp[b, :f["n"], :2].tolist())))
        assert sum(v >= 2 for v in seen.values()) >= 4  # (x, y) values present in more than one image


def test_cases_cover_both_sides_of_the_thresholds():
    """Run lengths on both sides of the register limit, and long-run counts on both sides of the
    queue limit, are present among the cases."""
    lengths = set()
    for name in ("run_lengths", "run_tails", "levels_register", "levels_insertion"):
        for f in G.facts(name):
            lengths |= set(f["lengths"].tolist())
    assert {G.K_RUN_MAX - 1, G.K_RUN_MAX, G.K_RUN_MAX + 1} <= lengths
    nlong = sorted(G.facts(n)[0]["nlong"] for n in ("long_queue_2048", "long_queue_2049", "long_queue_2100"))
    assert nlong == [G.K_LONG_QUEUE, G.K_LONG_QUEUE + 1, 2100]


def test_coordinates_include_float32_neighbours_and_equal_x_runs():
    okp, counts, _, _ = G.case("long_queue_2100")
    r = okp[0, :counts[0]]
    xs = np.unique(r[:, 0])
    assert (np.nextafter(xs[:-1], np.float32(np.inf)) == xs[1:]).any()
    xy = np.unique(r[:, :2], axis=0)
    assert (np.unique(xy[:, 0], return_counts=True)[1] > 1).any()


def test_overflow_case():
    okp, counts, nfeatures, cap_img = G.overflow()
    assert list(counts) == G.OVERFLOW_COUNTS and counts[1] > cap_img and okp.shape == (3, cap_img, 8)
