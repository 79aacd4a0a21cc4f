"""The CPU restatement of the segment gate (``tests/segment_ref.py``) against plain float64
point-to-segment distance, and its tie to the circular gate of ``tests/gated_ref.py`` (no GPU)."""

import numpy as np
import pytest

from tests import gated_ref as G
from tests import segment_ref as S


@pytest.mark.parametrize("n0,n1", [(300, 400), (700, 900)])
@pytest.mark.parametrize("radius", [3.0, 8.0])
def test_gate_is_the_point_to_segment_distance(n0, n1, radius):
    """The division-free float32/float64 gate and the plain distance may differ only for pairs within
    1e-3 px of the boundary."""
    s = S.scene("sift", n0, n1, 1, radius=radius)
    cands = S.candidates(s.seg, s.radius, s.kp1)
    active = np.isfinite(s.seg).all(axis=1) & (s.radius >= 0)
    assert 0 < (~active).sum() <= 4 + (~s.valid).sum() and active.sum() > 0.9 * n0
    with np.errstate(invalid="ignore"):
        dist = S.point_segment_distance(s.seg, s.kp1)
    n_in = n_off = 0
    for i, c in enumerate(cands):
        if not active[i]:
            assert len(c) == 0
            continue
        inside = np.zeros(n1, bool)
        inside[c] = True
        plain = dist[i] <= radius
        off = inside != plain
        assert (np.abs(dist[i][off] - radius) < 1e-3).all()
        n_in += int(inside.sum())
        n_off += int(off.sum())
    assert n_in > n0 and n_off <= 2  # (0 at these shapes when this was written)
    seg_len = np.hypot(s.seg[active, 2] - s.seg[active, 0], s.seg[active, 3] - s.seg[active, 1])
    assert seg_len.max() > 350 and np.median(seg_len) > 20  # the capsules are long, not circles


def test_zero_length_segment_is_the_circular_gate():
    s = G.scene("sift", 300, 400, 1)
    seg = np.concatenate([s.pred, s.pred], axis=1)
    for radius in (s.radius, 0.0, 12.0, np.float32(15.999), np.inf, -1.0, np.nan):
        a, b = S.candidates(seg, radius, s.kp1), G.candidates(s.pred, radius, s.kp1)
        assert len(a) == len(b) == 300
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    ref = G.gated(s.d0, s.pred, s.radius, s.d1, s.kp1, 0.8, 300.0, True)
    got = S.segmented(s.d0, seg, s.radius, s.d1, s.kp1, 0.8, 300.0, True)
    assert G.informative(ref)
    np.testing.assert_array_equal(got.pairs, ref.pairs)
    np.testing.assert_array_equal(got.dist.view(np.uint32), ref.dist.view(np.uint32))
    assert (got.n_ratio, got.n_near, got.n_final) == (ref.n_ratio, ref.n_near, ref.n_final)


def test_hand_cases():
    kp = np.float32([[0, 0], [5, 3], [5, -3], [5, 3.001], [-3, 0], [-3.001, 0], [13, 0], [10, 3], [12, 2.5], [5, 0],
                     [np.nan, 0], [5, np.inf]])
    seg = np.float32([[0, 0, 10, 0], [10, 0, 0, 0], [0, 0, 0, 0], [0, 0, 10, np.nan]])
    c = S.candidates(seg, 3.0, kp)
    assert c[0].tolist() == [0, 1, 2, 4, 6, 7, 9]  # at exactly r from the interior and from both ends
    assert c[1].tolist() == c[0].tolist()  # a and b swapped: the same capsule
    assert c[2].tolist() == [0, 4] and len(c[3]) == 0
    assert [len(x) for x in S.candidates(seg, np.float32([np.inf, 0, -1, 3]), kp)] == [10, 2, 0, 0]
    assert S.candidates(seg, 0.0, kp)[0].tolist() == [0, 9]  # on the segment itself


def test_scene_is_informative():
    """What the GPU tests assert first, here for every scene shape they use."""
    for kind, md in (("sift", 300.0), ("float", 0.9)):
        for n0, n1 in ((300, 400), (700, 900)):
            s = S.scene(kind, n0, n1, 1)
            g = S.segmented(s.d0, s.seg, s.radius, s.d1, s.kp1, 0.8, md, True)
            assert S.informative(g), (np.bincount(np.minimum(g.n_cand, 3)), g.n_ratio, g.n_near, g.n_final)
            hit = s.truth[g.pairs[:, 0]] == g.pairs[:, 1]
            # the pairs are the planted ones; a near-duplicate (15 of every 75 matchable queries, truth -1)
            # may hold its original's keypoint instead
            assert hit.mean() > 0.75
