"""Hand-built known answers of the projection-gated matcher's CPU restatement (tests/gated_ref.py)."""

import numpy as np

from tests import gated_ref as G

F32 = np.float32


def _des(*rows):
    return np.array(rows, F32)


def test_boundary_345_is_inside_and_one_ulp_less_is_outside():
    pred = np.array([[10.0, 20.0]], F32)
    kp = np.array([[13.0, 24.0], [100.0, 100.0]], F32)  # (3, 4): distance exactly 5
    assert G.candidates(pred, 5.0, kp)[0].tolist() == [0]
    assert G.candidates(pred, np.nextafter(F32(5), F32(0)), kp)[0].tolist() == []
    d0, d1 = _des([1, 2, 3]), _des([1, 2, 4], [9, 9, 9])
    assert G.gated(d0, pred, 5.0, d1, kp).pairs.tolist() == [[0, 0]]
    assert G.gated(d0, pred, np.nextafter(F32(5), F32(0)), d1, kp).pairs.tolist() == []


def test_zero_radius_admits_a_coincident_keypoint_only():
    pred = np.array([[7.5, 3.25]], F32)
    kp = np.array([[7.5, np.nextafter(F32(3.25), F32(4))], [7.5, 3.25]], F32)
    assert G.candidates(pred, 0.0, kp)[0].tolist() == [1]
    g = G.gated(_des([0, 0]), pred, 0.0, _des([5, 5], [3, 4]), kp)
    assert g.pairs.tolist() == [[0, 1]] and g.dist.tolist() == [5.0]


def test_inactive_queries_and_keypoints():
    pred = np.array([[1, 1], [np.nan, 1], [1, np.inf], [1, 1], [1, 1], [1, 1]], F32)
    radius = np.array([2, 2, 2, -1, np.nan, np.inf], F32)
    kp = np.array([[1, 1], [np.nan, 1], [1, -np.inf], [1e30, -1e30]], F32)
    c = [x.tolist() for x in G.candidates(pred, radius, kp)]
    # +inf admits every keypoint with finite coordinates, and none with a non-finite one
    assert c == [[0], [], [], [], [], [0, 3]]


def test_lone_candidate_passes_the_ratio_test_and_max_dist_rejects_it():
    pred = np.array([[0.0, 0.0]], F32)
    kp = np.array([[1.0, 0.0], [50.0, 0.0]], F32)
    d0, d1 = _des([0, 0]), _des([30, 40], [0, 0])
    g = G.gated(d0, pred, 2.0, d1, kp, ratio=0.5)
    assert g.pairs.tolist() == [[0, 0]] and g.dist.tolist() == [50.0]
    assert G.gated(d0, pred, 2.0, d1, kp, ratio=0.5, max_dist=50.0).pairs.tolist() == [[0, 0]]  # <=
    g = G.gated(d0, pred, 2.0, d1, kp, ratio=0.5, max_dist=49.9)
    assert g.pairs.tolist() == [] and (g.n_ratio, g.n_near) == (1, 0)


def test_equal_distances_keep_the_lower_train_index():
    pred = np.array([[0.0, 0.0]], F32)
    kp = np.zeros((3, 2), F32)
    d1 = _des([9, 9], [3, 4], [4, 3])  # rows 1 and 2 both at distance 5
    assert G.gated(_des([0, 0]), pred, 1.0, d1, kp, ratio=10.0).pairs.tolist() == [[0, 1]]


def test_equal_best_and_second_fail_a_ratio_below_one():
    pred = np.array([[0.0, 0.0]], F32)
    kp = np.zeros((2, 2), F32)
    d1 = _des([3, 4], [4, 3])
    assert G.gated(_des([0, 0]), pred, 1.0, d1, kp, ratio=0.999).pairs.tolist() == []
    assert G.gated(_des([0, 0]), pred, 1.0, d1, kp, ratio=1.001).pairs.tolist() == [[0, 0]]


def test_unique_keeps_the_nearest_query_and_the_lower_query_on_a_tie():
    pred = np.zeros((3, 2), F32)
    kp = np.zeros((1, 2), F32)
    d1 = _des([0, 0])
    g = G.gated(_des([3, 4], [4, 3], [0, 6]), pred, 1.0, d1, kp)
    assert g.pairs.tolist() == [[0, 0]] and (g.n_near, g.n_final) == (3, 1)
    g = G.gated(_des([3, 4], [4, 3], [0, 4]), pred, 1.0, d1, kp)
    assert g.pairs.tolist() == [[2, 0]] and g.dist.tolist() == [4.0]
    assert G.gated(_des([3, 4], [4, 3], [0, 4]), pred, 1.0, d1, kp, unique=False).pairs.tolist() == \
        [[0, 0], [1, 0], [2, 0]]


def test_a_distance_that_is_not_below_flt_max_is_never_selected():
    pred = np.zeros((1, 2), F32)
    kp = np.zeros((3, 2), F32)
    big = np.finfo(F32).max
    d1 = _des([np.nan, 0], [big, big], [1, 0])  # NaN, an overflowing chain (+inf), and one real row
    g = G.gated(_des([0, 0]), pred, 1.0, d1, kp, ratio=0.1)
    assert g.pairs.tolist() == [[0, 2]]  # the lone selected candidate


def test_scene_builder_is_informative_and_seeded():
    s = G.scene("sift", 300, 400, 1)
    g = G.gated(s.d0, s.pred, s.radius, s.d1, s.kp1, 0.8, 300.0)
    assert G.informative(g)
    assert len(np.unique(g.pairs[:, 1])) == len(g.pairs)
    assert (g.pairs[:, 1] == s.truth[g.pairs[:, 0]]).mean() > 0.9
    t = G.scene("sift", 300, 400, 1)
    assert np.array_equal(s.d0, t.d0) and np.array_equal(s.kp1, t.kp1)
