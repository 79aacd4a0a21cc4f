"""``matcher.epipolar_segments`` by its properties (host plumbing, no GPU): a point whose depth lies
in the range projects onto its segment; valid segments lie inside the image; what cannot be seen is
invalid; forward motion gives segments through the epipole; ``min_length`` is honoured."""

import numpy as np

from tests import segment_ref as S
from visualodometry_amd import matcher
from visualodometry_amd.synthetic import KITTI_K, KITTI_WH

W, H = KITTI_WH
K = np.asarray(KITTI_K, np.float64)


def _dist(seg, p):
    return np.array([S.point_segment_distance(seg[i:i + 1], p[i:i + 1])[0, 0] for i in range(len(seg))])


def test_a_point_in_the_depth_range_projects_onto_its_segment():
    s = S.scene("sift", 700, 900, 1)
    seg, valid = matcher.epipolar_segments(s.kp0, s.T_cw0, s.T_cw1, s.K, s.size, S.Z_MIN, S.Z_MAX)
    assert seg.dtype == np.float32 and seg.shape == (700, 4) and valid.dtype == bool and valid.shape == (700,)
    seen = np.flatnonzero(s.truth >= 0)
    assert len(seen) > 300 and ((s.depth[seen] >= S.Z_MIN) & (s.depth[seen] <= S.Z_MAX)).all()
    assert valid[seen].all()
    # float32 segment ends and keypoints: about 1e-4 px at these coordinates, inside the 1e-3 asked for
    assert _dist(seg[seen], s.proj1[seen]).max() < 1e-3
    # a tighter range still holds every point inside it, and only those
    seg2, valid2 = matcher.epipolar_segments(s.kp0, s.T_cw0, s.T_cw1, s.K, s.size, 10.0, 30.0)
    mid = seen[(s.depth[seen] >= 10) & (s.depth[seen] <= 30)]
    out = seen[(s.depth[seen] < 8) | (s.depth[seen] > 36)]
    assert len(mid) > 50 and len(out) > 50 and valid2[mid].all()
    assert _dist(seg2[mid], s.proj1[mid]).max() < 1e-3
    far = out[valid2[out]]
    assert (_dist(seg2[far], s.proj1[far]) > 1e-3).mean() > 0.9  # (a point near the epipole hardly moves)


def test_valid_segments_lie_inside_the_image_and_invalid_rows_are_inactive():
    s = S.scene("sift", 700, 900, 1)
    seg, valid = matcher.epipolar_segments(s.kp0, s.T_cw0, s.T_cw1, s.K, s.size, S.Z_MIN, S.Z_MAX)
    v = seg[valid]
    assert 0 < (~valid).sum() < 70
    assert (v[:, [0, 2]] >= 0).all() and (v[:, [0, 2]] <= W).all() and (v[:, [1, 3]] >= 0).all() and \
        (v[:, [1, 3]] <= H).all()
    assert np.isnan(seg[~valid]).all()
    assert all(len(c) == 0 for c in S.candidates(seg[~valid], 1e9, s.kp1))
    # a is the near end: for this forward motion the nearer a point, the farther from the epipole
    T10 = s.T_cw1 @ np.linalg.inv(s.T_cw0)
    e = K @ T10[:3, 3]
    e = e[:2] / e[2]
    assert (np.hypot(*(v[:, :2] - e).T) >= np.hypot(*(v[:, 2:] - e).T) - 1e-3).all()


def test_behind_the_camera_and_outside_the_image_are_invalid():
    T0 = np.eye(4)
    back = np.eye(4)
    back[:3, :3] = np.diag([-1.0, 1.0, -1.0])  # camera 1 looks the other way from the same place
    kp = np.float32([[600, 180], [100, 50], [1200, 300]])
    _, valid = matcher.epipolar_segments(kp, T0, back, K, (W, H), 1.0, 100.0)
    assert not valid.any()
    # a sideways step of 50 m: everything nearer than 50 m projects far outside the image
    side = np.eye(4)
    side[0, 3] = -50.0
    seg, valid = matcher.epipolar_segments(kp, T0, side, K, (W, H), 1.0, 20.0)
    assert not valid.any()
    seg, valid = matcher.epipolar_segments(kp, T0, side, K, (W, H), 1.0, np.inf)
    assert valid.all()  # the far part of the ray comes back into the image: it ends at the keypoint itself
    np.testing.assert_allclose(seg[:, 2:], kp, atol=1e-4)
    assert (seg[:, 0] == 0).all()  # ... and was clipped where it enters at the left border
    # a ray crossing camera 1's plane is cut, not dropped: camera 1 five metres ahead
    ahead = np.eye(4)
    ahead[2, 3] = -5.0
    seg, valid = matcher.epipolar_segments(kp, T0, ahead, K, (W, H), 1.0, np.inf)
    assert valid.all() and np.isfinite(seg).all()
    e, v = matcher.epipolar_segments(np.zeros((0, 2)), T0, ahead, K, (W, H), 1.0)
    assert e.shape == (0, 4) and v.shape == (0,)


def test_forward_motion_points_at_the_epipole_and_min_length_is_honoured():
    T0, T1 = np.eye(4), np.eye(4)
    T1[2, 3] = -1.0  # one metre straight ahead: the epipole is the principal point
    rng = np.random.default_rng(0)
    kp = np.stack([rng.uniform(0, W, 200), rng.uniform(0, H, 200)], axis=1).astype(np.float32)
    seg, valid = matcher.epipolar_segments(kp, T0, T1, K, (W, H), 2.0, np.inf)
    assert valid.all()
    e = K[:2, 2]
    a, b = seg[:, :2].astype(np.float64), seg[:, 2:].astype(np.float64)
    # the far end is the vanishing point, the keypoint itself under pure translation
    np.testing.assert_allclose(b, kp, atol=1e-4)
    cross = (a[:, 0] - e[0]) * (b[:, 1] - e[1]) - (a[:, 1] - e[1]) * (b[:, 0] - e[0])
    assert (np.abs(cross) / np.maximum(np.hypot(*(a - e).T), 1.0) < 1e-3).all()  # e, b, a on one line
    length = np.hypot(*(b - a).T)
    assert length.min() < 8.0 < length.max()
    for m in (0.0, 8.0, 50.0):
        _, v = matcher.epipolar_segments(kp, T0, T1, K, (W, H), 2.0, np.inf, min_length=m)
        np.testing.assert_array_equal(v, length >= m)
