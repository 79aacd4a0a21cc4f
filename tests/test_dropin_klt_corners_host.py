"""``cfg.klt_corner_replenish`` in the wrapped frontend and VO methods on the host, with the stub
classes and the ``klt.track`` stand-in of ``test_dropin_klt_host.py`` and a stand-in
``corners.good_features`` (lattice points away from ``keep``): what the detector is called with,
the appended rows and their descriptor flag, the flag following its rows, the descriptor fallback
of ``match_frames``, the excluded combinations, and a switch that is off touching nothing (no GPU)."""

import numpy as np
import pytest

from tests.test_dropin_klt_host import (FLOW, Cfg, H, W, classes, detections, frame, matched, start,  # noqa: F401
                                        track)
from visualodometry_amd import corners, matcher
from visualodometry_amd.dropin import hooks
from visualodometry_amd.dropin.config.config import VOConfig, get_config


class CornerCfg(Cfg):
    klt_corner_replenish = True
    klt_corner_quality = 0.02
    klt_corner_block = 5


class Detector:
    """``corners.good_features`` stand-in: the points of a 10-pixel lattice at least ``min_distance``
    from every row of ``keep``, the first ``max_corners`` of them."""

    def __init__(self):
        self.calls = []

    def __call__(self, img, max_corners, quality=0.01, min_distance=8.0, mask=None, block_size=3, keep=None, tag=0,
                 ctx=None, shape=None):
        keep = np.asarray(keep, np.float32).reshape(-1, 2)
        self.calls.append(dict(k=int(img[0, 0]), max_corners=max_corners, quality=quality, min_distance=min_distance,
                               block_size=block_size, keep=keep.copy(), tag=tag, mask=mask))
        gx, gy = np.meshgrid(np.arange(10, W - 5, 10), np.arange(10, H - 5, 10))
        pts = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32)
        far = np.linalg.norm(pts[:, None] - keep[None], axis=2).min(1) >= min_distance if len(keep) else \
            np.ones(len(pts), bool)
        pts = pts[far][:max_corners]
        return pts, np.linspace(2, 1, len(pts)).astype(np.float32)


@pytest.fixture
def detector(monkeypatch):
    d = Detector()
    monkeypatch.setattr(corners, "good_features", d)
    return d


def make_keyframe(vo, track, lose=range(0, 150, 3), k=1):
    """Frame k tracked from the detected keyframe 0 and made the new keyframe."""
    track.lose = {k: list(lose)}
    f = vo.frontend.process_image(frame(k))
    pairs = vo.frontend.match_frames(vo.keyframe["feats"], f)
    ids = np.full(len(pairs), -1)
    ids[:40] = np.arange(40)
    vo._create_keyframe(f, ids, pairs[:, 0], pairs[:, 1])
    track.lose = {}
    return f, ids


def test_config_fields_are_off_by_default_and_the_switch_has_an_environment_name(monkeypatch):
    c = VOConfig()
    assert c.klt_corner_replenish is False and get_config("kitti").klt_corner_replenish is False
    assert (c.klt_corner_quality, c.klt_corner_block) == (0.01, 3)
    monkeypatch.setenv("VO_AMD_KLT_CORNERS", "1")
    cfg = get_config("kitti")
    assert cfg.klt_corner_replenish is True and cfg.klt_tracking is False


def test_replenishment_calls_the_detector_with_the_kept_points_and_the_tag(classes, track, detector):
    vo, f0 = start(classes, CornerCfg)
    f1, ids = make_keyframe(vo, track)
    assert vo.frontend.detected == [0]  # no SIFT detection on the keyframe's image
    assert len(detector.calls) == 1
    c = detector.calls[0]
    assert c["k"] == 1 and c["tag"] == f1[hooks._KLT_TAG] != 0 and c["mask"] is None
    assert (c["quality"], c["block_size"], c["min_distance"]) == (0.02, 5, Cfg.klt_min_distance)
    assert c["max_corners"] == Cfg.sift_n_features - 100
    np.testing.assert_array_equal(c["keep"], f1["keypoints"][0])
    feats, kids = vo.keyframe["feats"], vo.keyframe["ids"]
    kp, des, has = feats["keypoints"][0], feats["descriptors"][0], feats[hooks._KLT_HAS_DESC]
    n = Cfg.sift_n_features
    assert kp.shape == (n, 2) and des.shape == (n, 16) and has.shape == (n,) and has.dtype == bool
    assert feats["keypoints"].shape == (1, n, 2) and feats["descriptors"].shape == (1, n, 16)
    np.testing.assert_array_equal(kp[:100], f1["keypoints"][0])  # kept rows keep their indices
    np.testing.assert_array_equal(des[:100], f1["descriptors"][0])
    np.testing.assert_array_equal(kids[:100], ids)
    assert (kids[100:] == -1).all() and kids.shape == (n,)
    assert has[:100].all() and not has[100:].any() and not des[100:].any()
    assert np.linalg.norm(kp[100:, None] - kp[None, :100], axis=2).min() >= Cfg.klt_min_distance
    assert hooks._KLT_SRC not in feats and feats[hooks._KLT_IMAGE][0, 0] == 1
    assert vo._vo_amd_window.frames[-1].uv.shape == (100, 2)  # the window was fed before the replenishment


def test_no_room_appends_nothing_but_still_flags_the_rows(classes, track, detector):
    cfg = type("C", (CornerCfg,), {"sift_n_features": 100})
    vo, f0 = start(classes, cfg)
    make_keyframe(vo, track)
    assert not detector.calls
    feats = vo.keyframe["feats"]
    assert feats["keypoints"].shape == (1, 100, 2) and feats[hooks._KLT_HAS_DESC].all()


def test_the_flag_follows_its_rows_through_a_tracked_frame_and_the_next_keyframe(classes, track, detector):
    vo, f0 = start(classes, CornerCfg)
    make_keyframe(vo, track)
    kf = vo.keyframe["feats"]
    n = Cfg.sift_n_features
    lost = [2, 50, 99, 100, 101, 150]
    track.lose = {2: lost}
    f2 = vo.frontend.process_image(frame(2))
    assert len(track.calls[-1]["pts0"]) == n  # corners are tracked like every other row
    alive = np.delete(np.arange(n), lost)
    np.testing.assert_array_equal(f2[hooks._KLT_SRC_IDX], alive)
    np.testing.assert_array_equal(f2[hooks._KLT_HAS_DESC], kf[hooks._KLT_HAS_DESC][alive])
    np.testing.assert_array_equal(f2["descriptors"][0], kf["descriptors"][0][alive])
    np.testing.assert_array_equal(f2["keypoints"][0], kf["keypoints"][0][alive] + FLOW)
    pairs = vo.frontend.match_frames(kf, f2)
    np.testing.assert_array_equal(pairs, np.stack([alive, np.arange(len(alive))], 1))
    # the next keyframe: the carried flags first, then the new corners' false ones
    vo._create_keyframe(f2, np.full(len(alive), -1), pairs[:, 0], pairs[:, 1])
    k2 = vo.keyframe["feats"]
    has = k2[hooks._KLT_HAS_DESC]
    assert len(has) == n == k2["keypoints"].shape[1]
    np.testing.assert_array_equal(has[:len(alive)], f2[hooks._KLT_HAS_DESC])
    assert not has[len(alive):].any() and has.sum() == 97
    np.testing.assert_array_equal(detector.calls[-1]["keep"], f2["keypoints"][0])
    assert detector.calls[-1]["tag"] == f2[hooks._KLT_TAG] and detector.calls[-1]["max_corners"] == len(lost)


def test_descriptor_fallback_matches_flagged_rows_only_and_maps_back(classes, track, detector, monkeypatch):
    vo, f0 = start(classes, CornerCfg)
    make_keyframe(vo, track)
    kf = vo.keyframe["feats"]
    calls = []

    def knn(des0, des1, **kw):
        d0, d1 = np.asarray(des0), np.asarray(des1)
        calls.append((d0.copy(), d1.copy(), kw))
        m = min(d0.shape[-2], d1.shape[-2], 30)
        return np.stack([np.arange(m) * 3, np.arange(m)[::-1]], 1).astype(np.int64)  # (query, train) in sub-rows

    monkeypatch.setattr(matcher, "match_knn2_ratio", knn)
    track.lose = {2: "all"}  # nothing survives: frame 2 detects and is matched by descriptors
    f2 = vo.frontend.process_image(frame(2))
    assert vo.frontend.detected == [0, 2] and hooks._KLT_HAS_DESC not in f2
    # shuffle the flags so that the mapping is not the identity
    has = kf[hooks._KLT_HAS_DESC]
    has[:] = False
    rows = np.arange(5, 180, 2)
    has[rows] = True
    pairs = vo.frontend.match_frames(kf, f2)
    d0, d1, kw = calls[-1]
    np.testing.assert_array_equal(d0.reshape(-1, 16), kf["descriptors"][0][rows])
    np.testing.assert_array_equal(d1.reshape(-1, 16), f2["descriptors"][0])
    assert pairs.dtype == np.int64 and pairs.shape == (30, 2)
    np.testing.assert_array_equal(pairs[:, 0], rows[np.arange(30) * 3])
    np.testing.assert_array_equal(pairs[:, 1], np.arange(30)[::-1])
    # the flagged dict on the train side
    back = vo.frontend.match_frames(f2, kf)
    np.testing.assert_array_equal(back[:, 1], rows[np.arange(30)[::-1]])
    np.testing.assert_array_equal(back[:, 0], np.arange(30) * 3)
    # no row with a descriptor: nothing to match, the matcher is not called
    has[:] = False
    before = len(calls)
    none = vo.frontend.match_frames(kf, f2)
    assert none.shape == (0, 2) and none.dtype == np.int64 and len(calls) == before


@pytest.mark.parametrize("other", ["map_reobserve", "map_epipolar_search"])
def test_combinations_that_read_descriptors_of_keyframe_rows_raise(classes, other):
    fe_cls, vo_cls = classes
    cfg = type("C", (CornerCfg,), {other: True})
    with pytest.raises(ValueError, match=f"klt_corner_replenish cannot be combined with {other}"):
        fe_cls(cfg())
    fe_cls(type("C", (Cfg,), {other: True})())  # without the switch the combination stands as before


def test_switch_off_is_what_it_is_today(classes, track, detector, matched):
    class Raising(Cfg):
        def __getattr__(self, name):
            if name.startswith("klt_corner_") and name != "klt_corner_replenish":
                raise AssertionError(f"{name} read with the switch off")
            raise AttributeError(name)

    vo, f0 = start(classes, Raising)
    f1, ids = make_keyframe(vo, track)
    assert vo.frontend.detected == [0, 1] and not detector.calls  # replenished by detection, as today
    feats = vo.keyframe["feats"]
    assert set(feats) == {"keypoints", "descriptors", "image_size", hooks._KLT_IMAGE, hooks._KLT_TAG}
    assert feats["keypoints"].shape[1] == Cfg.sift_n_features
    det_kp = detections(1)[0]
    assert all((det_kp == p).all(1).any() for p in feats["keypoints"][0][100:])
    f2 = vo.frontend.process_image(frame(2))
    assert set(f2) == {"keypoints", "descriptors", "image_size", hooks._KLT_IMAGE, hooks._KLT_TAG, hooks._KLT_SRC,
                       hooks._KLT_SRC_IDX}
    track.lose = {3: "all"}
    f3 = vo.frontend.process_image(frame(3))
    vo.frontend.match_frames(feats, f3)
    assert len(matched) == 1 and matched[0][0] == (1, Cfg.sift_n_features, 16) and matched[0][2]["cache_query"]
