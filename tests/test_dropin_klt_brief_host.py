"""``cfg.klt_corner_describe`` in the wrapped frontend and VO methods on the host, with the stub
classes and stand-ins of ``test_dropin_klt_host.py`` / ``test_dropin_klt_corners_host.py`` and
stand-in ``brief.describe`` and ``matcher.match_hamming``: the BRIEF rows a keyframe keeps, the key
following its rows, the corners a fallback frame receives, the union of SIFT and Hamming pairs mapped
back to dict rows, empty sides, and a switch that is off touching nothing (no GPU)."""

import numpy as np
import pytest

from tests.test_dropin_klt_corners_host import CornerCfg, Detector, detector, make_keyframe  # noqa: F401
from tests.test_dropin_klt_host import Cfg, H, W, classes, frame, matched, start, track  # noqa: F401
from visualodometry_amd import brief, matcher
from visualodometry_amd.dropin import hooks
from visualodometry_amd.dropin.config.config import VOConfig, get_config


class BriefCfg(CornerCfg):
    klt_corner_describe = True
    klt_brief_ratio = 0.7
    klt_brief_max_dist = 50


def row_of(pts, k):
    """The stand-in descriptor of points (n, 2) in frame k: word 0 = frame, 1 = x, 2 = y, 3 = 1."""
    p = np.asarray(pts, np.float32).reshape(-1, 2)
    out = np.zeros((len(p), 8), np.uint32)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = k, p[:, 0], p[:, 1], 1
    return out


@pytest.fixture
def describer(monkeypatch):
    calls = []

    def describe(img, pts, tag=0, ctx=None, shape=None):
        k = int(img[0, 0])
        calls.append(dict(k=k, pts=np.array(pts, np.float32), tag=tag))
        n = len(pts)
        return row_of(pts, k), np.zeros(n, np.int32), np.zeros(n, np.uint8)

    monkeypatch.setattr(brief, "describe", describe)
    return calls


@pytest.fixture
def hamming(monkeypatch):
    calls = []

    def match(des0, des1, ratio=0.8, max_dist=None, cross_check=False, return_dist=False, return_knn=False, ctx=None):
        calls.append(dict(des0=np.array(des0), des1=np.array(des1), ratio=ratio, max_dist=max_dist,
                          cross_check=cross_check))
        m = min(len(des0), len(des1), 7)
        return np.stack([np.arange(m) * 2, np.arange(m)[::-1]], 1).astype(np.int64)  # sub-rows (query, train)

    monkeypatch.setattr(matcher, "match_hamming", match)
    return calls


def test_config_fields_are_off_by_default_and_the_switch_has_an_environment_name(monkeypatch):
    c = VOConfig()
    assert c.klt_corner_describe is False and get_config("kitti").klt_corner_describe is False
    assert (c.klt_brief_ratio, c.klt_brief_max_dist) == (0.8, 64)
    monkeypatch.setenv("VO_AMD_KLT_BRIEF", "1")
    cfg = get_config("kitti")
    assert cfg.klt_corner_describe is True and cfg.klt_corner_replenish is False and cfg.klt_tracking is False


@pytest.mark.parametrize("other", ["map_reobserve", "map_epipolar_search"])
def test_the_exclusions_of_corner_replenishment_stay(classes, other):
    fe_cls, _ = classes
    with pytest.raises(ValueError, match=f"klt_corner_replenish cannot be combined with {other}"):
        fe_cls(type("C", (BriefCfg,), {other: True})())


def test_keyframe_keeps_brief_rows_and_they_follow_their_rows(classes, track, detector, describer):
    vo, f0 = start(classes, BriefCfg)
    f1, ids = make_keyframe(vo, track)
    kf = vo.keyframe["feats"]
    n = Cfg.sift_n_features
    rows, has, kp = kf[hooks._KLT_BRIEF], kf[hooks._KLT_HAS_DESC], kf["keypoints"][0]
    assert rows.shape == (n, 8) and rows.dtype == np.uint32 and not rows[:100].any()
    assert len(describer) == 1 and describer[0]["k"] == 1 and describer[0]["tag"] == f1[hooks._KLT_TAG] != 0
    np.testing.assert_array_equal(describer[0]["pts"], kp[100:])
    np.testing.assert_array_equal(rows[100:], row_of(kp[100:], 1))
    assert has[:100].all() and not has[100:].any()
    # a tracked frame carries the key along with its rows, and so does the next keyframe
    lost = [2, 50, 99, 100, 101, 150]
    track.lose = {2: lost}
    f2 = vo.frontend.process_image(frame(2))
    alive = np.delete(np.arange(n), lost)
    np.testing.assert_array_equal(f2[hooks._KLT_BRIEF], rows[alive])
    np.testing.assert_array_equal(f2[hooks._KLT_HAS_DESC], has[alive])
    pairs = vo.frontend.match_frames(kf, f2)
    vo._create_keyframe(f2, np.full(len(alive), -1), pairs[:, 0], pairs[:, 1])
    k2 = vo.keyframe["feats"]
    r2, kp2 = k2[hooks._KLT_BRIEF], k2["keypoints"][0]
    assert r2.shape == (n, 8) and len(describer) == 2 and describer[1]["k"] == 2
    np.testing.assert_array_equal(r2[:len(alive)], rows[alive])  # carried, not described again
    np.testing.assert_array_equal(r2[len(alive):], row_of(kp2[len(alive):], 2))
    assert hooks._KLT_SRC not in k2


def test_no_room_keeps_zero_rows_and_describes_nothing(classes, track, detector, describer):
    vo, f0 = start(classes, type("C", (BriefCfg,), {"sift_n_features": 100}))
    make_keyframe(vo, track)
    kf = vo.keyframe["feats"]
    assert not describer and kf[hooks._KLT_BRIEF].shape == (100, 8) and not kf[hooks._KLT_BRIEF].any()


def fallback(vo, track, k=2):
    track.lose = {k: "all"}
    f = vo.frontend.process_image(frame(k))
    track.lose = {}
    return f


def test_fallback_frame_receives_described_corners(classes, track, detector, describer):
    vo, f0 = start(classes, BriefCfg)
    f1, _ = make_keyframe(vo, track)
    f2 = fallback(vo, track)
    assert vo.frontend.detected == [0, 2] and hooks._KLT_SRC not in f2
    n = Cfg.sift_n_features
    kp, des, has, rows = f2["keypoints"][0], f2["descriptors"][0], f2[hooks._KLT_HAS_DESC], f2[hooks._KLT_BRIEF]
    assert kp.shape == (n, 2) and des.shape == (n, 16) and f2["keypoints"].shape == (1, n, 2)
    assert has[:150].all() and not has[150:].any() and not des[150:].any() and not rows[:150].any()
    c = detector.calls[-1]
    assert c["k"] == 2 and c["max_corners"] == n - 150 and c["tag"] == f2[hooks._KLT_TAG] != 0
    assert (c["quality"], c["block_size"], c["min_distance"]) == (0.02, 5, Cfg.klt_min_distance)
    np.testing.assert_array_equal(c["keep"], kp[:150])
    assert describer[-1]["k"] == 2 and describer[-1]["tag"] == f2[hooks._KLT_TAG]
    np.testing.assert_array_equal(describer[-1]["pts"], kp[150:])
    np.testing.assert_array_equal(rows[150:], row_of(kp[150:], 2))
    assert np.linalg.norm(kp[150:, None] - kp[None, :150], axis=2).min() >= Cfg.klt_min_distance
    # the first frame of a drive is no fallback: detected as without the route
    assert set(f0) == {"keypoints", "descriptors", "image_size", hooks._KLT_IMAGE, hooks._KLT_TAG}


def test_union_of_pairs_is_mapped_back_and_one_to_one(classes, track, detector, describer, hamming, monkeypatch):
    vo, f0 = start(classes, BriefCfg)
    make_keyframe(vo, track)
    kf = vo.keyframe["feats"]
    f2 = fallback(vo, track)

    def knn(des0, des1, **kw):
        m = min(np.asarray(des0).shape[-2], np.asarray(des1).shape[-2], 30)
        return np.stack([np.arange(m) * 3, np.arange(m)[::-1]], 1).astype(np.int64)

    monkeypatch.setattr(matcher, "match_knn2_ratio", knn)
    # shuffle both flags so that neither mapping is the identity (the BRIEF rows stay with their rows)
    has0, has1 = kf[hooks._KLT_HAS_DESC], f2[hooks._KLT_HAS_DESC]
    has0[:] = True
    has0[3::4] = False
    has1[:] = True
    has1[1::5] = False
    d0, d1 = np.flatnonzero(has0), np.flatnonzero(has1)
    c0, c1 = np.flatnonzero(~has0), np.flatnonzero(~has1)
    pairs = vo.frontend.match_frames(kf, f2)
    h = hamming[-1]
    assert (h["ratio"], h["max_dist"], h["cross_check"]) == (0.7, 50, True)
    np.testing.assert_array_equal(h["des0"], kf[hooks._KLT_BRIEF][c0])
    np.testing.assert_array_equal(h["des1"], f2[hooks._KLT_BRIEF][c1])
    want = np.concatenate([np.stack([d0[np.arange(30) * 3], d1[np.arange(30)[::-1]]], 1),
                           np.stack([c0[np.arange(7) * 2], c1[np.arange(7)[::-1]]], 1)])
    want = want[np.argsort(want[:, 0], kind="stable")]
    assert pairs.dtype == np.int64
    np.testing.assert_array_equal(pairs, want)
    assert len(set(pairs[:, 0].tolist())) == len(pairs) == len(set(pairs[:, 1].tolist())) == 37
    assert (has0[pairs[:, 0]] == has1[pairs[:, 1]]).all()  # descriptor rows with descriptor rows, corners with corners


def test_an_empty_side_gives_no_pairs_from_that_part(classes, track, detector, describer, hamming, matched):
    vo, f0 = start(classes, BriefCfg)
    make_keyframe(vo, track)
    kf = vo.keyframe["feats"]
    f2 = fallback(vo, track)
    has0, has1 = kf[hooks._KLT_HAS_DESC], f2[hooks._KLT_HAS_DESC]
    keep0, keep1 = has0.copy(), has1.copy()
    has1[:] = True  # the frame has no corner rows: SIFT part only, the Hamming matcher is not called
    assert vo.frontend.match_frames(kf, f2).shape == (0, 2) and len(matched) == 1 and not hamming
    has1[:] = keep1
    has0[:] = False  # the keyframe has no descriptor rows: Hamming part only, the SIFT matcher is not called
    pairs = vo.frontend.match_frames(kf, f2)
    assert len(matched) == 1 and len(hamming) == 1 and pairs.shape == (7, 2)
    np.testing.assert_array_equal(pairs[:, 0], np.arange(7) * 2)
    np.testing.assert_array_equal(pairs[:, 1], np.flatnonzero(~keep1)[np.arange(7)[::-1]])
    has0[:] = keep0
    # a frame detected without corners (no flags, no BRIEF rows): the SIFT part as before
    f3 = {k: v for k, v in f2.items() if k not in (hooks._KLT_HAS_DESC, hooks._KLT_BRIEF)}
    assert vo.frontend.match_frames(kf, f3).shape == (0, 2) and len(matched) == 2 and len(hamming) == 1


def test_switch_off_reads_no_new_setting_and_adds_no_key(classes, track, detector, describer, hamming, matched):
    class Raising(CornerCfg):
        def __getattr__(self, name):
            if name.startswith("klt_brief_"):
                raise AssertionError(f"{name} read with the switch off")
            raise AttributeError(name)

    vo, f0 = start(classes, Raising)
    make_keyframe(vo, track)
    kf = vo.keyframe["feats"]
    assert set(kf) == {"keypoints", "descriptors", "image_size", hooks._KLT_IMAGE, hooks._KLT_TAG, hooks._KLT_HAS_DESC}
    f2 = vo.frontend.process_image(frame(2))
    assert hooks._KLT_BRIEF not in f2
    f3 = fallback(vo, track, 3)
    assert set(f3) == {"keypoints", "descriptors", "image_size", hooks._KLT_IMAGE, hooks._KLT_TAG}
    assert len(detector.calls) == 1  # the keyframe's replenishment only
    vo.frontend.match_frames(kf, f3)
    assert not describer and not hamming and len(matched) == 1

    class NoCorners(Cfg):  # without klt_corner_replenish the switch itself is never read
        def __getattr__(self, name):
            if name.startswith("klt_brief_") or name == "klt_corner_describe":
                raise AssertionError(f"{name} read without klt_corner_replenish")
            raise AttributeError(name)

    vo, f0 = start(classes, NoCorners)
    assert vo.frontend._vo_amd_klt.describe is False
    vo.frontend.process_image(frame(1))
