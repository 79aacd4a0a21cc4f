"""``cfg.klt_tracking`` in the wrapped frontend and VO methods on the host, with stub frontend and
VO classes and a stand-in ``klt.track`` (planted per-frame flow, chosen points lost): the pairs a
tracked frame brings, lost points never returning, the fallback below ``klt_min_tracks``, the
replenishment of a new keyframe, reset, and a route that is off touching nothing (no GPU)."""

import numpy as np
import pytest

from visualodometry_amd import klt, matcher
from visualodometry_amd.dropin import hooks
from visualodometry_amd.dropin.config.config import VOConfig, get_config

H, W = 240, 400
FLOW = np.float32((2.0, 1.0))  # per frame


def frame(k):
    """Frame k as an image: the stand-ins read the frame number from its first pixel."""
    img = np.zeros((H, W), np.uint8)
    img[0, 0] = k
    return img


def detections(k, n=150):
    rng = np.random.default_rng(100 + k)
    kp = np.stack([rng.uniform(5, W - 5, n), rng.uniform(5, H - 5, n)], 1).astype(np.float32)
    return kp[np.argsort(kp[:, 0], kind="stable")], rng.integers(0, 256, (n, 16)).astype(np.float32)


class Cfg:
    extractor_type = "sift"
    match_on_gpu = True
    sift_on_gpu = False
    sift_n_features = 180
    ba_enabled = False
    klt_tracking = True
    klt_min_tracks = 20
    klt_min_distance = 8.0


class Frontend:
    def __init__(self, config):
        self.conf = config
        self.detected = []

    def process_image(self, img):
        k = int(np.ravel(img)[0])
        self.detected.append(k)
        kp, des = detections(k)
        return {"keypoints": kp[None], "descriptors": des[None], "image_size": np.array([(W, H)])}

    def match_frames(self, feats0, feats1):
        raise AssertionError("the original matcher is not reached with match_on_gpu")


class VO:
    def __init__(self, K, config):
        self.K, self.cfg = K, config
        self.frontend = Frontend(config)
        self.keyframe, self.map_points, self.next_pt_id, self.T_wc = None, {}, 0, np.eye(4)
        self.last_pos = np.zeros(3)

    def _create_keyframe(self, curr_feats, curr_ids, ref_indices, curr_indices):
        self.keyframe = {"feats": curr_feats, "ids": curr_ids, "T_wc": self.T_wc.copy()}

    def _reset_system(self):
        self.keyframe, self.map_points = None, {}

    def _prune_map(self):
        pass


@pytest.fixture
def classes():
    """Fresh stub classes with the hooks installed."""
    fe = type("FE", (Frontend,), {})

    def vo_init(self, K, config):
        VO.__init__(self, K, config)
        self.frontend = fe(config)

    vo = type("V", (VO,), {"__init__": vo_init})
    hooks.install(fe, vo)
    return fe, vo


class Track:
    """``klt.track`` stand-in: every point moves by FLOW per frame; ``lose[k]`` are keyframe-row
    positions (indices into the call's points) lost in frame k."""

    def __init__(self):
        self.calls, self.lose = [], {}

    def __call__(self, img0, img1, pts0, guess=None, win_radius=10, levels=4, max_iters=30, eps=0.01, min_eig=1e-4,
                 fb_thresh=None, max_err=None, tags=(0, 0), ctx=None):
        k0, k1 = int(img0[0, 0]), int(img1[0, 0])
        pts0 = np.asarray(pts0, np.float32)
        self.calls.append(dict(k0=k0, k1=k1, pts0=pts0.copy(), guess=None if guess is None else np.array(guess),
                               win_radius=win_radius, levels=levels, fb_thresh=fb_thresh, tags=tags))
        status = np.zeros(len(pts0), np.uint8)
        lose = self.lose.get(k1, ())
        status[:len(pts0) if lose == "all" else 0] = 3
        if lose != "all":
            status[list(lose)] = 4
        p1 = np.where(status[:, None] == 0, pts0 + FLOW * (k1 - k0), pts0)
        return p1, status, np.zeros(len(pts0), np.float32)


@pytest.fixture
def track(monkeypatch):
    t = Track()
    monkeypatch.setattr(klt, "track", t)
    return t


@pytest.fixture
def matched(monkeypatch):
    calls = []

    def knn(des0, des1, **kw):
        calls.append((np.asarray(des0).shape, np.asarray(des1).shape, kw))
        return np.zeros((0, 2), np.int64)

    monkeypatch.setattr(matcher, "match_knn2_ratio", knn)
    return calls


def start(classes, cfg=Cfg):
    _, vo_cls = classes
    vo = vo_cls(np.eye(3), cfg())
    f0 = vo.frontend.process_image(frame(0))
    vo.keyframe = {"feats": f0, "ids": np.full(f0["keypoints"].shape[1], -1), "T_wc": np.eye(4)}
    return vo, f0


def test_config_fields_are_off_by_default_and_the_switch_has_an_environment_name(monkeypatch):
    c = VOConfig()
    assert c.klt_tracking is False and get_config("kitti").klt_tracking is False
    assert (c.klt_win_radius, c.klt_levels, c.klt_fb_thresh, c.klt_min_tracks, c.klt_min_distance) == \
        (10, 4, 1.0, 50, 8.0)
    monkeypatch.setenv("VO_AMD_KLT", "1")
    assert get_config("kitti").klt_tracking is True


def test_first_frame_detects_and_later_frames_bring_their_pairs(classes, track, matched):
    vo, f0 = start(classes)
    assert vo.frontend.detected == [0] and not track.calls
    assert vo.frontend._vo_amd_klt.owner() is vo
    f1 = vo.frontend.process_image(frame(1))
    assert vo.frontend.detected == [0] and len(track.calls) == 1
    call = track.calls[0]
    assert (call["k0"], call["k1"], call["win_radius"], call["levels"], call["fb_thresh"]) == (0, 1, 10, 4, 1.0)
    assert call["tags"][0] != 0 and call["tags"][1] not in (0, call["tags"][0])
    np.testing.assert_array_equal(call["pts0"], f0["keypoints"][0])
    np.testing.assert_array_equal(call["guess"], f0["keypoints"][0])
    np.testing.assert_array_equal(f1["keypoints"][0], f0["keypoints"][0] + FLOW)
    np.testing.assert_array_equal(f1["descriptors"][0], f0["descriptors"][0])
    np.testing.assert_array_equal(f1["image_size"], f0["image_size"])
    pairs = vo.frontend.match_frames(vo.keyframe["feats"], f1)
    assert pairs.dtype == np.int64
    np.testing.assert_array_equal(pairs, np.stack([np.arange(150), np.arange(150)], 1))
    assert not matched
    # the keyframe's pyramid is a cache hit on every later frame: the same tag
    vo.frontend.process_image(frame(2))
    assert track.calls[1]["tags"][0] == call["tags"][0] and track.calls[1]["tags"][1] != call["tags"][1]
    # another pair of dicts is matched as without the route
    vo.frontend.match_frames(f1, f0)
    assert len(matched) == 1


def test_lost_points_never_return_and_the_guess_is_the_previous_position(classes, track):
    vo, f0 = start(classes)
    kp0 = f0["keypoints"][0]
    track.lose = {1: [3, 7], 2: [0]}
    f1 = vo.frontend.process_image(frame(1))
    alive1 = np.delete(np.arange(150), [3, 7])
    np.testing.assert_array_equal(vo.frontend.match_frames(f0, f1), np.stack([alive1, np.arange(148)], 1))
    f2 = vo.frontend.process_image(frame(2))
    c2 = track.calls[1]
    np.testing.assert_array_equal(c2["pts0"], kp0[alive1])          # from the keyframe, the lost ones left out
    np.testing.assert_array_equal(c2["guess"], kp0[alive1] + FLOW)  # where they were in frame 1
    alive2 = alive1[1:]
    np.testing.assert_array_equal(vo.frontend.match_frames(f0, f2), np.stack([alive2, np.arange(147)], 1))
    np.testing.assert_array_equal(f2["keypoints"][0], kp0[alive2] + 2 * FLOW)
    np.testing.assert_array_equal(f2["descriptors"][0], f0["descriptors"][0][alive2])
    f3 = vo.frontend.process_image(frame(3))
    assert len(track.calls[2]["pts0"]) == 147 and f3["keypoints"].shape == (1, 147, 2)


def test_fewer_survivors_than_min_tracks_detects_for_that_frame(classes, track, matched):
    vo, f0 = start(classes)
    track.lose = {1: list(range(135))}  # 15 survive < 20
    f1 = vo.frontend.process_image(frame(1))
    assert vo.frontend.detected == [0, 1]
    np.testing.assert_array_equal(f1["keypoints"][0], detections(1)[0])
    assert hooks._KLT_SRC not in f1 and f1[hooks._KLT_IMAGE][0, 0] == 1
    vo.frontend.match_frames(f0, f1)
    assert len(matched) == 1 and matched[0][0] == (1, 150, 16)
    # the lost stay lost: the next frame has too few to track and detects without a track call
    vo.frontend.process_image(frame(2))
    assert vo.frontend.detected == [0, 1, 2] and len(track.calls) == 1


def test_a_colour_frame_is_left_to_the_detector(classes, track):
    vo, f0 = start(classes)
    rgb = np.zeros((H, W, 3), np.uint8)
    rgb[0, 0] = 4
    f = vo.frontend.process_image(rgb)
    assert vo.frontend.detected == [0, 4] and not track.calls and hooks._KLT_IMAGE not in f


def test_new_keyframe_is_replenished_away_from_the_kept_keypoints(classes, track):
    vo, f0 = start(classes)
    track.lose = {1: list(range(0, 150, 3))}
    f1 = vo.frontend.process_image(frame(1))
    pairs = vo.frontend.match_frames(f0, f1)
    ids = np.full(100, -1)
    ids[:40] = np.arange(40)
    vo._create_keyframe(f1, ids, pairs[:, 0], pairs[:, 1])
    feats, kids = vo.keyframe["feats"], vo.keyframe["ids"]
    assert feats is not f1 and vo.frontend.detected == [0, 1]  # detected on the keyframe's own image
    kp, des = feats["keypoints"][0], feats["descriptors"][0]
    n = len(kp)
    assert 100 < n <= Cfg.sift_n_features and des.shape == (n, 16) and kids.shape == (n,)
    np.testing.assert_array_equal(kp[:100], f1["keypoints"][0])  # the rows it had keep their indices
    np.testing.assert_array_equal(des[:100], f1["descriptors"][0])
    np.testing.assert_array_equal(kids[:100], ids)
    assert (kids[100:] == -1).all()
    d = np.linalg.norm(kp[100:, None] - kp[None, :100], axis=2)
    assert d.min() >= Cfg.klt_min_distance
    det_kp, det_des = detections(1)
    far = np.linalg.norm(det_kp[:, None] - kp[None, :100], axis=2).min(1) >= Cfg.klt_min_distance
    assert far.sum() > Cfg.sift_n_features - 100  # more candidates than room: the cap binds
    assert n == Cfg.sift_n_features
    where = [int(np.flatnonzero((det_kp == p).all(1))[0]) for p in kp[100:]]
    assert far[where].all() and len(set(where)) == len(where)
    np.testing.assert_array_equal(des[100:], det_des[where])
    assert hooks._KLT_SRC not in feats and feats[hooks._KLT_IMAGE][0, 0] == 1
    assert vo._vo_amd_window.frames[-1].uv.shape == (100, 2)  # the window was fed before the replenishment
    # the next frame tracks all rows of the new keyframe, from its image
    track.lose = {}
    f2 = vo.frontend.process_image(frame(2))
    c = track.calls[-1]
    assert (c["k0"], c["k1"]) == (1, 2) and len(c["pts0"]) == n
    np.testing.assert_array_equal(vo.frontend.match_frames(feats, f2)[:, 0], np.arange(n))
    # a keyframe made from a detected frame is complete: nothing appended
    track.lose = {3: "all"}
    f3 = vo.frontend.process_image(frame(3))
    vo._create_keyframe(f3, np.full(150, -1), np.zeros(0, int), np.zeros(0, int))
    assert vo.keyframe["feats"] is f3 and len(vo.keyframe["ids"]) == 150


def test_far_from_is_the_exact_distance_rule():
    rng = np.random.default_rng(2)
    kept, cand = rng.uniform(-20, 300, (400, 2)), rng.uniform(-20, 300, (500, 2))
    cand[:5] = kept[:5] + [[7.9, 0], [0, 8.0], [5.7, 5.7], [-5.6, 5.6], [0, 0]]
    for d in (8.0, 3.0, 25.0):
        want = np.linalg.norm(cand[:, None] - kept[None], axis=2).min(1) >= d
        np.testing.assert_array_equal(hooks.far_from(kept, cand, d), want)
    assert hooks.far_from(kept[:0], cand, 8.0).all() and hooks.far_from(kept, cand[:0], 8.0).shape == (0,)


def test_reset_drops_the_tracker_state(classes, track):
    vo, f0 = start(classes)
    track.lose = {1: [1, 2]}
    vo.frontend.process_image(frame(1))
    st = vo.frontend._vo_amd_klt
    assert st.src is f0 and len(st.alive) == 148
    vo._reset_system()
    assert st.src is None and st.alive is None and st.last is None and vo.keyframe is None
    f2 = vo.frontend.process_image(frame(2))  # no keyframe: detects
    assert vo.frontend.detected == [0, 2] and hooks._KLT_SRC not in f2


class OffCfg:
    """A config of a drive without the route that raises on any ``klt_*`` access."""
    extractor_type = "sift"
    match_on_gpu = True
    sift_on_gpu = False
    ba_enabled = False

    def __getattr__(self, name):
        if name.startswith("klt_"):
            raise AssertionError(f"{name} read with the route off")
        raise AttributeError(name)


def test_route_off_touches_nothing(classes, track, matched):
    fe_cls, vo_cls = classes
    for raising in (False, True):
        vo = vo_cls(np.eye(3), type("C", (Cfg,), {"klt_tracking": False})())
        assert not hasattr(vo.frontend, "_vo_amd_klt")
        if raising:  # construction alone reads the switch; nothing on the frame path reads a klt_* setting
            vo.cfg = vo.frontend.conf = OffCfg()
        f0 = vo.frontend.process_image(frame(0))
        assert set(f0) == {"keypoints", "descriptors", "image_size"}
        vo.keyframe = {"feats": f0, "ids": np.full(150, -1), "T_wc": np.eye(4)}
        f1 = vo.frontend.process_image(frame(1))
        assert set(f1) == {"keypoints", "descriptors", "image_size"}
        before = len(matched)
        vo.frontend.match_frames(f0, f1)
        assert len(matched) == before + 1
        vo._create_keyframe(f1, np.full(150, -1), np.zeros(0, int), np.zeros(0, int))
        assert vo.keyframe["feats"] is f1 and len(vo.keyframe["ids"]) == 150
        vo._reset_system()
        assert not track.calls and not hasattr(vo.frontend, "_vo_amd_klt")
