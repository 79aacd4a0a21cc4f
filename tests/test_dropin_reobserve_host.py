"""``cfg.map_reobserve`` in the wrapped ``_create_keyframe`` on the host, under a stub ``match_gated``
(the CPU restatement of ``tests/gated_ref.py`` behind the real signature): off by default and inert when
off; when on, new landmarks get descriptors, only live ids absent from ``curr_ids`` are offered, only
unlabelled keypoints are candidates, matched ids land in ``keyframe["ids"]`` and in the window's
observations, and reset and prune clear the descriptor store."""

import numpy as np
import pytest

from tests import gated_ref
from tests.reobserve_scene import DescScene, ReCfg, drive, losable
from tests.vo_scene import Cfg, FakeVO
from visualodometry_amd import matcher
from visualodometry_amd.dropin import hooks
from visualodometry_amd.dropin.config.config import VOConfig, get_config
from visualodometry_amd.mapstore import MAX_POINTS, LandmarkDescriptors, MapStore

LOSE_AT = 3


def _hooked():
    return hooks._wrap_create_keyframe(FakeVO._create_keyframe)


class Stub:
    """``matcher.match_gated`` on the CPU, recording every call."""

    def __init__(self):
        self.calls = []

    def __call__(self, des0, pred, radius, des1, kp1, ratio=0.75, max_dist=0.0, unique=True, image_size=None,
                 return_dist=False, ctx=None):
        self.calls.append(dict(des0=np.array(des0), pred=np.array(pred), radius=radius, des1=np.array(des1),
                               kp1=np.array(kp1), ratio=ratio, max_dist=max_dist, unique=unique,
                               image_size=image_size))
        return gated_ref.gated(des0, pred, radius, des1, kp1, ratio, max_dist, unique).pairs


@pytest.fixture
def stub(monkeypatch):
    s = Stub()
    monkeypatch.setattr(matcher, "match_gated", s)
    return s


def _run(cfg, lose=True, on_keyframe=None):
    scene = DescScene()
    vo = FakeVO(cfg, tri_noise=0.01)
    lost = losable(scene, LOSE_AT, 8)
    assert len(lost) == 8
    drive(vo, scene, _hooked(), {LOSE_AT: lost} if lose else None, on_keyframe)
    return vo, scene, lost


def test_switch_is_off_by_default_and_inert_when_off(stub, monkeypatch):
    assert VOConfig().map_reobserve is False and get_config("kitti").map_reobserve is False
    monkeypatch.setenv("VO_AMD_REOBSERVE", "1")
    assert get_config("kitti").map_reobserve is True
    monkeypatch.delenv("VO_AMD_REOBSERVE")
    bare, _, _ = _run(Cfg(ba_enabled=False))  # a config from before the switch existed
    off, _, _ = _run(ReCfg(map_reobserve=False))
    assert not stub.calls
    for vo in (bare, off):
        assert not hasattr(vo, "_vo_amd_lm_desc")
    assert bare.map_points.keys() == off.map_points.keys()
    assert all(np.array_equal(bare.map_points[i], off.map_points[i]) for i in bare.map_points)
    np.testing.assert_array_equal(bare.keyframe["ids"], off.keyframe["ids"])
    assert len(bare._vo_amd_window.frames) == len(off._vo_amd_window.frames) == 6
    for a, b in zip(bare._vo_amd_window.frames, off._vo_amd_window.frames):
        np.testing.assert_array_equal(a.ids, b.ids)
        np.testing.assert_array_equal(a.uv, b.uv)
        np.testing.assert_array_equal(a.T_wc, b.T_wc)
        assert len(a.extra_ids) == len(b.extra_ids)
        for x, y in zip(a.extra_ids + a.extra_uv, b.extra_ids + b.extra_uv):
            np.testing.assert_array_equal(x, y)


def test_a_lost_landmark_stays_unlabelled_with_the_switch_off(stub):
    vo, scene, lost = _run(ReCfg(map_reobserve=False))
    fr, lm = vo._vo_amd_window.frames[LOSE_AT], vo._lm_log[LOSE_AT]
    slots = [slot for slot in range(len(lm)) if lm[slot] in lost]
    assert len(slots) == len(lost) and (fr.ids[slots] == -1).all()
    assert len(first_ids(vo, lost)) >= 4  # although most of them were in the map by then


def first_ids(vo, lost, below=10 ** 9):
    """The first id each lost landmark ever got, among the ids ``< below``."""
    out = {}
    for i in sorted(vo.truth):
        out.setdefault(vo.truth[i], i)
    return {out[lm] for lm in lost if lm in out and out[lm] < below}


@pytest.fixture(autouse=True)
def _log_landmarks(monkeypatch):
    """Keep each keyframe's true landmark per keypoint on the VO double (test bookkeeping)."""
    orig = FakeVO._create_keyframe

    def logged(self, curr_feats, curr_ids, ref_indices, curr_indices):
        if not hasattr(self, "_lm_log"):
            self._lm_log = {0: self.keyframe["feats"]["lm"]}
        self._lm_log[len(self._lm_log)] = curr_feats["lm"]
        return orig(self, curr_feats, curr_ids, ref_indices, curr_indices)

    monkeypatch.setattr(FakeVO, "_create_keyframe", logged)


def test_on_offers_the_right_sets_and_writes_the_ids(stub):
    seen = {}

    def before(k, cur, curr_ids):
        n_calls = len(stub.calls)

        def after():
            vo = seen["vo"]
            store = vo._vo_amd_lm_desc
            assert isinstance(store, LandmarkDescriptors)
            ids_now = vo.keyframe["ids"]
            assert ids_now is curr_ids  # the array the keyframe keeps: later PnP sees the ids too
            if len(stub.calls) == n_calls:
                return
            call = stub.calls[-1]
            assert call["unique"] is True and call["image_size"] == (1241, 376)
            assert (call["radius"], call["ratio"], call["max_dist"]) == (10.0, 0.8, 120.0)
            # reconstruct the moment of the call: ids written by the re-observation are the old ones
            # (< the first id this keyframe created) sitting on keypoints the association left free
            pairs = gated_ref.gated(call["des0"], call["pred"], call["radius"], call["des1"], call["kp1"],
                                    call["ratio"], call["max_dist"], True).pairs
            des = cur["descriptors"][0]
            kp = cur["keypoints"][0]
            # candidates: exactly the keypoints without an id at that moment, in order
            free = np.flatnonzero(np.isin(np.arange(len(ids_now)), seen["free"][k]))
            np.testing.assert_array_equal(call["des1"], des[free])
            np.testing.assert_array_equal(call["kp1"], kp[free])
            # offered: live map ids absent from curr_ids with a stored descriptor, projecting into the image
            offered = seen["offered"][k]
            np.testing.assert_array_equal(call["des0"], store.gather(offered))
            assert len(call["pred"]) == len(offered)
            # matched ids landed on the free keypoints they were matched to
            np.testing.assert_array_equal(ids_now[free[pairs[:, 1]]], offered[pairs[:, 0]])
            seen.setdefault("matched", {})[k] = offered[pairs[:, 0]]

        return after

    # the sets at the moment of the call are captured by wrapping reobserve_map itself
    real = hooks.reobserve_map

    def spy(vo, curr_feats, curr_ids, first_new):
        k = len(vo._lm_log) - 1
        seen["vo"] = vo
        seen.setdefault("free", {})[k] = np.flatnonzero(curr_ids == -1)
        live = np.array(sorted(vo.map_points), np.int64)
        absent = live[~np.isin(live, curr_ids)]
        # new landmarks get descriptors first, so every live id has one here
        T_cw = np.linalg.inv(vo.T_wc)
        xyz = np.array([vo.map_points[int(i)] for i in absent], np.float64).reshape(-1, 3)
        _, valid = matcher.project_points(xyz, T_cw, vo.K, (1241, 376), vo.cfg.min_depth)
        seen.setdefault("offered", {})[k] = absent[valid]
        seen.setdefault("new", {})[k] = (curr_ids[curr_ids >= first_new].copy(),
                                         curr_feats["descriptors"][0][curr_ids >= first_new].copy())
        return real(vo, curr_feats, curr_ids, first_new)

    hooks.reobserve_map = spy
    try:
        vo, scene, lost = _run(ReCfg(map_reobserve=True), on_keyframe=before)
    finally:
        hooks.reobserve_map = real
    store = vo._vo_amd_lm_desc
    # every landmark ever created has the descriptor of the keypoint it was created from
    assert len(seen["new"]) == 5 and sum(len(i) for i, _ in seen["new"].values()) == vo.next_pt_id > 100
    for ids, des in seen["new"].values():
        assert store.contains(ids).all()
        np.testing.assert_array_equal(store.gather(ids), des)
    assert len(store) == vo.next_pt_id and store.dim == 32
    # the landmarks whose match into keyframe LOSE_AT was lost got their ids back there
    fr = vo._vo_amd_window.frames[LOSE_AT]
    lm = vo._lm_log[LOSE_AT]
    held = first_ids(vo, lost, below=int(seen["new"][LOSE_AT][0].min()))  # in the map before that keyframe
    assert len(held) >= 4
    back = [int(i) for slot, i in enumerate(fr.ids) if lm[slot] in lost and i >= 0]
    assert set(back) == held and all(vo.truth[i] == lm[list(fr.ids).index(i)] for i in back)
    assert held <= set(seen["matched"][LOSE_AT].tolist())
    # ... and the window's observations have them in that keyframe
    kf, uv, pid = vo._vo_amd_window.observations(vo.map_points)
    for i in held:
        assert LOSE_AT in kf[pid == i].tolist()
    # no id twice in a keyframe
    for f in vo._vo_amd_window.frames:
        live = f.ids[f.ids >= 0]
        assert len(np.unique(live)) == len(live)


def test_reset_and_prune_clear_the_store(stub):
    vo, _, _ = _run(ReCfg(map_reobserve=True))
    store = vo._vo_amd_lm_desc
    n = len(store)
    assert n == vo.next_pt_id > 0
    vo.next_pt_id = MAX_POINTS + 50  # ids below 50 are due
    pruned = []
    hooks._wrap_prune(lambda self: pruned.append(1))(vo)  # a dict map: the original prunes the map
    assert pruned == [1] and len(store) == n - 50 and not store.contains(np.arange(50)).any()
    vo.map_points = MapStore()
    hooks._wrap_prune(lambda self: pruned.append(2))(vo)
    assert pruned == [1]
    hooks._wrap_reset(FakeVO._reset_system)(vo)
    assert len(store) == 0 and vo._vo_amd_lm_desc is store


def test_landmark_descriptors_store():
    s = LandmarkDescriptors(capacity=4)
    assert s.slots == 8 and len(s) == 0 and not s.contains([0, 3]).any()
    s.put([], np.zeros((0, 5)))
    assert s.dim is None
    d = np.arange(15, dtype=np.float32).reshape(3, 5)
    s.put([1, 2, 9], d)  # 1 and 9 share slot 1: the newer id holds it
    assert s.dim == 5 and s.contains([1, 2, 9, -1, 17]).tolist() == [False, True, True, False, False]
    np.testing.assert_array_equal(s.gather([9, 2]), d[[2, 1]])
    with pytest.raises(KeyError):
        s.gather([1])
    with pytest.raises(ValueError):
        s.put([3], np.zeros((1, 4)))
    assert s.prune_below(9) == 1 and s.contains([2, 9]).tolist() == [False, True]
    s.clear()
    assert len(s) == 0
