"""``cfg.map_epipolar_search`` in the wrapped ``_create_keyframe`` on the host, under stubs:
``matcher.match_segment`` is the CPU restatement of ``tests/segment_ref.py`` behind the real
signature and ``triangulate.triangulate_points`` is ``oracle/triangulate_ref.py``.  Off by default
and inert when off; when on, only unlabelled keypoints that took no part in the keyframe's own
match are offered, every surviving pair becomes a landmark with both of its rays in the window,
the pairs join keypoints of the same true landmark, the landmarks the original made keep their
rays, and reset and prune behave."""

import numpy as np
import pytest

from oracle import triangulate_ref
from tests import segment_ref
from tests.epipolar_scene import LOSE_AT, EpiCfg, run
from tests.vo_scene import Cfg, FakeVO
from visualodometry_amd import matcher, triangulate
from visualodometry_amd.dropin import hooks
from visualodometry_amd.dropin.config.config import VOConfig, get_config
from visualodometry_amd.mapstore import LandmarkDescriptors


class MatchStub:
    """``matcher.match_segment`` on the CPU, recording every call."""

    def __init__(self):
        self.calls = []

    def __call__(self, des0, seg, radius, des1, kp1, ratio=0.75, max_dist=0.0, unique=True, image_size=None,
                 return_dist=False, ctx=None):
        pairs = segment_ref.segmented(des0, seg, radius, des1, kp1, ratio, max_dist, unique).pairs
        self.calls.append(dict(des0=np.array(des0), seg=np.array(seg), radius=radius, des1=np.array(des1),
                               kp1=np.array(kp1), ratio=ratio, max_dist=max_dist, unique=unique,
                               image_size=image_size, pairs=pairs))
        return pairs


class TriStub:
    """``triangulate.triangulate_points`` as the oracle, recording every call."""

    def __init__(self):
        self.calls = []

    def __call__(self, T_cw1, T_cw2, pts1, pts2, K, config, ctx=None):
        pts, mask = triangulate_ref.triangulate_points(T_cw1, T_cw2, pts1, pts2, K, config.min_depth,
                                                       config.max_reproj_err)
        self.calls.append(dict(pts1=np.array(pts1), pts2=np.array(pts2), mask=mask, pts=pts))
        return pts, mask


@pytest.fixture
def stubs(monkeypatch):
    m, t = MatchStub(), TriStub()
    monkeypatch.setattr(matcher, "match_segment", m)
    monkeypatch.setattr(triangulate, "triangulate_points", t)
    return m, t


def _same_window(a, b):
    assert len(a._vo_amd_window.frames) == len(b._vo_amd_window.frames) == 6
    for x, y in zip(a._vo_amd_window.frames, b._vo_amd_window.frames):
        np.testing.assert_array_equal(x.ids, y.ids)
        np.testing.assert_array_equal(x.uv, y.uv)
        np.testing.assert_array_equal(x.T_wc, y.T_wc)
        assert len(x.extra_ids) == len(y.extra_ids)
        for p, q in zip(x.extra_ids + x.extra_uv, y.extra_ids + y.extra_uv):
            np.testing.assert_array_equal(p, q)


def test_switch_is_off_by_default_and_inert_when_off(stubs, monkeypatch):
    assert VOConfig().map_epipolar_search is False and get_config("kitti").map_epipolar_search is False
    cfg = VOConfig()
    assert (cfg.map_epipolar_radius, cfg.map_epipolar_ratio, cfg.map_epipolar_max_dist, cfg.map_epipolar_min_depth,
            cfg.map_epipolar_max_depth, cfg.map_epipolar_min_length) == (2.0, 0.8, None, 1.0, 0.0, 8.0)
    monkeypatch.setenv("VO_AMD_EPIPOLAR", "1")
    assert get_config("kitti").map_epipolar_search is True and get_config("kitti").map_reobserve is False
    monkeypatch.setenv("VO_AMD_EPIPOLAR", "0")
    assert get_config("kitti").map_epipolar_search is False
    monkeypatch.delenv("VO_AMD_EPIPOLAR")
    bare = run(Cfg(ba_enabled=False))  # a config from before the switch existed
    off = run(EpiCfg(map_epipolar_search=False))
    assert not stubs[0].calls and not stubs[1].calls and not bare.calls and not off.calls
    assert bare.vo.prunes == off.vo.prunes == 0  # (the double's original does not prune)
    assert bare.vo.map_points.keys() == off.vo.map_points.keys() and bare.vo.next_pt_id == off.vo.next_pt_id
    assert all(np.array_equal(bare.vo.map_points[i], off.vo.map_points[i]) for i in bare.vo.map_points)
    np.testing.assert_array_equal(bare.vo.keyframe["ids"], off.vo.keyframe["ids"])
    _same_window(bare.vo, off.vo)
    for r in (bare, off):
        assert not hasattr(r.vo, "_vo_amd_lm_desc")
    # the lost landmarks are unlabelled in keyframe LOSE_AT without the search
    fr = off.vo._vo_amd_window.frames[LOSE_AT]
    slots = [s for s, lm in enumerate(off.feats[LOSE_AT]["lm"]) if lm in off.lost]
    assert len(slots) == len(off.lost) and (fr.ids[slots] == -1).all()


def test_on_offers_the_right_sets_and_makes_landmarks_with_two_rays(stubs):
    match, tri = stubs
    r = run(EpiCfg(map_epipolar_search=True))
    vo = r.vo
    assert len(r.calls) == 5  # every keyframe with a predecessor
    made = [c for c in r.calls if len(c["ids"])]
    assert made and made[0]["k"] == LOSE_AT and len(match.calls) >= len(made) and len(tri.calls) == \
        sum(1 for m in match.calls if len(m["pairs"]))
    truth = dict(vo.truth)  # id -> true landmark; the double fills it for the ids its original made
    mi = ti = 0
    for c in r.calls:
        k, prev, cur = c["k"], c["prev"], r.feats[c["k"]]
        assert prev["feats"] is r.feats[k - 1]
        # the sets at the moment of the call
        q = np.flatnonzero((c["prev_ids"] == -1) & ~np.isin(np.arange(len(c["prev_ids"])), c["ref"]))
        free = np.flatnonzero((c["ids_before"] == -1) & ~np.isin(np.arange(len(c["ids_before"])), c["cur"]))
        changed = np.flatnonzero(c["ids_after"] != c["ids_before"])
        if q.size == 0 or free.size == 0:
            assert len(c["ids"]) == 0 and changed.size == 0
            continue
        kp0, kp1 = prev["feats"]["keypoints"][0], cur["keypoints"][0]
        seg, valid = matcher.epipolar_segments(kp0[q], np.linalg.inv(prev["T_wc"]), np.linalg.inv(r.scene.T_wc[k]),
                                               vo.K, (1241, 376), 1.0, np.inf, 8.0)
        if not valid.any():
            assert len(c["ids"]) == 0 and changed.size == 0
            continue
        q = q[valid]
        m = match.calls[mi]
        mi += 1
        assert m["unique"] is True and m["image_size"] == (1241, 376)
        assert (m["radius"], m["ratio"], m["max_dist"]) == (2.0, 0.8, 120.0)
        np.testing.assert_array_equal(m["des0"], prev["feats"]["descriptors"][0][q])
        np.testing.assert_array_equal(m["seg"], seg[valid])
        np.testing.assert_array_equal(m["des1"], cur["descriptors"][0][free])
        np.testing.assert_array_equal(m["kp1"], kp1[free])
        pairs = m["pairs"]
        if len(pairs) == 0:
            assert len(c["ids"]) == 0 and changed.size == 0
            continue
        qi, ci = q[pairs[:, 0]], free[pairs[:, 1]]
        # the pairs join keypoints of the same true landmark
        np.testing.assert_array_equal(prev["feats"]["lm"][qi], cur["lm"][ci])
        t = tri.calls[ti]
        ti += 1
        np.testing.assert_array_equal(t["pts1"], kp0[qi])
        np.testing.assert_array_equal(t["pts2"], kp1[ci])
        qi, ci = qi[t["mask"]], ci[t["mask"]]
        # every surviving pair: a fresh id, ascending with the query, on its keypoint and in the map
        ids = c["ids"]
        np.testing.assert_array_equal(ids, c["next_before"] + np.arange(len(qi)))
        np.testing.assert_array_equal(np.sort(changed), np.sort(ci))
        np.testing.assert_array_equal(c["ids_after"][ci], ids)
        np.testing.assert_array_equal(c["uv"], kp0[qi])
        assert c["uv"].dtype == np.float32 and ids.dtype == np.int64
        for i, X in zip(ids, t["pts"]):
            assert vo.map_points[int(i)].dtype == np.float32
            np.testing.assert_array_equal(vo.map_points[int(i)], X.astype(np.float32))
            truth[int(i)] = int(cur["lm"][list(c["ids_after"]).index(i)])
    assert mi == len(match.calls) and ti == len(tri.calls)
    assert vo.prunes == len(made)  # _prune_map once more per keyframe that made landmarks
    # keyframe LOSE_AT: most of the lost landmarks became landmarks there after all
    first = made[0]
    got = {truth[int(i)] for i in first["ids"]}
    assert got <= set(r.lost) and len(got) >= len(r.lost) // 2
    assert vo.next_pt_id == len(vo.map_points) == len(truth)
    # both rays of every landmark ever made are in the window: each id sits on a keypoint of its true
    # landmark in the keyframe that made it, and its other ray is the previous keyframe's keypoint of it
    frames = vo._vo_amd_window.frames
    seen_extra = set()
    for k, fr in enumerate(frames):
        lm = r.feats[k]["lm"]
        for s, i in enumerate(fr.ids):
            assert i < 0 or truth[int(i)] == lm[s]
        live = fr.ids[fr.ids >= 0]
        assert len(np.unique(live)) == len(live)
        for ids, uv in zip(fr.extra_ids, fr.extra_uv):
            for i, p in zip(ids, uv):
                s = list(lm).index(truth[int(i)])
                np.testing.assert_array_equal(p, r.feats[k]["keypoints"][0][s])
                assert fr.ids[s] != i and int(i) in frames[k + 1].ids.tolist()
                seen_extra.add(int(i))
    assert {int(i) for c in made for i in c["ids"]} <= seen_extra
    kf, _, pid = vo._vo_amd_window.observations(vo.map_points)
    for c in made:
        for i in c["ids"]:
            assert sorted(kf[pid == i].tolist())[:2] == [c["k"] - 1, c["k"]]


def test_the_originals_landmarks_keep_their_rays(stubs):
    """Up to the keyframe where the search first makes a landmark the two runs see the same input, so
    there the ids the original made and their previous-keyframe rays are those of the run without
    the switch, and the search's own follow them."""
    off = run(EpiCfg(map_epipolar_search=False))
    on = run(EpiCfg(map_epipolar_search=True))
    a, b = off.vo._vo_amd_window.frames[LOSE_AT - 1], on.vo._vo_amd_window.frames[LOSE_AT - 1]
    first = [c for c in on.calls if c["k"] == LOSE_AT][0]
    assert len(a.extra_ids) == len(b.extra_ids) == 1 and len(first["ids"]) > 0
    n = len(a.extra_ids[0])
    assert n > 50 and len(b.extra_ids[0]) == n + len(first["ids"])
    np.testing.assert_array_equal(b.extra_ids[0][:n], a.extra_ids[0])
    np.testing.assert_array_equal(b.extra_uv[0][:n], a.extra_uv[0])
    np.testing.assert_array_equal(b.extra_ids[0][n:], first["ids"])
    np.testing.assert_array_equal(b.extra_uv[0][n:], first["uv"])
    # the original's ids sit where they sat; the search only filled keypoints that were free
    ka, kb = off.vo._vo_amd_window.frames[LOSE_AT].ids, on.vo._vo_amd_window.frames[LOSE_AT].ids
    np.testing.assert_array_equal(kb[ka >= 0], ka[ka >= 0])
    assert ((ka == -1) & (kb >= 0)).sum() == len(first["ids"]) and (first["ids"] >= ka.max() + 1).all()


def test_with_reobserve_the_new_ids_have_descriptors(stubs, monkeypatch):
    from tests import gated_ref

    monkeypatch.setattr(matcher, "match_gated",
                        lambda des0, pred, radius, des1, kp1, ratio=0.75, max_dist=0.0, unique=True, image_size=None,
                        return_dist=False, ctx=None: gated_ref.gated(des0, pred, radius, des1, kp1, ratio, max_dist,
                                                                     unique).pairs)
    r = run(EpiCfg(map_epipolar_search=True, map_reobserve=True))
    store = r.vo._vo_amd_lm_desc
    assert isinstance(store, LandmarkDescriptors)
    made = [c for c in r.calls if len(c["ids"])]
    assert made
    for c in made:
        assert store.contains(c["ids"]).all()
        des = r.feats[c["k"]]["descriptors"][0]
        slots = [list(c["ids_after"]).index(i) for i in c["ids"]]
        np.testing.assert_array_equal(store.gather(c["ids"]), des[slots])
    assert len(store) == r.vo.next_pt_id  # every landmark, the original's and the search's
    # without map_reobserve no store appears
    assert not hasattr(run(EpiCfg(map_epipolar_search=True)).vo, "_vo_amd_lm_desc")


def test_reset_and_prune_behave(stubs):
    r = run(EpiCfg(map_epipolar_search=True, map_reobserve=False))
    vo = r.vo
    assert vo.prunes >= 1 and len(vo._vo_amd_window.frames) == 6
    hooks._wrap_reset(FakeVO._reset_system)(vo)
    assert len(vo._vo_amd_window.frames) == 0 and vo.keyframe is None and not vo.map_points
    # a keyframe without a predecessor: nothing to search from, no call
    n = len(stubs[0].calls)
    cur = r.feats[2]
    ids = np.full(cur["lm"].size, -1)
    hooks._wrap_create_keyframe(type(vo)._create_keyframe)(vo, cur, ids, np.zeros(0, int), np.zeros(0, int))
    assert len(stubs[0].calls) == n and len(vo._vo_amd_window.frames) == 1 and (ids == -1).all()
