"""``cfg.map_epipolar_search`` through the real ``matcher.match_segment`` and the real
``triangulate.triangulate_points`` on the GPU: the host test's drive gives the same
``keyframe["ids"]`` and the same window as under its stubs (the CPU restatement and the
triangulation oracle), and map points within the triangulation's documented parity."""

import numpy as np
import pytest

from oracle import triangulate_ref
from tests import segment_ref
from tests.epipolar_scene import LOSE_AT, EpiCfg, run
from visualodometry_amd import matcher, triangulate

pytestmark = pytest.mark.gpu


def _stubbed(monkeypatch):
    with monkeypatch.context() as m:
        m.setattr(matcher, "match_segment",
                  lambda des0, seg, radius, des1, kp1, ratio=0.75, max_dist=0.0, unique=True, image_size=None,
                  return_dist=False, ctx=None: segment_ref.segmented(des0, seg, radius, des1, kp1, ratio, max_dist,
                                                                     unique).pairs)
        m.setattr(triangulate, "triangulate_points",
                  lambda T1, T2, p1, p2, K, cfg, ctx=None: triangulate_ref.triangulate_points(
                      T1, T2, p1, p2, K, cfg.min_depth, cfg.max_reproj_err))
        return run(EpiCfg(map_epipolar_search=True))


def test_the_real_calls_give_the_stubbed_run(ctx, monkeypatch):
    ref = _stubbed(monkeypatch)
    got = run(EpiCfg(map_epipolar_search=True))
    made = [c for c in got.calls if len(c["ids"])]
    assert made and made[0]["k"] == LOSE_AT and len(made[0]["ids"]) >= len(got.lost) // 2
    assert [len(c["ids"]) for c in got.calls] == [len(c["ids"]) for c in ref.calls]
    np.testing.assert_array_equal(got.vo.keyframe["ids"], ref.vo.keyframe["ids"])
    assert got.vo.next_pt_id == ref.vo.next_pt_id
    a, b = got.vo._vo_amd_window.frames, ref.vo._vo_amd_window.frames
    assert len(a) == len(b) == 6
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.ids, y.ids)
        np.testing.assert_array_equal(x.uv, y.uv)
        np.testing.assert_array_equal(x.T_wc, y.T_wc)
        assert len(x.extra_ids) == len(y.extra_ids)
        for p, q in zip(x.extra_ids + x.extra_uv, y.extra_ids + y.extra_uv):
            np.testing.assert_array_equal(p, q)
    assert got.vo.map_points.keys() == ref.vo.map_points.keys()
    for c in made:
        for i in c["ids"]:
            P, Q = got.vo.map_points[int(i)], ref.vo.map_points[int(i)]
            assert P.dtype == np.float32
            # the triangulation's parity with its oracle for well-conditioned points (test_gpu_triangulate.py)
            np.testing.assert_allclose(P, Q, rtol=1e-5, atol=1e-5)
    # the landmarks made at LOSE_AT are the lost ones, each on a keypoint of its own landmark
    first = made[0]
    cur_lm = got.feats[LOSE_AT]["lm"]
    slots = [list(first["ids_after"]).index(i) for i in first["ids"]]
    assert set(cur_lm[slots].tolist()) <= set(got.lost)
