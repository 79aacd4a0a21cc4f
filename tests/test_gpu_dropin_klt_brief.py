"""``cfg.klt_corner_describe`` end to end on the MI355X: the real frontend hooks (GPU SIFT,
``klt.track``, ``corners.good_features``, ``brief.describe``, both matchers) over a short drive cut
from the scene of tests/klt_dropin_scene.py with its stub owner.  Frames 1 and 2 are tracked, frame
2 becomes a keyframe replenished with described corners, and frame 3 is the scene turned upside down
(a half turn about the optical axis, plus a small shift): nothing can be tracked into it, so it is
the one frame that falls back to detection.  With the switch on its corner rows find the keyframe's
again, each within 2 px of the planted motion; with the switch off no corner row is ever matched."""

import numpy as np
import pytest

from tests import klt_dropin_scene as D
from tests import klt_scene as S
from visualodometry_amd import brief, corners

pytestmark = pytest.mark.gpu

SHIFTS = [(0, 0), (2, 1), (5, 2), (8, 3)]
BOUND_PX = 2.0
ROWS = 800


def frames():
    base = S.base_image(D.H, D.W, 8)
    f = [S.crop(base, D.H, D.W, s) for s in SHIFTS]
    f[3] = np.ascontiguousarray(f[3][::-1, ::-1])  # the half turn
    return f


def planted(p):
    """Where a point of frame 2 is in frame 3."""
    q = np.asarray(p, np.float64) + (SHIFTS[3][0] - SHIFTS[2][0], SHIFTS[3][1] - SHIFTS[2][1])
    return np.stack([D.W - 1 - q[:, 0], D.H - 1 - q[:, 1]], 1)


def drive(describe: bool, monkeypatch):
    from visualodometry_amd.dropin import hooks

    calls = {"corners": 0, "brief": 0}
    real_corners, real_brief = corners.good_features, brief.describe

    def counted_corners(*a, **kw):
        calls["corners"] += 1
        return real_corners(*a, **kw)

    def counted_brief(*a, **kw):
        calls["brief"] += 1
        return real_brief(*a, **kw)

    monkeypatch.setattr(corners, "good_features", counted_corners)
    monkeypatch.setattr(brief, "describe", counted_brief)
    cfg = D.config(None)
    # SIFT finds about 520 keypoints a frame at this threshold, so 800 rows leave room for corners; about 450 of
    # them are tracked into frames 1 and 2 and about 50 into the frame turned upside down (measured on the MI355X)
    cfg.sift_contrast_threshold, cfg.sift_n_features, cfg.klt_min_tracks = 0.04, ROWS, 200
    cfg.klt_corner_replenish, cfg.klt_corner_quality, cfg.klt_corner_block = True, 0.01, 3
    if describe:
        # The planted motion copies pixels exactly and a half turn leaves a descriptor unchanged, so a true corner pair
        # away from the border has distance 0: the limit is the smallest there is (0 would switch it off).  The blobs
        # of this scene look alike: with the default limit of 64 three of 127 corner pairs were false ones at distances
        # 43..49.
        cfg.klt_corner_describe, cfg.klt_brief_ratio, cfg.klt_brief_max_dist = True, 0.8, 1
    _, Owner = D.classes()
    vo = Owner(np.eye(3), cfg)
    fe = vo.frontend
    assert fe._vo_amd_klt.describe is describe
    fr = frames()
    f0 = fe.process_image(fr[0])
    vo.keyframe = {"feats": f0, "ids": np.full(len(hooks._keypoints(f0)), -1), "T_wc": np.eye(4)}
    fell_back = []
    for k in (1, 2):
        fk = fe.process_image(fr[k])
        fell_back.append(hooks._KLT_SRC not in fk)
        pairs = fe.match_frames(f0, fk)
    vo._create_keyframe(fk, np.full(len(pairs), -1), pairs[:, 0], pairs[:, 1])
    kf = vo.keyframe["feats"]
    f3 = fe.process_image(fr[3])
    fell_back.append(hooks._KLT_SRC not in f3)
    assert fell_back == [False, False, True]  # exactly one frame falls back to detection
    return hooks, kf, f3, fe.match_frames(kf, f3), len(pairs), calls


def test_switch_on_finds_the_keyframes_corners_again_in_the_frame_that_fell_back(ctx, monkeypatch):
    hooks, kf, f3, pairs, n_kept, calls = drive(True, monkeypatch)
    kp, has, rows = hooks._keypoints(kf), kf[hooks._KLT_HAS_DESC], kf[hooks._KLT_BRIEF]
    assert rows.shape == (len(kp), 8) and rows.dtype == np.uint32 and not rows[has].any() and rows[~has].any(1).all()
    assert has[:n_kept].all() and not has[n_kept:].any() and len(kp) > n_kept
    np.testing.assert_array_equal(rows[~has], brief.describe(kf[hooks._KLT_IMAGE], kp[~has], ctx=ctx)[0])
    kp3, has3, rows3 = hooks._keypoints(f3), f3[hooks._KLT_HAS_DESC], f3[hooks._KLT_BRIEF]
    assert len(kp3) == len(has3) == len(rows3) <= ROWS and has3.any() and not has3.all()
    assert tuple(f3["descriptors"].shape) == (1, len(kp3), 128) and not hooks._np(f3["descriptors"])[0][~has3].any()
    assert calls == {"corners": 2, "brief": 3}  # keyframe and fallback frame (and the check above)
    assert pairs.dtype == np.int64 and pairs.shape[1] == 2
    corner = ~has[pairs[:, 0]]
    assert corner.sum() >= 1
    assert (~has3[pairs[corner, 1]]).all() and has3[pairs[~corner, 1]].all()  # corners pair with corners only
    dev = np.abs(kp3[pairs[corner, 1]].astype(np.float64) - planted(kp[pairs[corner, 0]])).max(1)
    print(f"{corner.sum()} corner pairs of {(~has).sum()} keyframe and {(~has3).sum()} frame corners, "
          f"{(~corner).sum()} descriptor pairs; deviation max {dev.max():.3f} px")
    assert dev.max() <= BOUND_PX
    assert len(set(pairs[corner, 0].tolist())) == corner.sum() == len(set(pairs[corner, 1].tolist()))
    assert (np.diff(pairs[:, 0]) >= 0).all()


def test_switch_off_never_matches_a_corner_row(ctx, monkeypatch):
    hooks, kf, f3, pairs, n_kept, calls = drive(False, monkeypatch)
    has = kf[hooks._KLT_HAS_DESC]
    assert hooks._KLT_BRIEF not in kf and hooks._KLT_BRIEF not in f3 and hooks._KLT_HAS_DESC not in f3
    assert calls == {"corners": 1, "brief": 0}
    assert not has[n_kept:].any() and len(has) > n_kept
    assert has[pairs[:, 0]].all()  # no corner row appears
