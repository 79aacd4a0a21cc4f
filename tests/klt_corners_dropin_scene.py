"""The ``cfg.klt_corner_replenish`` route end to end for the GPU tests: the real frontend hooks (GPU
SIFT, ``klt.track``, ``corners.good_features``, the descriptor matcher) over the crop sequence of
tests/klt_dropin_scene.py with a stub owner holding ``keyframe``.  ``run(device)`` is shared by the
in-process test (numpy feature dicts) and the torch script (CUDA tensors); it returns the figures it
checked."""

from __future__ import annotations

import numpy as np

from tests import corners_ref as R
from tests import klt_dropin_scene as D
from tests import klt_scene as S


def run(device=None) -> dict:
    from visualodometry_amd import matcher
    from visualodometry_amd.dropin import hooks

    def on_device(feats):
        for key in ("keypoints", "descriptors"):
            v = feats[key]
            if device is None:
                assert isinstance(v, np.ndarray), key
            else:
                assert hasattr(v, "detach") and v.device.type == device.type, (key, getattr(v, "device", None))

    cfg = D.config(device)
    cfg.klt_corner_replenish, cfg.klt_corner_quality, cfg.klt_corner_block = True, 0.01, 3
    base = S.base_image(D.H, D.W, 8)
    frames = [S.crop(base, D.H, D.W, s) for s in D.SHIFTS]
    _, Owner = D.classes()
    vo = Owner(np.eye(3), cfg)
    fe = vo.frontend
    assert fe._vo_amd_klt.corners
    f0 = fe.process_image(frames[0])
    n0 = len(hooks._keypoints(f0))
    vo.keyframe = {"feats": f0, "ids": np.full(n0, -1), "T_wc": np.eye(4)}
    for k in (1, 2):
        fk = fe.process_image(frames[k])
        pairs = fe.match_frames(f0, fk)
        assert len(pairs) >= D.MIN_TRACKS and hooks._KLT_HAS_DESC not in fk  # a detected keyframe has no flag
    vo._create_keyframe(fk, np.full(len(pairs), -1), pairs[:, 0], pairs[:, 1])
    kf = vo.keyframe["feats"]
    on_device(kf)
    kp, has = hooks._keypoints(kf), kf[hooks._KLT_HAS_DESC]
    n_kept, n_kf = len(pairs), len(kp)
    assert n_kept < n_kf <= 600 and has.shape == (n_kf,) and has[:n_kept].all() and not has[n_kept:].any()
    assert len(vo.keyframe["ids"]) == n_kf and (vo.keyframe["ids"][n_kept:] == -1).all()
    assert tuple(kf["descriptors"].shape) == (1, n_kf, 128) and not hooks._np(kf["descriptors"])[0][n_kept:].any()
    np.testing.assert_array_equal(kp[:n_kept], hooks._keypoints(fk))
    # the corners are the restatement's for this image, these kept points and this room
    want, _ = R.good_features(frames[2], 600 - n_kept, 0.01, 8.0, keep=kp[:n_kept])
    np.testing.assert_array_equal(kp[n_kept:], want)
    d = np.linalg.norm(kp[n_kept:, None].astype(np.float64) - kp[None, :n_kept].astype(np.float64), axis=2)
    assert d.min() >= 8.0
    dd = np.linalg.norm(want[:, None] - want[None], axis=2) + 1e9 * np.eye(len(want))
    assert dd.min() >= 8.0
    # tracking carries on from the corners
    shift = np.float32((D.SHIFTS[3][0] - D.SHIFTS[2][0], D.SHIFTS[3][1] - D.SHIFTS[2][1]))
    f3 = fe.process_image(frames[3])
    assert f3.get(hooks._KLT_SRC) is kf
    on_device(f3)
    p3 = fe.match_frames(kf, f3)
    kp3 = hooks._keypoints(f3)
    assert np.isfinite(kp3).all()
    np.testing.assert_array_equal(f3[hooks._KLT_HAS_DESC], has[p3[:, 0]])
    corner_rows = p3[:, 0] >= n_kept
    inside = S.window_inside(kp[n_kept:], 10, D.H, D.W) & S.window_inside(kp[n_kept:] + shift, 10, D.H, D.W)
    dev = np.abs(kp3[p3[corner_rows, 1]] - kp[p3[corner_rows, 0]] - shift).max(1)
    print(f"{corner_rows.sum()} of {inside.sum()} corners inside tracked, deviation median {np.median(dev):.4f} "
          f"max {dev.max():.4f} px")
    assert corner_rows.sum() >= 0.5 * inside.sum() > 0
    assert np.median(dev) <= D.BOUND_PX
    # a frame that shares no content: detection, then descriptors over the rows that have one
    other = S.crop(S.base_image(D.H, D.W, 21), D.H, D.W)
    f4 = fe.process_image(other)
    assert hooks._KLT_SRC not in f4 and hooks._KLT_HAS_DESC not in f4
    got = fe.match_frames(kf, f4)
    sub = matcher.match_knn2_ratio(hooks._np(kf["descriptors"])[0][:n_kept], hooks._np(f4["descriptors"])[0],
                                   kind=matcher.DESC_SIFT)
    np.testing.assert_array_equal(got, sub)  # the kept rows are the first n_kept: the mapping is the identity here
    assert (got[:, 0] < n_kept).all()
    return {"kept": n_kept, "corners": n_kf - n_kept, "corners_tracked": int(corner_rows.sum()),
            "fallback_pairs": int(len(got))}
