"""The ``cfg.klt_tracking`` route end to end for the GPU tests: the real frontend hooks (GPU SIFT,
``klt.track``, the descriptor matcher) over crops of one textured image at planted offsets, with a
stub owner holding ``keyframe``.  ``run(device)`` is shared by the in-process test (numpy feature
dicts) and the torch script (CUDA tensors); it returns the figures it checked."""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from tests import klt_scene as S

H, W = 200, 320
# frame k's content relative to frame 0.  Offsets of a few pixels per frame: the points are DoG extrema, not
# corners, and at (9, 3) and beyond one of ~500 settles 6 px off, consistently forwards and backwards, so the
# check at 1 px cannot see it (measured with the restatement; the tracker itself is checked in test_gpu_klt.py)
SHIFTS = [(0, 0), (2, 1), (5, 2), (8, 3)]
BOUND_PX = 0.1
MIN_TRACKS = 100


def config(device):
    return SimpleNamespace(extractor_type="sift", sift_on_gpu=True, match_on_gpu=True, sift_n_features=600,
                           sift_contrast_threshold=0.02, sift_edge_threshold=2.0, sift_sigma=1.6, ba_enabled=False,
                           klt_tracking=True, klt_win_radius=10, klt_levels=4, klt_fb_thresh=1.0,
                           klt_min_tracks=MIN_TRACKS, klt_min_distance=8.0, device=device)


def classes():
    """Stand-ins for the reference's FeatureFrontend and VisualOdometry with the hooks installed."""
    from visualodometry_amd.dropin import hooks

    class Frontend:
        def __init__(self, config):
            self.conf = config
            self.device = config.device
            self.extractor = None

        def process_image(self, img):  # the reference's body (frontend.py:51-75) on numpy
            kps, des = self.extractor.detectAndCompute(img, None)
            pts = np.array([k.pt for k in kps], np.float32).reshape(-1, 2)
            return {"keypoints": pts[None], "descriptors": np.asarray(des, np.float32).reshape(-1, 128)[None],
                    "image_size": np.array([(img.shape[1], img.shape[0])])}

        def match_frames(self, feats0, feats1):
            raise AssertionError("the reference's matcher is not reached")

    class Owner:
        def __init__(self, K, config):
            self.K, self.cfg = K, config
            self.frontend = Frontend(config)
            self.keyframe, self.map_points, self.next_pt_id, self.T_wc = None, {}, 0, np.eye(4)
            self.last_pos = np.zeros(3)

        def _create_keyframe(self, curr_feats, curr_ids, ref_indices, curr_indices):
            self.keyframe = {"feats": curr_feats, "ids": curr_ids, "T_wc": self.T_wc.copy()}

        def _reset_system(self):
            self.keyframe = None

    hooks.install(Frontend, Owner)
    return Frontend, Owner


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

    base = S.base_image(H, W, 8)
    frames = [S.crop(base, H, W, s) for s in SHIFTS]
    _, Owner = classes()
    vo = Owner(np.eye(3), config(device))
    fe = vo.frontend
    f0 = fe.process_image(frames[0])
    on_device(f0)
    kp0 = hooks._keypoints(f0)
    n0 = len(kp0)
    assert n0 >= 3 * MIN_TRACKS, n0
    assert hooks._KLT_SRC not in f0 and f0[hooks._KLT_IMAGE] is frames[0]
    vo.keyframe = {"feats": f0, "ids": np.full(n0, -1), "T_wc": np.eye(4)}
    out = {"n0": n0, "tracked": [], "max_dev": []}
    alive = None

    def check_tracked(fk, src_feats, shift):
        assert fk.get(hooks._KLT_SRC) is src_feats
        on_device(fk)
        pairs = fe.match_frames(src_feats, fk)
        assert pairs.dtype == np.int64 and pairs.shape[1] == 2
        np.testing.assert_array_equal(pairs[:, 1], np.arange(len(pairs)))
        src_kp, kp = hooks._keypoints(src_feats), hooks._keypoints(fk)
        assert fk["keypoints"].shape == (1, len(pairs), 2) and fk["descriptors"].shape == (1, len(pairs), 128)
        np.testing.assert_array_equal(hooks._np(fk["descriptors"])[0], hooks._np(src_feats["descriptors"])[0][pairs[:, 0]])
        dev = np.abs(kp[pairs[:, 1]] - src_kp[pairs[:, 0]] - np.float32(shift)).max()
        inside = S.window_inside(src_kp, 10, H, W) & S.window_inside(src_kp + np.float32(shift), 10, H, W)
        out["tracked"].append((len(pairs), int(inside.sum())))
        out["max_dev"].append(float(dev))
        print(f"shift {shift}: {len(pairs)} pairs of {inside.sum()} keypoints inside, max deviation {dev:.4f} px")
        assert dev <= BOUND_PX
        # DoG extrema are not all corners: some fail the eigenvalue test.  Half of those that stay
        # inside is the guard against a route that passes by dropping points.
        assert len(pairs) >= 0.5 * inside.sum() and len(pairs) >= MIN_TRACKS
        return pairs

    for k in (1, 2):
        fk = fe.process_image(frames[k])
        pairs = check_tracked(fk, f0, SHIFTS[k])
        if alive is not None:  # a point once lost stays lost
            assert np.isin(pairs[:, 0], alive).all()
        alive = pairs[:, 0]
    # frame 2 becomes the keyframe: replenished by detection away from its tracked keypoints
    ids = np.full(len(pairs), -1)
    vo._create_keyframe(fk, ids, pairs[:, 0], pairs[:, 1])
    kf = vo.keyframe["feats"]
    on_device(kf)
    n_kept, n_kf = len(pairs), hooks._keypoints(kf).shape[0]
    assert n_kept < n_kf <= 600 and len(vo.keyframe["ids"]) == n_kf and (vo.keyframe["ids"][n_kept:] == -1).all()
    kp_kf = hooks._keypoints(kf)
    np.testing.assert_array_equal(kp_kf[:n_kept], hooks._keypoints(fk))
    d = np.linalg.norm(kp_kf[n_kept:, None] - kp_kf[None, :n_kept], axis=2)
    assert d.min() >= 8.0
    out["replenished"] = n_kf - n_kept
    f3 = fe.process_image(frames[3])
    check_tracked(f3, kf, (SHIFTS[3][0] - SHIFTS[2][0], SHIFTS[3][1] - SHIFTS[2][1]))
    # a frame that shares no content with the keyframe: detection and descriptor matching
    other = S.crop(S.base_image(H, W, 21), H, W)
    f4 = fe.process_image(other)
    on_device(f4)
    assert hooks._KLT_SRC not in f4 and f4[hooks._KLT_IMAGE] is other
    got = fe.match_frames(kf, f4)
    want = matcher.match_knn2_ratio(hooks._np(kf["descriptors"])[0], hooks._np(f4["descriptors"])[0],
                                    kind=matcher.DESC_SIFT)
    np.testing.assert_array_equal(got, want)
    out["fallback_keypoints"] = int(hooks._keypoints(f4).shape[0])
    vo._reset_system()
    assert fe._vo_amd_klt.src is None
    return out
