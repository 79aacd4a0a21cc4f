"""A keyframe sequence with descriptors for the ``cfg.map_reobserve`` tests (tests only).

``tests.vo_scene.Scene`` gives landmarks, poses and noisy keypoints; here every landmark also has a
descriptor (integers 0..255, each keypoint a noisy copy), and the driver can lose chosen
keyframe-to-keyframe matches: the keypoint is there, but the association step misses it, so without
re-observation its landmark never gets another observation.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests.vo_scene import Cfg, FakeVO, Scene
from visualodometry_amd.synthetic import KITTI_WH

DIM = 32


@dataclass
class ReCfg(Cfg):
    ba_enabled: bool = False
    min_depth: float = 0.001
    map_reobserve: bool = False
    map_reobserve_radius: float = 10.0
    map_reobserve_ratio: float = 0.8
    map_reobserve_max_dist: float | None = 120.0  # noisy copies sit near 4 sqrt(2 DIM) = 32, strangers near 590


class DescScene(Scene):
    def __init__(self, n_kf=6, n_pts=300, seed=1, noise_px=0.5):
        super().__init__(n_kf, n_pts, seed, noise_px)
        self.D = np.random.default_rng(seed + 100).integers(0, 256, (n_pts, DIM)).astype(np.float32)

    def keypoints(self, k):
        f = super().keypoints(k)
        noise = self.rng.normal(0.0, 4.0, (f["lm"].size, DIM))
        f["descriptors"] = np.clip(np.rint(self.D[f["lm"]] + noise), 0, 255).astype(np.float32)[None]
        f["image_size"] = np.array([KITTI_WH])
        return f


def drive(vo: FakeVO, scene: DescScene, create_keyframe, lose=None, on_keyframe=None):
    """``tests.vo_scene.drive`` with exact poses; ``lose`` maps a keyframe index to true landmark
    indices whose match into that keyframe is dropped; ``on_keyframe(k, cur, curr_ids)`` runs before
    each call (``curr_ids`` is the array the call mutates) and its return value after it, if callable."""
    vo.scene = scene
    f0 = scene.keypoints(0)
    vo.keyframe = {"feats": f0, "ids": np.full(f0["lm"].size, -1), "T_wc": scene.T_wc[0].copy()}
    for k in range(1, scene.n_kf):
        prev = vo.keyframe
        cur = scene.keypoints(k)
        pos = {lm: i for i, lm in enumerate(cur["lm"])}
        lost = set((lose or {}).get(k, ()))
        ref_idx = np.array([i for i, lm in enumerate(prev["feats"]["lm"]) if lm in pos and lm not in lost], int)
        cur_idx = np.array([pos[prev["feats"]["lm"][i]] for i in ref_idx], int)
        curr_ids = np.full(cur["lm"].size, -1)
        carried = prev["ids"][ref_idx]
        ok = (carried >= 0) & np.array([c in vo.map_points for c in carried], bool)
        curr_ids[cur_idx[ok]] = carried[ok]
        vo.T_wc = scene.T_wc[k].copy()
        after = on_keyframe(k, cur, curr_ids) if on_keyframe else None
        create_keyframe(vo, cur, curr_ids, ref_idx, cur_idx)
        if callable(after):
            after()


def losable(scene: DescScene, k: int, n: int):
    """``n`` true landmarks visible in keyframes ``k - 2`` .. ``k + 1``: with ``k >= 2`` they carry an id
    into keyframe ``k``.  (Visibility alone: the scene's random stream is not touched.)"""
    from visualodometry_amd.synthetic import KITTI_K

    seen = None
    for j in (k - 2, k - 1, k, k + 1):
        T_cw = np.linalg.inv(scene.T_wc[j])
        pc = scene.X @ T_cw[:3, :3].T + T_cw[:3, 3]
        uv = pc[:, :2] / np.maximum(pc[:, 2:3], 1e-9) * [KITTI_K[0, 0], KITTI_K[1, 1]] + [KITTI_K[0, 2], KITTI_K[1, 2]]
        # a margin inside the image: the keypoints' pixel noise never moves these across its border
        vis = (pc[:, 2] > 2) & (uv[:, 0] >= 20) & (uv[:, 0] < KITTI_WH[0] - 20) & (uv[:, 1] >= 20) & \
            (uv[:, 1] < KITTI_WH[1] - 20)
        seen = vis if seen is None else seen & vis
    return np.flatnonzero(seen)[:n].tolist()
