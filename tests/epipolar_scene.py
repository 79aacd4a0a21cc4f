"""The drive the ``cfg.map_epipolar_search`` tests share (tests only): ``tests.reobserve_scene``'s
keyframe sequence with descriptors, in which the keyframe-to-keyframe match of chosen landmarks that
have no id yet is lost, so only the epipolar search can make them landmarks at that keyframe."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests.reobserve_scene import DescScene, ReCfg, drive
from tests.vo_scene import FakeVO
from visualodometry_amd.dropin import hooks
from visualodometry_amd.synthetic import KITTI_K, KITTI_WH

LOSE_AT = 1  # before keyframe 1 nothing has an id
N_LOST = 60


@dataclass
class EpiCfg(ReCfg):
    max_reproj_err: float = 5.0
    map_epipolar_search: bool = False
    map_epipolar_radius: float = 2.0
    map_epipolar_ratio: float = 0.8
    map_epipolar_max_dist: float | None = 120.0  # noisy copies sit near 4 sqrt(2 DIM) = 32, strangers near 590
    map_epipolar_min_depth: float = 1.0
    map_epipolar_max_depth: float = 0.0
    map_epipolar_min_length: float = 8.0


class PruningVO(FakeVO):
    """The double with the reference's ``_prune_map`` call sites counted (``vo.py:288``)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.prunes = 0

    def _prune_map(self):
        self.prunes += 1


def covisible(scene: DescScene, k: int, n: int):
    """``n`` true landmarks visible, 20 px inside the image, in keyframes ``k - 1`` and ``k``.
    (Visibility alone: the scene's random stream is not touched.)"""
    seen = None
    for j in (k - 1, k):
        T_cw = np.linalg.inv(scene.T_wc[j])
        pc = scene.X @ T_cw[:3, :3].T + T_cw[:3, 3]
        uv = pc[:, :2] / np.maximum(pc[:, 2:3], 1e-9) * [KITTI_K[0, 0], KITTI_K[1, 1]] + [KITTI_K[0, 2], KITTI_K[1, 2]]
        vis = (pc[:, 2] > 2) & (uv[:, 0] >= 20) & (uv[:, 0] < KITTI_WH[0] - 20) & (uv[:, 1] >= 20) & \
            (uv[:, 1] < KITTI_WH[1] - 20)
        seen = vis if seen is None else seen & vis
    return np.flatnonzero(seen)[:n].tolist()


@dataclass
class Run:
    vo: PruningVO
    scene: DescScene
    lost: list
    feats: list   # the feature dict of every keyframe, 0 first
    calls: list   # what epipolar_search saw and returned, one entry per call


def run(cfg, lose=True) -> Run:
    """Drive the hooked ``_create_keyframe`` over the scene; every ``hooks.epipolar_search`` call is
    recorded with copies of the arrays as they stood when it was made."""
    scene = DescScene()
    vo = PruningVO(cfg, tri_noise=0.01)
    lost = covisible(scene, LOSE_AT, N_LOST)
    assert len(lost) == N_LOST
    feats, calls = [], []
    real = hooks.epipolar_search

    def spy(vo_, prev, curr_feats, curr_ids, ref_indices, curr_indices):
        rec = dict(k=len(feats) - 1, prev=prev, prev_ids=np.array(prev["ids"]), ids_before=curr_ids.copy(),
                   ref=np.array(ref_indices), cur=np.array(curr_indices), next_before=vo_.next_pt_id,
                   prunes_before=vo_.prunes)
        rec["uv"], rec["ids"] = real(vo_, prev, curr_feats, curr_ids, ref_indices, curr_indices)
        rec["ids_after"] = curr_ids.copy()
        calls.append(rec)
        return rec["uv"], rec["ids"]

    def on_keyframe(k, cur, curr_ids):
        if not feats:
            feats.append(vo.keyframe["feats"])
        feats.append(cur)

    hooks.epipolar_search = spy
    try:
        drive(vo, scene, hooks._wrap_create_keyframe(PruningVO._create_keyframe), {LOSE_AT: lost} if lose else None,
              on_keyframe)
    finally:
        hooks.epipolar_search = real
    return Run(vo, scene, lost, feats, calls)
