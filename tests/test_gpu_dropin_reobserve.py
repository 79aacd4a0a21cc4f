"""``cfg.map_reobserve`` through the real ``matcher.match_gated`` on the GPU: a scene with known
landmarks, descriptors and poses in which some keyframe-to-keyframe matches are lost; those
landmarks get their true ids back in that keyframe, and no id appears twice in a keyframe."""

import numpy as np
import pytest

from tests.reobserve_scene import DescScene, ReCfg, drive, losable
from tests.vo_scene import FakeVO
from visualodometry_amd.dropin import hooks

pytestmark = pytest.mark.gpu

LOSE_AT = 3


def _run(on):
    scene = DescScene()
    vo = FakeVO(ReCfg(map_reobserve=on), tri_noise=0.01)
    lost = losable(scene, LOSE_AT, 8)
    lm_log = []
    drive(vo, scene, hooks._wrap_create_keyframe(FakeVO._create_keyframe), {LOSE_AT: lost},
          lambda k, cur, ids: lm_log.append(cur["lm"]))
    return vo, lost, lm_log[LOSE_AT - 1]


def test_lost_landmarks_get_their_ids_back(ctx):
    off, lost, lm = _run(False)
    fr = off._vo_amd_window.frames[LOSE_AT]
    slots = np.array([s for s in range(len(lm)) if lm[s] in lost])
    assert len(slots) == 8 and (fr.ids[slots] == -1).all()  # today: unlabelled, and never again observed
    on, _, lm_on = _run(True)
    np.testing.assert_array_equal(lm, lm_on)
    fr = on._vo_amd_window.frames[LOSE_AT]
    # the ids these landmarks held before that keyframe (the double triangulates 90 % of its matches)
    born = {}
    for i in sorted(on.truth):
        born.setdefault(on.truth[i], i)
    prev_ids = on._vo_amd_window.frames[LOSE_AT - 1].ids
    held = {lmk: born[lmk] for lmk in lost if lmk in born and born[lmk] in prev_ids.tolist()}
    assert len(held) >= 4
    for s in slots:
        if lm[s] in held:
            assert fr.ids[s] == held[lm[s]], "the landmark's own id, not a neighbour's"
    # every id written anywhere names the landmark actually seen there, and none appears twice
    n_back = 0
    for f in on._vo_amd_window.frames:
        live = f.ids[f.ids >= 0]
        assert len(np.unique(live)) == len(live)
    for s, i in enumerate(fr.ids):
        if i >= 0:
            assert on.truth[int(i)] == lm[s]
            n_back += 1
    assert n_back > (off._vo_amd_window.frames[LOSE_AT].ids >= 0).sum()
    # the window sees the longer tracks
    kf, _, pid = on._vo_amd_window.observations(on.map_points)
    for i in held.values():
        assert LOSE_AT in kf[pid == i].tolist()
