"""``KeyframeWindow`` / ``run_window_ba`` with ``cfg.ba_motion_factors`` on the host, under a stub BA:
the front end's relative pose is recorded with each keyframe as the poses stand then, ``build`` emits
the chain over the consecutive pairs still in the window only when the switch is on, a pair whose
older keyframe left on a slide is not emitted, a reset clears the record, and a window built with the
switch off equals today's field for field."""

import dataclasses

import numpy as np

from tests.test_dropin_marginalize_host import SIZE, FakeVO, StubBA, _cfg
from visualodometry_amd.ba import BAWindow
from visualodometry_amd.dropin.config.config import VOConfig
from visualodometry_amd.dropin.hooks import KeyframeWindow, run_window_ba

SIGMA_T, SIGMA_R = 0.25, 0.05


class MovingBA(StubBA):
    """The stub BA, but it moves every pose a little: what was recorded before BA must not follow."""

    def optimize(self, window, **kw):
        res = super().optimize(window, **kw)
        res.poses_cw = window.poses_cw.copy()
        res.poses_cw[:, 0, 3] += 0.125
        return res


def _pose(k):
    T = np.eye(4)
    c, s = np.cos(0.1 * k), np.sin(0.1 * k)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    T[:3, 3] = [k, 0.5 * k, 0.0]
    return T


def _window(cfg):
    return KeyframeWindow(SIZE, cfg.ba_fixed, motion_factors=cfg.ba_motion_factors, motion_sigma_t=cfg.ba_motion_sigma_t,
                          motion_sigma_r=cfg.ba_motion_sigma_r)


def _drive(cfg, ba, n_keyframes):
    vo = FakeVO(cfg, ba)
    win = _window(cfg)
    before = []  # per keyframe: (T_wc of the previous keyframe, T_wc of the new one) at add time
    for k in range(n_keyframes):
        ids = np.arange(k, k + 3)
        for i in ids:
            vo.map_points.setdefault(int(i), np.array([float(i), 0.0, 5.0]))
        prev = win.frames[-1].T_wc.copy() if win.frames else None
        win.add(_pose(k), np.zeros((3, 2), np.float32) + k, ids)
        before.append((prev, _pose(k)))
        run_window_ba(vo, win)
    return vo, win, before


def _on(**kw):
    return _cfg(ba_motion_factors=True, ba_motion_sigma_t=SIGMA_T, ba_motion_sigma_r=SIGMA_R, **kw)


def test_switch_is_off_by_default_and_changes_nothing_when_off():
    cfg = VOConfig()
    assert cfg.ba_motion_factors is False
    ba_off, ba_bare = StubBA(), StubBA()
    _drive(_cfg(), ba_off, 7)
    vo = FakeVO(_cfg(), ba_bare)
    win = KeyframeWindow(SIZE, 2)  # as built before the switch existed
    for k in range(7):
        ids = np.arange(k, k + 3)
        for i in ids:
            vo.map_points.setdefault(int(i), np.array([float(i), 0.0, 5.0]))
        win.add(_pose(k), np.zeros((3, 2), np.float32) + k, ids)
        run_window_ba(vo, win)
    assert all(fr.motion is None for fr in win.frames)
    assert len(ba_off.windows) == len(ba_bare.windows) > 0
    names = [f.name for f in dataclasses.fields(BAWindow)]
    assert "factors" in names
    for a, b in zip(ba_off.windows, ba_bare.windows):
        assert a.factors is None and b.factors is None
        for f in names:
            x, y = getattr(a, f), getattr(b, f)
            if isinstance(x, np.ndarray):
                np.testing.assert_array_equal(x, y)
            else:
                assert x == y, f
    assert ba_off.kw == ba_bare.kw


def test_the_chain_is_recorded_before_ba_and_emitted():
    ba = MovingBA()
    vo, win, before = _drive(_on(), ba, 7)
    info = np.diag([1 / SIGMA_T**2] * 3 + [1 / SIGMA_R**2] * 3)
    for n, w in enumerate(ba.windows):
        k_last = n + 2  # the first window is built at the third keyframe (n_fixed = 2)
        k_first = max(0, k_last - SIZE + 1)
        fs = w.factors
        assert fs is not None and len(fs) == w.poses_cw.shape[0] - 1
        for q, f in enumerate(fs):
            assert (f.cam_i, f.cam_j) == (q, q + 1), "between window cameras k - 1 and k"
            prev, new = before[k_first + q + 1]
            # Z = T_cw(prev) T_cw(new)^-1 as the two stood when the newer was added: the older one after
            # the BA calls before that moment, the newer one as the front end gave it
            np.testing.assert_allclose(f.meas, np.linalg.inv(prev) @ new, rtol=0, atol=1e-12)
            np.testing.assert_array_equal(f.info, info)
    # the recorded motions did not follow the BA's later pose changes
    assert not np.allclose(win.frames[-2].T_wc, _pose(5))


def test_a_pair_whose_older_keyframe_left_is_not_emitted_and_reset_clears():
    ba = StubBA()
    vo, win, _ = _drive(_on(ba_marginalize=True), ba, 8)
    for w in ba.windows:
        n = w.poses_cw.shape[0]
        assert [(f.cam_i, f.cam_j) for f in w.factors] == [(q, q + 1) for q in range(n - 1)]
        assert n <= SIZE
    # the oldest keyframe of the window still holds its record to a keyframe that left: not emitted
    assert win.frames[0].motion is not None and len(win.factors()) == len(win.frames) - 1
    win.reset()
    assert not win.frames and win.factors() is None
    win.add(_pose(0), np.zeros((1, 2), np.float32), np.array([0]))
    assert win.frames[0].motion is None and win.factors() is None
