"""``KeyframeWindow`` / ``run_window_ba`` with ``cfg.ba_marginalize`` on the host, under a stub BA:
the absorbed landmarks leave the window, n_fixed goes 2 -> 1 -> 0, the prior is carried forward,
a reset and a rejected window clear it, and a configuration without the switch builds the windows
it built before."""

import numpy as np

from visualodometry_amd.ba import BAResult, PosePrior
from visualodometry_amd.dropin.config.config import VOConfig
from visualodometry_amd.dropin.hooks import KeyframeWindow, run_window_ba

SIZE = 4


class StubBA:
    """Returns the window unchanged with a falling cost; on ``marginalize=1`` a prior over the next
    window's two leading free poses and the landmarks camera 0 sees as absorbed."""

    def __init__(self, reject=False):
        self.windows, self.kw, self.reject = [], [], reject

    def optimize(self, window, **kw):
        self.windows.append(window)
        self.kw.append(kw)
        cost = np.array([1.0, 2.0]) if self.reject else np.array([2.0, 1.0])
        res = BAResult(window.poses_cw.copy(), window.points.copy(), cost)
        if kw.get("marginalize"):
            assert kw["marginalize"] == 1
            seen = np.zeros(window.points.shape[0], bool)
            seen[window.obs_pt[window.obs_cam == 0]] = True
            first = max(window.n_fixed, 1)  # the remaining free cameras start here
            res.prior = PosePrior(np.eye(12) * (len(self.windows) + 1), np.zeros(12), window.poses_cw[first:first + 2].copy(), 1.0)
            res.point_marginalised = seen
        return res


class FakeVO:
    def __init__(self, cfg, ba):
        self.cfg, self._vo_amd_ba, self.K = cfg, ba, np.eye(3)
        self.map_points = {}
        self.keyframe = {"T_wc": np.eye(4)}
        self.T_wc = np.eye(4)
        self.last_pos = np.zeros(3)


def _drive(cfg, ba, n_keyframes, win=None):
    """Keyframe k sees landmarks k .. k + 2 (so landmark i is seen by keyframes i - 2 .. i)."""
    vo = FakeVO(cfg, ba)
    win = win or KeyframeWindow(SIZE, cfg.ba_fixed)
    out = []
    for k in range(n_keyframes):
        ids = np.arange(k, k + 3)
        for i in ids:
            vo.map_points.setdefault(int(i), np.array([float(i), 0.0, 5.0]))
        T = np.eye(4)
        T[0, 3] = k
        win.add(T, np.zeros((3, 2), np.float32) + k, ids)
        res = run_window_ba(vo, win)
        out.append((res, win.cur_fixed, win.prior, set(win.marginalised)))
    return vo, win, out


def _cfg(**kw):
    cfg = VOConfig()
    cfg.ba_enabled, cfg.ba_window, cfg.ba_fixed = True, SIZE, 2
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_switch_is_off_by_default_and_changes_nothing_when_off():
    assert VOConfig().ba_marginalize is False
    ba_off, ba_plain = StubBA(), StubBA()
    _, win, out = _drive(_cfg(), ba_off, 8)
    cfg = _cfg()
    bare = type("Cfg", (), {k: getattr(cfg, k) for k in ("ba_enabled", "ba_window", "ba_fixed")})()  # no switch at all
    _drive(bare, ba_plain, 8)
    assert all("marginalize" not in kw for kw in ba_off.kw + ba_plain.kw)
    assert win.prior is None and not win.marginalised and win.cur_fixed == 2
    assert len(ba_off.windows) == len(ba_plain.windows)
    for a, b in zip(ba_off.windows, ba_plain.windows):
        assert a.n_fixed == b.n_fixed == 2 and a.prior is None and b.prior is None
        for f in ("poses_cw", "points", "obs_uv", "obs_cam", "obs_pt"):
            np.testing.assert_array_equal(getattr(a, f), getattr(b, f))


def test_marginalised_landmarks_leave_and_the_prior_is_carried():
    ba = StubBA()
    vo, win, out = _drive(_cfg(ba_marginalize=True), ba, 8)
    asked = [bool(kw.get("marginalize")) for kw in ba.kw]
    n_first = asked.index(True)
    assert not any(asked[:n_first]) and all(asked[n_first:]), "marginalisation starts with the first full window"
    assert ba.windows[n_first].poses_cw.shape[0] == SIZE and ba.windows[n_first].prior is None
    assert [w.n_fixed for w in ba.windows[n_first:n_first + 4]] == [2, 1, 0, 0]
    for j in range(n_first, len(ba.windows) - 1):
        nxt = ba.windows[j + 1]
        res = out[-(len(ba.windows) - j)][0]
        # the next window carries exactly the prior this one returned
        assert nxt.prior is res.prior and nxt.prior.n_poses <= nxt.poses_cw.shape[0] - nxt.n_fixed
        assert nxt.poses_cw.shape[0] == SIZE
    # absorbed ids: out of every later window, still in the map
    _, _, _, absorbed = out[-1]
    assert absorbed and all(i in vo.map_points for i in absorbed)
    kf, uv, pid = win.observations(vo.map_points)
    assert not set(pid.tolist()) & absorbed
    # the set does not grow with the drive: only ids a frame of the window still sees are kept
    held = set(np.concatenate([fr.ids for fr in win.frames]).tolist())
    assert absorbed <= held and len(absorbed) <= 3 * SIZE
    assert any(a - absorbed for _, _, _, a in out), "ids absorbed earlier have been pruned since"
    win.reset()
    assert win.prior is None and not win.marginalised and win.cur_fixed == 2 and not win.frames


def test_a_rejected_window_clears_the_prior():
    cfg = _cfg(ba_marginalize=True)
    _, win, out = _drive(cfg, StubBA(), 6)
    assert win.prior is not None and win.marginalised and win.cur_fixed < 2
    vo = FakeVO(cfg, StubBA(reject=True))
    vo.map_points = {i: np.array([float(i), 0.0, 5.0]) for i in range(12)}
    T = np.eye(4)
    T[0, 3] = 6
    win.add(T, np.zeros((3, 2), np.float32), np.arange(6, 9))
    res = run_window_ba(vo, win)
    assert res is not None and res.cost_per_iter[-1] > res.cost_per_iter[0]
    assert win.prior is None and not win.marginalised and win.cur_fixed == 2
