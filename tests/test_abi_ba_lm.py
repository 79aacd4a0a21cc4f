"""Host-side surface of the BA's Levenberg-Marquardt step control: the three C-ABI prototypes load
from the built library, and the drop-in configuration carries the switch (off by default) into
SlidingWindowBA.  Option validation needs a session, so it is in tests/test_gpu_ba_lm.py.
"""

import ctypes as C
import re
import types
from pathlib import Path

import numpy as np

from visualodometry_amd import _lib
from visualodometry_amd.ba import BAResult, BASession, SlidingWindowBA
from visualodometry_amd.dropin.config.config import VOConfig

HEADER = Path(__file__).resolve().parents[1] / "include" / "vo_hip.h"


def test_prototypes_load():
    lib = _lib.load()
    for name in ("vo_ba_run_lm", "vo_ba_run_lm_async", "vo_ba_lm_log"):
        assert name in _lib.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SIGNATURES[name][1]
        assert re.search(rf"\bint {name}\(", HEADER.read_text())
    assert lib.vo_abi_version() == 1
    assert C.sizeof(_lib.BALmOptionsC) == 5 * 8
    assert [f[0] for f in _lib.BALmOptionsC._fields_] == ["lambda0", "up", "down", "lambda_min", "lambda_max"]
    for m in ("run_lm", "run_lm_async", "lm_log"):
        assert callable(getattr(BASession, m))


def test_config_switch_is_off_by_default_and_reaches_the_ba():
    assert VOConfig().ba_lm is False
    K = np.eye(3)
    assert SlidingWindowBA(K, VOConfig()).lm is False
    cfg = VOConfig()
    cfg.ba_lm = True
    ba = SlidingWindowBA(K, cfg)
    assert ba.lm is True and ba.lam == cfg.ba_lambda  # ba_lambda: then the schedule's starting value
    assert SlidingWindowBA(K).lm is False and SlidingWindowBA(K, lm=True).lm is True
    r = BAResult(np.zeros((0, 4, 4)), np.zeros((0, 3)))
    assert r.lambdas is None and r.accepted is None


def test_keyframe_hook_hands_the_config_to_the_ba(monkeypatch):
    """dropin/hooks.py builds its SlidingWindowBA from the VO's cfg: ba_lm needs nothing more there."""
    from visualodometry_amd.dropin import hooks

    seen = {}

    class Spy(SlidingWindowBA):
        def optimize(self, window, return_residuals=False):
            seen["lm"], seen["lam"] = self.lm, self.lam
            return BAResult(np.zeros((0, 4, 4)), np.zeros((0, 3)), status="skipped")

    monkeypatch.setattr(hooks, "SlidingWindowBA", Spy)
    cfg = VOConfig()
    cfg.ba_lm = True
    vo = types.SimpleNamespace(cfg=cfg, K=np.eye(3), map_points={})
    win = types.SimpleNamespace(build=lambda map_points: (object(), []))
    res = hooks.run_window_ba(vo, win)
    assert res.status == "skipped" and seen == {"lm": True, "lam": cfg.ba_lambda}
