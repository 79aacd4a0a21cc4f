"""The covariance entry point through the layers that need no GPU: declared in the product header
with the documented signature, exported, bound in ``_lib.SIGNATURES``; the Python knobs default to
off."""

import ctypes as C
import re

import numpy as np

from visualodometry_amd import _lib
from visualodometry_amd.ba import BAResult, SlidingWindowBA


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", _lib.HEADER.read_text(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared in include/vo_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_covariance_is_declared_exported_and_bound():
    assert _declaration("vo_ba_covariance") == ["vo_ctx* ctx", "uint64_t session", "double lambda",
                                                "double* pose_cov_out", "double* pose_dense_out",
                                                "double* point_cov_out"]
    PD = C.POINTER(C.c_double)
    assert _lib.SIGNATURES["vo_ba_covariance"] == (C.c_int, [C.c_void_p, C.c_uint64, C.c_double, PD, PD, PD])
    assert hasattr(_lib.load(), "vo_ba_covariance"), "vo_ba_covariance not exported by libvo_hip.so"
    for header in (_lib.TEST_HEADER, _lib.TEST_HEADER.with_name("vo_hip_testing_chain.h")):
        assert "vo_ba_covariance" not in header.read_text()
    # the header states the scaling convention
    text = _lib.HEADER.read_text()
    doc = text[text.index("Covariance read-out"):text.index("int vo_ba_covariance")]
    assert "UNIT" in doc and "sigma^2" in doc


def test_profile_ids_unchanged():
    m = re.search(r"#define\s+VO_PROFILE_KERNELS\s+(\d+)", _lib.HEADER.read_text())
    assert m and int(m.group(1)) == 25


def test_keyframe_hook_honours_the_knob(monkeypatch):
    """dropin/hooks.py asks for the covariance only when cfg.ba_covariance is set, and hands the
    result back (the keyframe hook keeps it on vo._vo_amd_last_ba)."""
    import types

    from visualodometry_amd.dropin import hooks
    from visualodometry_amd.dropin.config.config import VOConfig

    seen = []

    class Spy(SlidingWindowBA):
        def optimize(self, window, return_residuals=False, return_covariance=False):
            seen.append((return_covariance, self.covariance))
            return BAResult(np.zeros((0, 4, 4)), np.zeros((0, 3)), status="skipped")

    monkeypatch.setattr(hooks, "SlidingWindowBA", Spy)
    win = types.SimpleNamespace(build=lambda map_points: (object(), []))
    for on in (False, True):
        cfg = VOConfig()
        cfg.ba_covariance = on
        vo = types.SimpleNamespace(cfg=cfg, K=np.eye(3), map_points={})
        assert hooks.run_window_ba(vo, win).status == "skipped"
    assert seen == [(False, False), (True, True)]


def test_python_knobs_default_to_off():
    K = np.eye(3)
    assert SlidingWindowBA(K).covariance is False
    assert SlidingWindowBA(K, covariance=True).covariance is True
    cfg = type("Cfg", (), {"ba_covariance": True})()
    assert SlidingWindowBA(K, cfg).covariance is True
    r = BAResult(np.zeros((1, 4, 4)), np.zeros((1, 3)))
    assert r.pose_cov is None and r.point_cov is None and r.cov_sigma2 is None
    from visualodometry_amd.dropin.config.config import VOConfig

    assert VOConfig().ba_covariance is False
