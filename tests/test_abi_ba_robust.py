"""The robust-cost entry points through the layers that need no GPU: declared in the product
header with the documented signatures, exported, bound in ``_lib.SIGNATURES``; the Python knobs
default to off."""

import ctypes as C
import re

import numpy as np
import pytest

from visualodometry_amd import _lib
from visualodometry_amd.ba import BAResult, SlidingWindowBA


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", _lib.HEADER.read_text(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared in include/vo_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_new_calls_are_declared_exported_and_bound():
    assert _declaration("vo_ba_set_robust") == ["vo_ctx* ctx", "uint64_t session", "double huber_delta"]
    assert _declaration("vo_ba_residuals") == ["vo_ctx* ctx", "uint64_t session", "double* err2_out",
                                               "double* depth_out"]
    lib = _lib.load()
    PD = C.POINTER(C.c_double)
    assert _lib.SIGNATURES["vo_ba_set_robust"] == (C.c_int, [C.c_void_p, C.c_uint64, C.c_double])
    assert _lib.SIGNATURES["vo_ba_residuals"] == (C.c_int, [C.c_void_p, C.c_uint64, PD, PD])
    for name in ("vo_ba_set_robust", "vo_ba_residuals"):
        assert hasattr(lib, name), f"{name} not exported by libvo_hip.so"
    assert "vo_ba_set_robust" not in _lib.TEST_HEADER.read_text()


def test_python_knobs_default_to_off():
    K = np.eye(3)
    assert SlidingWindowBA(K).huber == 0.0
    assert SlidingWindowBA(K, huber=2.0).huber == 2.0
    cfg = type("Cfg", (), {"ba_huber": 1.5})()
    assert SlidingWindowBA(K, cfg, huber=2.0).huber == 1.5
    for bad in (-1.0, float("nan"), float("inf")):  # a configuration error, not a skipped window
        with pytest.raises(ValueError):
            SlidingWindowBA(K, huber=bad)
        with pytest.raises(ValueError):
            SlidingWindowBA(K, type("Cfg", (), {"ba_huber": bad})())
    r = BAResult(np.zeros((1, 4, 4)), np.zeros((1, 3)))
    assert r.obs_err2 is None and r.obs_depth is None
    from visualodometry_amd.dropin.config.config import VOConfig

    assert VOConfig().ba_huber == 0.0
