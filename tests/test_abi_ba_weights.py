"""The observation-weight and cull entry points through the layers that need no GPU: declared in the
product header with the documented signatures, exported, bound in ``_lib.SIGNATURES``; the options
struct has the header's layout; the Python knobs default to off and refuse bad values."""

import ctypes as C
import re

import numpy as np
import pytest

from visualodometry_amd import _lib
from visualodometry_amd.ba import BAResult, BASession, BAWindow, SlidingWindowBA


def _header():
    return re.sub(r"/\*.*?\*/", "", _lib.HEADER.read_text(), flags=re.S)


def _declaration(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, f"{name} is not declared in include/vo_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_entry_points_are_declared_exported_and_bound():
    assert _declaration("vo_ba_set_obs_weights") == ["vo_ctx* ctx", "uint64_t session", "const double* w"]
    assert _declaration("vo_ba_get_obs_weights") == ["vo_ctx* ctx", "uint64_t session", "double* w_out"]
    assert _declaration("vo_ba_cull") == ["vo_ctx* ctx", "uint64_t session", "const vo_ba_cull_options* opt",
                                          "int32_t* n_culled_out", "int32_t* n_active_out"]
    assert _declaration("vo_ba_cull_async") == ["vo_ctx* ctx", "uint64_t session", "const vo_ba_cull_options* opt"]
    PD, PI = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    PO = C.POINTER(_lib.BACullOptionsC)
    sig = _lib.SIGNATURES
    assert sig["vo_ba_set_obs_weights"] == (C.c_int, [C.c_void_p, C.c_uint64, PD])
    assert sig["vo_ba_get_obs_weights"] == (C.c_int, [C.c_void_p, C.c_uint64, PD])
    assert sig["vo_ba_cull"] == (C.c_int, [C.c_void_p, C.c_uint64, PO, PI, PI])
    assert sig["vo_ba_cull_async"] == (C.c_int, [C.c_void_p, C.c_uint64, PO])
    lib = _lib.load()
    for name in ("vo_ba_set_obs_weights", "vo_ba_get_obs_weights", "vo_ba_cull", "vo_ba_cull_async"):
        assert hasattr(lib, name), f"{name} not exported by libvo_hip.so"
        for header in (_lib.TEST_HEADER, _lib.TEST_HEADER.with_name("vo_hip_testing_chain.h")):
            assert name not in header.read_text()


def test_abi_version_and_profile_ids_unchanged():
    text = _lib.HEADER.read_text()
    m = re.search(r"#define\s+VO_ABI_VERSION\s+(\d+)", text)
    assert m and int(m.group(1)) == 1
    m = re.search(r"#define\s+VO_PROFILE_KERNELS\s+(\d+)", text)
    assert m and int(m.group(1)) == 25


def test_cull_options_layout():
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*vo_ba_cull_options\s*;", _header())
    assert m, "vo_ba_cull_options is not declared"
    fields = [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == ["double max_chi2", "double min_depth", "int32_t min_track", "int32_t reserved"]
    assert [(n, t) for n, t in _lib.BACullOptionsC._fields_] == [
        ("max_chi2", C.c_double), ("min_depth", C.c_double), ("min_track", C.c_int32), ("reserved", C.c_int32)]
    assert C.sizeof(_lib.BACullOptionsC) == 24


def test_header_states_the_semantics():
    text = _lib.HEADER.read_text()
    doc = text[text.index("Observation weights."):text.index("int vo_ba_set_obs_weights")]
    assert "select" in doc and "whitened" in doc and "sqrt(w_o)" in doc
    doc = text[text.index("Device-side outlier culling"):text.index("int vo_ba_cull(")]
    assert "w_o * err2_o > max_chi2" in doc and "z_o <= min_depth" in doc and "min_track" in doc


def test_session_wrapper_checks_the_weight_count():
    """One weight per observation: checked in Python before the library reads past a short array."""
    s = BASession.__new__(BASession)  # no device: only the shape check is reached
    s.obs_cam = np.zeros(5, dtype=np.int32)
    with pytest.raises(ValueError):
        s.set_obs_weights(np.ones(4))


def test_write_back_skips_a_landmark_without_active_observations():
    """The keyframe hook under culling: a landmark all of whose observations were culled was held by
    nothing in the last solve, so its adjusted position does not reach the map."""
    from visualodometry_amd.dropin.hooks import KeyframeWindow

    win = KeyframeWindow(size=4, n_fixed=1)
    for k in range(2):
        win.add(np.eye(4), np.zeros((3, 2), np.float32), np.array([10, 11, 12]))
    old = {10: np.zeros(3), 11: np.zeros(3), 12: np.zeros(3)}
    obs_pt = np.array([0, 0, 1, 1, 2, 2])
    active = np.array([True, True, False, False, True, False])  # landmark 1 lost both, landmark 2 one
    res = BAResult(np.tile(np.eye(4), (2, 1, 1)), np.arange(9.0).reshape(3, 3) + 1.0, obs_active=active)
    mp = {k: v.copy() for k, v in old.items()}
    win.write_back(res, np.array([10, 11, 12]), mp, obs_pt)
    np.testing.assert_array_equal(mp[10], [1.0, 2.0, 3.0])
    np.testing.assert_array_equal(mp[11], old[11])
    np.testing.assert_array_equal(mp[12], [7.0, 8.0, 9.0])
    mp = {k: v.copy() for k, v in old.items()}
    res.obs_active = None  # no culling: every landmark is written, as before
    win.write_back(res, np.array([10, 11, 12]), mp, obs_pt)
    np.testing.assert_array_equal(mp[11], [4.0, 5.0, 6.0])


def test_python_knobs_default_to_off_and_refuse_bad_values():
    K = np.eye(3)
    ba = SlidingWindowBA(K)
    assert ba.cull_rounds == 0 and ba.cull_chi2 == 0.0 and ba.cull_min_depth == 0.0
    cfg = type("Cfg", (), {"ba_cull_rounds": 2, "ba_cull_chi2": 9.0, "ba_cull_min_depth": 0.1})()
    ba = SlidingWindowBA(K, cfg)
    assert (ba.cull_rounds, ba.cull_chi2, ba.cull_min_depth) == (2, 9.0, 0.1)
    assert SlidingWindowBA(K, cull_rounds=1, cull_chi2=4.0).cull_rounds == 1
    for bad in (dict(cull_rounds=-1), dict(cull_chi2=-1.0), dict(cull_chi2=float("nan")),
                dict(cull_min_depth=float("inf"))):
        with pytest.raises(ValueError):
            SlidingWindowBA(K, **bad)
    r = BAResult(np.zeros((1, 4, 4)), np.zeros((1, 3)))
    assert r.obs_active is None
    w = BAWindow(np.zeros((1, 4, 4)), np.zeros((1, 3)), np.zeros((1, 2), np.float32), np.zeros(1, int), np.zeros(1, int))
    assert w.obs_weight is None
    from visualodometry_amd.dropin.config.config import VOConfig

    c = VOConfig()
    assert c.ba_cull_rounds == 0 and c.ba_cull_chi2 == 0.0 and c.ba_cull_min_depth == 0.0
