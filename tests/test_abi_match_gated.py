"""vo_match_gated's C-ABI surface: declared, bound, and its arguments checked before any device
(or context) is touched (no GPU)."""

import ctypes as C
import re

import numpy as np
import pytest

from visualodometry_amd import _lib

F = np.ones((4, 8), np.float32)
XY = np.zeros((4, 2), np.float32)


def _call(n0=4, n1=4, dim=8, des0=F, des1=F, pred=XY, kp1=XY, radius=None, ratio=0.8, max_dist=0.0, flags=0,
          reserved=0, opt=True, pairs=True, count=True):
    lib = _lib.load()
    o = _lib.MatchGateOptionsC(pred=pred.ctypes.data if pred is not None else None,
                               radius=radius.ctypes.data if radius is not None else None,
                               kp1=kp1.ctypes.data if kp1 is not None else None, radius0=5.0, width=64, height=64,
                               ratio=ratio, max_dist=max_dist, flags=flags, reserved=reserved)
    out = np.zeros((max(n0, 1), 2), np.int32)
    cnt = np.zeros(1, np.int32)
    rc = lib.vo_match_gated(None, C.c_void_p(des0.ctypes.data if des0 is not None else None), n0,
                            C.c_void_p(des1.ctypes.data if des1 is not None else None), n1, dim,
                            C.byref(o) if opt else None, _lib.ptr(out, C.c_int32) if pairs else None, None,
                            _lib.ptr(cnt, C.c_int32) if count else None)
    return rc, lib.vo_last_error().decode()


def test_header_declares_the_function_the_flag_and_the_options():
    text = _lib.HEADER.read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+vo_match_gated\s*\(", code)
    assert re.search(r"#define\s+VO_MATCH_GATE_UNIQUE\s+2\b", code)
    assert "vo_match_gate_options" in code
    for field in ("pred", "radius", "radius0", "kp1", "width", "height", "ratio", "max_dist", "flags", "reserved"):
        assert re.search(rf"\b{field}\b", code.split("vo_match_gate_options")[0].rsplit("typedef struct", 1)[1]), field


def test_lib_binds_it_and_the_versions_stay():
    lib = _lib.load()
    assert "vo_match_gated" in _lib.SIGNATURES and hasattr(lib, "vo_match_gated")
    assert _lib.VO_MATCH_GATE_UNIQUE == 2 and _lib.VO_MATCH_DEVICE_PTRS == 1
    assert lib.vo_abi_version() == 1
    text = _lib.HEADER.read_text()
    assert re.search(r"#define\s+VO_ABI_VERSION\s+1\b", text)
    assert re.search(r"#define\s+VO_PROFILE_KERNELS\s+25\b", text)
    assert len(_lib.KERNEL_NAMES) == 25


def test_options_struct_matches_the_header_layout():
    o = _lib.MatchGateOptionsC
    assert (o.pred.offset, o.radius.offset, o.kp1.offset, o.radius0.offset, o.width.offset, o.height.offset,
            o.ratio.offset, o.max_dist.offset, o.flags.offset, o.reserved.offset) == (0, 8, 16, 24, 28, 32, 40, 48, 56,
                                                                                      60)
    assert C.sizeof(o) == 64


@pytest.mark.parametrize("kw, word", [
    (dict(opt=False), "null options"),
    (dict(pairs=False), "null options or outputs"),
    (dict(count=False), "null options or outputs"),
    (dict(n0=-1), "bad shape"),
    (dict(n1=-1), "bad shape"),
    (dict(dim=0), "bad shape"),
    (dict(flags=4), "unknown flags"),
    (dict(flags=-1), "unknown flags"),
    (dict(reserved=1), "reserved"),
    (dict(ratio=float("nan")), "ratio"),
    (dict(ratio=-0.5), "ratio"),
    (dict(ratio=float("inf")), "ratio"),
    (dict(max_dist=float("inf")), "max_dist"),
    (dict(max_dist=-1.0), "max_dist"),
    (dict(des0=None), "null array"),
    (dict(pred=None), "null array"),
    (dict(des1=None), "null array"),
    (dict(kp1=None), "null array"),
])
def test_bad_arguments_are_refused_before_the_context_is_touched(kw, word):
    rc, msg = _call(**kw)
    assert rc == _lib.VO_ERR_ARG
    assert word in msg and "vo_ctx" not in msg


def test_good_arguments_get_as_far_as_the_context():
    for kw in (dict(), dict(flags=3), dict(n0=0, des0=None, pred=None), dict(n1=0, des1=None, kp1=None),
               dict(radius=np.ones(4, np.float32), max_dist=2.0)):
        rc, msg = _call(**kw)
        assert rc == _lib.VO_ERR_ARG and "null vo_ctx" in msg


def test_project_points():
    from visualodometry_amd import matcher

    K = np.array([[100.0, 0, 50], [0, 100.0, 40], [0, 0, 1]])
    T = np.eye(4)
    T[:3, 3] = [0, 0, 1.0]  # camera frame = world + (0, 0, 1)
    X = np.array([[0, 0, 1.0], [0.1, -0.1, 1.0], [0, 0, -1.0], [0, 0, -0.95], [5.0, 0, 1.0], [0, -1.0, 1.0],
                  [-1.0, 0, 1.0]])
    pred, valid = matcher.project_points(X, T, K, (100, 80), 0.1)
    assert pred.dtype == np.float32 and pred.shape == (7, 2) and valid.dtype == bool
    assert valid.tolist() == [True, True, False, False, False, False, True]
    assert np.array_equal(pred[0], [50, 40]) and np.array_equal(pred[1], np.float32([55, 35]))
    assert np.array_equal(pred[6], [0, 40])  # u = 0 is inside, u = width is not
    assert not matcher.project_points(np.array([[1.0, 0, 1.0]]), T, K, (100, 80), 0.1)[1][0]  # u = 100
    e, v = matcher.project_points(np.zeros((0, 3)), T, K, (100, 80), 0.1)
    assert e.shape == (0, 2) and v.shape == (0,)
