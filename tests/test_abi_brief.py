"""The C-ABI surface of the BRIEF descriptor and the Hamming matcher: declared, exported, bound, the
options struct laid out as the header's, and the arguments checked before any device (or context)
is touched (no GPU)."""

import ctypes as C
import re

import numpy as np
import pytest

from visualodometry_amd import _lib, brief, matcher

IMG = np.zeros((40, 48), np.uint8)
PTS = np.full((4, 2), 20.0, np.float32)
D0 = np.zeros((5, 8), np.uint32)
D1 = np.ones((6, 8), np.uint32)


def _describe(img=IMG, tag=0, h=40, w=48, pts=PTS, n=4, flags=0, des=True):
    lib = _lib.load()
    out = np.zeros((8, 8), np.uint32)
    rc = lib.vo_brief_describe(None, None if img is None else img.ctypes.data, tag, h, w,
                               None if pts is None else pts.ctypes.data, n, flags, out.ctypes.data if des else None,
                               None, None)
    return rc, lib.vo_last_error().decode()


def _hamming(des0=D0, n0=5, des1=D1, n1=6, words=8, opt=True, pairs=True, count=True, knn=False, **fields):
    lib = _lib.load()
    o = dict(ratio=0.8, max_dist=64, flags=0, reserved=0)
    o.update(fields)
    o = _lib.MatchHammingOptionsC(**o)
    out = np.zeros((16, 2), np.int32)
    cnt = C.c_int32(-7)
    kidx, kdist = np.zeros((16, 2), np.int32), np.zeros((16, 2), np.int32)
    rc = lib.vo_match_hamming(None, None if des0 is None else des0.ctypes.data, n0,
                              None if des1 is None else des1.ctypes.data, n1, words, C.byref(o) if opt else None,
                              out.ctypes.data if pairs else None, None, C.byref(cnt) if count else None,
                              kidx.ctypes.data if knn else None, kdist.ctypes.data if knn else None)
    return rc, lib.vo_last_error().decode(), cnt.value, kidx, kdist


def test_header_declares_the_functions_and_the_options():
    text = _lib.HEADER.read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for fn in ("vo_brief_describe", "vo_brief_pattern", "vo_match_hamming"):
        assert re.search(rf"\bint\s+{fn}\s*\(", code), fn
        assert fn in _lib.SIGNATURES and hasattr(_lib.load(), fn)
    body = code.split("vo_match_hamming_options")[0].rsplit("typedef struct", 1)[1]
    names = re.findall(r"\b(ratio|max_dist|flags|reserved)\b", body)
    assert names == [n for n, _ in _lib.MatchHammingOptionsC._fields_]
    assert C.sizeof(_lib.MatchHammingOptionsC) == 24
    assert [getattr(_lib.MatchHammingOptionsC, n).offset for n in names] == [0, 8, 12, 16]
    assert re.search(r"#define\s+VO_MATCH_HAMMING_MUTUAL\s+4\b", text) and _lib.VO_MATCH_HAMMING_MUTUAL == 4


def test_the_versions_and_the_profiler_table_stay():
    text = _lib.HEADER.read_text()
    assert _lib.load().vo_abi_version() == 1
    assert re.search(r"#define\s+VO_ABI_VERSION\s+1\b", text)
    assert re.search(r"#define\s+VO_PROFILE_KERNELS\s+25\b", text)
    assert len(_lib.KERNEL_NAMES) == 25


@pytest.mark.parametrize("kw, word", [
    (dict(des=False), "null des_out"),
    (dict(pts=None), "null pts"),
    (dict(img=None), "null image with tag 0"),
    (dict(h=0), "bad shape"),
    (dict(w=-2), "bad shape"),
    (dict(h=1 << 16, w=1 << 15), "bad shape"),
    (dict(n=-1), "bad shape"),
    (dict(flags=1), "unknown flags"),
])
def test_describe_refuses_bad_arguments_without_a_device(kw, word):
    rc, msg = _describe(**kw)
    assert rc == _lib.VO_ERR_ARG and word in msg, (rc, msg)


def test_describe_of_no_points_touches_nothing():
    assert _describe(n=0)[0] == _lib.VO_OK and _describe(n=0, pts=None)[0] == _lib.VO_OK
    des, bins, status = brief.describe(IMG, np.zeros((0, 2), np.float32))
    assert des.shape == (0, 8) and des.dtype == np.uint32 and bins.shape == (0,) and status.shape == (0,)
    # a good call gets as far as the context: a NULL one is refused there, after the arguments
    rc, msg = _describe()
    assert rc == _lib.VO_ERR_ARG and "null vo_ctx" in msg


def test_pattern_needs_no_context_and_refuses_null_outputs():
    lib = _lib.load()
    d = np.zeros(64, np.int32)
    assert lib.vo_brief_pattern(None, d.ctypes.data) == _lib.VO_ERR_ARG
    P, Cc, S = brief.pattern()
    assert P.shape == (32, 256, 4) and Cc[0] == 16384 and S[8] == 16384 and Cc[16] == -16384


@pytest.mark.parametrize("kw, word", [
    (dict(opt=False), "null options or outputs"),
    (dict(pairs=False), "null options or outputs"),
    (dict(count=False), "null options or outputs"),
    (dict(des0=None), "null array"),
    (dict(des1=None), "null array"),
    (dict(n0=-1), "bad shape"),
    (dict(n1=-1), "bad shape"),
    (dict(words=0), "bad shape"),
    (dict(words=17), "bad shape"),
    (dict(ratio=float("nan")), "ratio"),
    (dict(ratio=float("inf")), "ratio"),
    (dict(ratio=-0.1), "ratio"),
    (dict(max_dist=-1), "max_dist"),
    (dict(flags=2), "unknown flags"),
    (dict(flags=8), "unknown flags"),
    (dict(reserved=1), "reserved"),
])
def test_hamming_refuses_bad_arguments_without_a_device(kw, word):
    rc, msg, cnt, _, _ = _hamming(**kw)
    assert rc == _lib.VO_ERR_ARG and word in msg, (rc, msg)
    assert cnt == -7


def test_hamming_with_an_empty_side_touches_nothing():
    rc, _, cnt, _, _ = _hamming(n0=0, des0=None)
    assert rc == _lib.VO_OK and cnt == 0
    rc, _, cnt, kidx, kdist = _hamming(n1=0, des1=None, knn=True)
    assert rc == _lib.VO_OK and cnt == 0
    assert (kidx[:5] == -1).all() and (kdist[:5] == np.iinfo(np.int32).max).all() and not kidx[5:].any()
    # a good call gets as far as the context
    rc, msg, _, _, _ = _hamming()
    assert rc == _lib.VO_ERR_ARG and "null vo_ctx" in msg


def test_python_wrapper_checks_shapes_and_types_before_the_library():
    with pytest.raises(ValueError, match="widths differ"):
        matcher.match_hamming(np.zeros((0, 8), np.uint32), np.zeros((3, 4), np.uint32))
    with pytest.raises(ValueError, match="1..16"):
        matcher.match_hamming(np.zeros((0, 17), np.uint32), np.zeros((3, 17), np.uint32))
    with pytest.raises(ValueError, match="multiple of 4"):
        matcher.match_hamming(np.zeros((2, 30), np.uint8), np.zeros((3, 30), np.uint8))
    with pytest.raises(ValueError, match="uint32, int32 or uint8"):
        matcher.match_hamming(np.zeros((2, 8), np.float32), np.zeros((3, 8), np.float32))
    u = brief.unpack(np.array([[1, 1 << 31], [0xffffffff, 0]], np.uint32))
    assert u.shape == (2, 64) and u.dtype == np.float32
    assert u[0].nonzero()[0].tolist() == [0, 63] and u[1].nonzero()[0].tolist() == list(range(32))
