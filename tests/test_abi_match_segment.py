"""vo_match_segment's C-ABI surface: declared, exported, bound, its options struct laid out as the
header's, and its arguments checked before any device (or context) is touched (no GPU)."""

import ctypes as C
import re

import numpy as np
import pytest

from visualodometry_amd import _lib

F = np.ones((4, 8), np.float32)
XY = np.zeros((4, 2), np.float32)
SEG = np.zeros((4, 4), np.float32)


def _call(n0=4, n1=4, dim=8, des0=F, des1=F, seg=SEG, kp1=XY, radius=None, ratio=0.8, max_dist=0.0, flags=0,
          reserved=0, opt=True, pairs=True, count=True):
    lib = _lib.load()
    o = _lib.MatchSegmentOptionsC(seg=seg.ctypes.data if seg is not None else None,
                                  radius=radius.ctypes.data if radius is not None else None,
                                  kp1=kp1.ctypes.data if kp1 is not None else None, radius0=5.0, width=64, height=64,
                                  ratio=ratio, max_dist=max_dist, flags=flags, reserved=reserved)
    out = np.zeros((max(n0, 1), 2), np.int32)
    cnt = np.zeros(1, np.int32)
    rc = lib.vo_match_segment(None, C.c_void_p(des0.ctypes.data if des0 is not None else None), n0,
                              C.c_void_p(des1.ctypes.data if des1 is not None else None), n1, dim,
                              C.byref(o) if opt else None, _lib.ptr(out, C.c_int32) if pairs else None, None,
                              _lib.ptr(cnt, C.c_int32) if count else None)
    return rc, lib.vo_last_error().decode()


def _header_struct():
    code = re.sub(r"/\*.*?\*/", "", _lib.HEADER.read_text(), flags=re.S)
    return code, code.split("vo_match_segment_options")[0].rsplit("typedef struct", 1)[1]


def test_header_declares_the_function_and_the_options():
    code, body = _header_struct()
    assert re.search(r"\bint\s+vo_match_segment\s*\(", code)
    assert "vo_match_segment_options" in code
    for field in ("seg", "radius", "radius0", "kp1", "width", "height", "ratio", "max_dist", "flags", "reserved"):
        assert re.search(rf"\b{field}\b", body), field


def test_lib_exports_and_binds_it_and_the_versions_stay():
    lib = _lib.load()
    assert "vo_match_segment" in _lib.SIGNATURES and hasattr(lib, "vo_match_segment")
    assert lib.vo_abi_version() == 1
    text = _lib.HEADER.read_text()
    assert re.search(r"#define\s+VO_ABI_VERSION\s+1\b", text)
    assert re.search(r"#define\s+VO_PROFILE_KERNELS\s+25\b", text)
    assert len(_lib.KERNEL_NAMES) == 25


def test_options_struct_matches_the_header_layout():
    """The header's fields in order, with C's natural alignment, against the ctypes structure."""
    _, body = _header_struct()
    sizes = {"const float*": 8, "float": 4, "int32_t": 4, "double": 8}
    fields = []
    for decl in body.strip(" {}\n").split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const float\*|float|int32_t|double)\s+(.*)$", decl)
        assert m, decl
        fields += [(name.strip(), sizes[m.group(1)]) for name in m.group(2).split(",")]
    assert [n for n, _ in fields] == ["seg", "radius", "kp1", "radius0", "width", "height", "ratio", "max_dist", "flags",
                                      "reserved"]
    off = 0
    o = _lib.MatchSegmentOptionsC
    assert [n for n, _ in o._fields_] == [n for n, _ in fields]
    for name, size in fields:
        off = (off + size - 1) // size * size
        assert getattr(o, name).offset == off and getattr(o, name).size == size, name
        off += size
    assert C.sizeof(o) == (off + 7) // 8 * 8 == 64
    # the same layout as vo_match_gate_options, seg in pred's place
    g = _lib.MatchGateOptionsC
    assert [(getattr(g, n).offset, getattr(g, n).size) for n, _ in g._fields_] == \
        [(getattr(o, n).offset, getattr(o, n).size) for n, _ in o._fields_]


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
    (dict(max_dist=float("nan")), "max_dist"),
    (dict(max_dist=-1.0), "max_dist"),
    (dict(des0=None), "null array"),
    (dict(seg=None), "null array"),
    (dict(des1=None), "null array"),
    (dict(kp1=None), "null array"),
])
def test_bad_arguments_are_refused_before_the_context_is_touched(kw, word):
    rc, msg = _call(**kw)
    assert rc == _lib.VO_ERR_ARG
    assert msg.startswith("vo_match_segment:") and word in msg and "vo_ctx" not in msg


def test_good_arguments_get_as_far_as_the_context():
    for kw in (dict(), dict(flags=3), dict(n0=0, des0=None, seg=None), dict(n1=0, des1=None, kp1=None),
               dict(radius=np.ones(4, np.float32), max_dist=2.0)):
        rc, msg = _call(**kw)
        assert rc == _lib.VO_ERR_ARG and "null vo_ctx" in msg


def test_python_wrapper_checks_shapes_before_the_library():
    from visualodometry_amd import matcher

    class NoCtx:  # a context whose library must not be reached
        device = 0
        _foreign_tensors = True

    with pytest.raises(ValueError, match=r"seg must be \(N, 4\)"):
        matcher.match_segment(F, XY, 3.0, F, XY, ctx=NoCtx())
    with pytest.raises(ValueError, match="seg has 3 rows"):
        matcher.match_segment(F, SEG[:3], 3.0, F, XY, ctx=NoCtx())
    with pytest.raises(ValueError, match="radius has 2 entries"):
        matcher.match_segment(F, SEG, np.ones(2), F, XY, ctx=NoCtx())
    with pytest.raises(ValueError, match="kp1 must be"):
        matcher.match_segment(F, SEG, 3.0, F, XY[:3], ctx=NoCtx())
    e = np.zeros((0, 8), np.float32)
    pairs, dist = matcher.match_segment(e, np.zeros((0, 4)), 3.0, F, XY, return_dist=True, ctx=NoCtx())
    assert pairs.shape == (0, 2) and pairs.dtype == np.int64 and dist.shape == (0,) and dist.dtype == np.float32
    assert matcher.match_segment(F, SEG, 3.0, e, np.zeros((0, 2)), ctx=NoCtx()).shape == (0, 2)
