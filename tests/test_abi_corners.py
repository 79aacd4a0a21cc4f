"""The corner detector's C-ABI surface: declared, exported, bound, the options struct laid out as
the header's, and the arguments checked before any device (or context) is touched (no GPU)."""

import ctypes as C
import re

import numpy as np
import pytest

from visualodometry_amd import _lib

IMG = np.zeros((40, 48), np.uint8)
KEEP = np.full((4, 2), 20.0, np.float32)
XY = np.array([[1, 2], [3, 4], [5, 6]], np.int32)
RESP = np.array([3.0, 2.0, 1.0], np.float32)


def _good(img=IMG, tag=0, h=40, w=48, keep=KEEP, n_keep=4, opt=True, corners=True, n_out=True, **fields):
    lib = _lib.load()
    o = dict(max_corners=100, block_radius=1, quality=0.01, min_distance=8.0, flags=0, reserved=0)
    o.update(fields)
    o = _lib.CornerOptionsC(**o)
    out = np.zeros((128, 2), np.float32)
    resp = np.zeros(128, np.float32)
    n = C.c_int32(-7)
    rc = lib.vo_good_features(None, None if img is None else img.ctypes.data, tag, h, w, None,
                              None if keep is None else keep.ctypes.data, n_keep, C.byref(o) if opt else None,
                              out.ctypes.data if corners else None, resp.ctypes.data, C.byref(n) if n_out else None)
    return rc, lib.vo_last_error().decode(), n.value


def _select(xy=XY, resp=RESP, n=3, keep=None, n_keep=0, d=2.0, max_corners=3, out=True, n_out=True):
    lib = _lib.load()
    idx = np.zeros(8, np.int32)
    got = C.c_int32(-7)
    rc = lib.vo_corner_select(None, None if xy is None else xy.ctypes.data, None if resp is None else resp.ctypes.data,
                              n, None if keep is None else keep.ctypes.data, n_keep, d, max_corners,
                              idx.ctypes.data if out else None, C.byref(got) if n_out else None)
    return rc, lib.vo_last_error().decode(), got.value


def test_header_declares_the_functions_and_the_options():
    code = re.sub(r"/\*.*?\*/", "", _lib.HEADER.read_text(), flags=re.S)
    for fn in ("vo_good_features", "vo_corner_response", "vo_corner_select"):
        assert re.search(rf"\bint\s+{fn}\s*\(", code), fn
        assert fn in _lib.SIGNATURES and hasattr(_lib.load(), fn)
    body = code.split("vo_corner_options")[0].rsplit("typedef struct", 1)[1]
    names = re.findall(r"\b(max_corners|block_radius|quality|min_distance|flags|reserved)\b", body)
    assert names == [n for n, _ in _lib.CornerOptionsC._fields_]
    assert C.sizeof(_lib.CornerOptionsC) == 24
    assert [getattr(_lib.CornerOptionsC, n).offset for n in names] == list(range(0, 24, 4))
    assert "§Corners" in _lib.HEADER.read_text()


def test_the_versions_and_the_profiler_table_stay():
    text = _lib.HEADER.read_text()
    assert _lib.load().vo_abi_version() == 1
    assert re.search(r"#define\s+VO_ABI_VERSION\s+1\b", text)
    assert re.search(r"#define\s+VO_PROFILE_KERNELS\s+25\b", text)
    assert len(_lib.KERNEL_NAMES) == 25


@pytest.mark.parametrize("kw, word", [
    (dict(opt=False), "null options or outputs"),
    (dict(corners=False), "null options or outputs"),
    (dict(n_out=False), "null options or outputs"),
    (dict(keep=None), "null keep"),
    (dict(n_keep=-1), "bad shape"),
    (dict(h=0), "bad shape"),
    (dict(w=-3), "bad shape"),
    (dict(h=1 << 16, w=1 << 15), "bad shape"),
    (dict(img=None), "null image with tag 0"),
    (dict(max_corners=0), "max_corners"),
    (dict(max_corners=40 * 48 + 1), "max_corners"),
    (dict(block_radius=0), "block_radius"),
    (dict(block_radius=4), "block_radius"),
    (dict(quality=0.0), "quality"),
    (dict(quality=-0.5), "quality"),
    (dict(quality=1.5), "quality"),
    (dict(quality=float("nan")), "quality"),
    (dict(quality=float("inf")), "quality"),
    (dict(min_distance=-1.0), "min_distance"),
    (dict(min_distance=1024.5), "min_distance"),
    (dict(min_distance=float("nan")), "min_distance"),
    (dict(min_distance=float("inf")), "min_distance"),
    (dict(flags=1), "unknown flags"),
    (dict(flags=-1), "unknown flags"),
    (dict(reserved=2), "reserved"),
])
def test_bad_arguments_are_refused_before_the_context_is_touched(kw, word):
    rc, msg, _ = _good(**kw)
    assert rc == _lib.VO_ERR_ARG
    assert msg.startswith("vo_good_features:") and word in msg and "vo_ctx" not in msg


def test_good_arguments_get_as_far_as_the_context():
    for kw in (dict(), dict(img=None, tag=9), dict(keep=None, n_keep=0), dict(block_radius=3, quality=1.0),
               dict(min_distance=0.0), dict(min_distance=1024.0, max_corners=40 * 48)):
        rc, msg, _ = _good(**kw)
        assert rc == _lib.VO_ERR_ARG and "null vo_ctx" in msg


def test_an_image_without_interior_is_ok_without_a_device():
    for h, w in ((2, 48), (40, 2), (1, 1)):
        rc, _, n = _good(h=h, w=w, max_corners=1)
        assert rc == _lib.VO_OK and n == 0


@pytest.mark.parametrize("kw, word", [
    (dict(out=False), "null outputs"),
    (dict(n_out=False), "null outputs"),
    (dict(n=-1), "negative count"),
    (dict(n_keep=-2), "negative count"),
    (dict(xy=None), "null candidates"),
    (dict(resp=None), "null candidates"),
    (dict(n_keep=2), "null keep"),
    (dict(d=-0.5), "min_distance"),
    (dict(d=float("nan")), "min_distance"),
    (dict(d=float("inf")), "min_distance"),
    (dict(max_corners=0), "max_corners"),
    (dict(resp=np.array([1.0, np.nan, 0.0], np.float32)), "not finite"),
    (dict(resp=np.array([np.inf, 1.0, 0.0], np.float32)), "not finite"),
    (dict(xy=np.array([[0, 0], [1 << 25, 0], [0, 0]], np.int32)), "coordinates"),
])
def test_select_refuses_bad_arguments_before_the_context(kw, word):
    rc, msg, _ = _select(**kw)
    assert rc == _lib.VO_ERR_ARG
    assert msg.startswith("vo_corner_select:") and word in msg and "vo_ctx" not in msg


def test_select_gets_as_far_as_the_context_and_nothing_is_ok():
    rc, msg, _ = _select()
    assert rc == _lib.VO_ERR_ARG and "null vo_ctx" in msg
    rc, msg, _ = _select(keep=KEEP, n_keep=4, d=0.0)
    assert rc == _lib.VO_ERR_ARG and "null vo_ctx" in msg
    rc, _, n = _select(n=0, xy=None, resp=None)
    assert rc == _lib.VO_OK and n == 0


def test_response_refuses_bad_arguments():
    lib = _lib.load()
    out = np.zeros(IMG.shape, np.float32)
    for args in ((None, 40, 48, 1, out.ctypes.data), (IMG.ctypes.data, 40, 48, 1, None),
                 (IMG.ctypes.data, 0, 48, 1, out.ctypes.data), (IMG.ctypes.data, 40, 48, 0, out.ctypes.data),
                 (IMG.ctypes.data, 40, 48, 4, out.ctypes.data)):
        assert lib.vo_corner_response(None, *args) == _lib.VO_ERR_ARG
        msg = lib.vo_last_error().decode()
        assert msg.startswith("vo_corner_response:") and "vo_ctx" not in msg
    assert lib.vo_corner_response(None, IMG.ctypes.data, 40, 48, 2, out.ctypes.data) == _lib.VO_ERR_ARG
    assert "null vo_ctx" in lib.vo_last_error().decode()


def test_python_wrapper_checks_before_the_library():
    from visualodometry_amd import corners

    class NoCtx:  # a context whose library must not be reached
        device = 0

    with pytest.raises(ValueError, match="2-D uint8"):
        corners.good_features(IMG.astype(np.float32), 10, ctx=NoCtx())
    with pytest.raises(ValueError, match="block_size"):
        corners.good_features(IMG, 10, block_size=4, ctx=NoCtx())
    with pytest.raises(ValueError, match="mask must be uint8"):
        corners.good_features(IMG, 10, mask=np.zeros((3, 3), np.uint8), ctx=NoCtx())
    with pytest.raises(ValueError, match=r"keep must be \(N, 2\)"):
        corners.good_features(IMG, 10, keep=np.zeros((4, 3)), ctx=NoCtx())
    with pytest.raises(ValueError, match="None without a tag"):
        corners.good_features(None, 10, ctx=NoCtx())
    with pytest.raises(ValueError, match="resp has 2 rows"):
        corners.select(XY, RESP[:2], 2.0, ctx=NoCtx())
    with pytest.raises(ValueError, match="Harris"):
        corners.goodFeaturesToTrack(IMG, 10, 0.01, 8, useHarrisDetector=True, ctx=NoCtx())
    for bs in (4, 1, 9):
        with pytest.raises(ValueError, match="blockSize"):
            corners.goodFeaturesToTrack(IMG, 10, 0.01, 8, blockSize=bs, ctx=NoCtx())
    assert "not its bits" in corners.goodFeaturesToTrack.__doc__
