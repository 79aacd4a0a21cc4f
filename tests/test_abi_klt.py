"""The KLT entry points' C-ABI surface: declared, exported, bound, the options struct laid out as
the header's, the arguments checked before any device (or context) is touched, and
``vo_klt_layout`` against the restatement's level sizes (no GPU)."""

import ctypes as C
import re

import numpy as np
import pytest

from tests import klt_ref as R
from visualodometry_amd import _lib

IMG = np.zeros((40, 48), np.uint8)
PTS = np.full((4, 2), 20.0, np.float32)


def _call(img0=IMG, img1=IMG, tag0=0, tag1=0, h=40, w=48, pts0=PTS, pts1=True, n=4, status=True, opt=True, **fields):
    lib = _lib.load()
    o = dict(win_radius=10, levels=4, max_iters=30, eps=0.01, min_eig=1e-4, fb_thresh=1.0, max_err=0.0, flags=0,
             reserved=0)
    o.update(fields)
    o = _lib.KltOptionsC(**o)
    out = np.zeros((max(n, 1), 2), np.float32)
    st = np.zeros(max(n, 1), np.uint8)
    err = np.zeros(max(n, 1), np.float32)
    good = C.c_int32(-7)
    rc = lib.vo_klt_track(None, None if img0 is None else img0.ctypes.data, tag0,
                          None if img1 is None else img1.ctypes.data, tag1, h, w,
                          None if pts0 is None else pts0.ctypes.data, out.ctypes.data if pts1 else None, n,
                          C.byref(o) if opt else None, st.ctypes.data if status else None, err.ctypes.data,
                          C.byref(good))
    return rc, lib.vo_last_error().decode(), good.value


def test_header_declares_the_functions_the_flags_and_the_options():
    code = re.sub(r"/\*.*?\*/", "", _lib.HEADER.read_text(), flags=re.S)
    for fn in ("vo_klt_track", "vo_klt_pyramid", "vo_klt_layout"):
        assert re.search(rf"\bint\s+{fn}\s*\(", code), fn
        assert fn in _lib.SIGNATURES and hasattr(_lib.load(), fn)
    assert re.search(r"#define\s+VO_KLT_GUESS\s+1\b", code) and _lib.VO_KLT_GUESS == 1
    assert re.search(r"#define\s+VO_KLT_FB\s+2\b", code) and _lib.VO_KLT_FB == 2
    body = code.split("vo_klt_options")[0].rsplit("typedef struct", 1)[1]
    names = re.findall(r"\b(win_radius|levels|max_iters|eps|min_eig|fb_thresh|max_err|flags|reserved)\b", body)
    assert names == [n for n, _ in _lib.KltOptionsC._fields_]
    assert C.sizeof(_lib.KltOptionsC) == 36
    assert [getattr(_lib.KltOptionsC, n).offset for n in names] == list(range(0, 36, 4))


def test_the_versions_and_the_profiler_table_stay():
    text = _lib.HEADER.read_text()
    assert _lib.load().vo_abi_version() == 1
    assert re.search(r"#define\s+VO_ABI_VERSION\s+1\b", text)
    assert re.search(r"#define\s+VO_PROFILE_KERNELS\s+25\b", text)
    assert len(_lib.KERNEL_NAMES) == 25


@pytest.mark.parametrize("kw, word", [
    (dict(opt=False), "null options or outputs"),
    (dict(pts1=False), "null options or outputs"),
    (dict(status=False), "null options or outputs"),
    (dict(n=-1), "bad shape"),
    (dict(h=-40), "bad shape"),
    (dict(w=-1), "bad shape"),
    (dict(h=0), "bad shape"),
    (dict(pts0=None), "null pts0"),
    (dict(img0=None), "null image with tag 0"),
    (dict(img1=None), "null image with tag 0"),
    (dict(img1=None, tag0=5), "null image with tag 0"),
    (dict(win_radius=0), "win_radius"),
    (dict(win_radius=16), "win_radius"),
    (dict(levels=0), "levels"),
    (dict(levels=9), "levels"),
    (dict(max_iters=0), "max_iters"),
    (dict(max_iters=101), "max_iters"),
    (dict(eps=float("nan")), "eps"),
    (dict(eps=-0.01), "eps"),
    (dict(min_eig=float("inf")), "min_eig"),
    (dict(min_eig=-1.0), "min_eig"),
    (dict(fb_thresh=float("nan")), "fb_thresh"),
    (dict(fb_thresh=-1.0), "fb_thresh"),
    (dict(max_err=float("inf")), "max_err"),
    (dict(max_err=-2.0), "max_err"),
    (dict(flags=4), "unknown flags"),
    (dict(flags=-1), "unknown flags"),
    (dict(reserved=1), "reserved"),
])
def test_bad_arguments_are_refused_before_the_context_is_touched(kw, word):
    rc, msg, _ = _call(**kw)
    assert rc == _lib.VO_ERR_ARG
    assert msg.startswith("vo_klt_track:") and word in msg and "vo_ctx" not in msg


def test_good_arguments_get_as_far_as_the_context():
    for kw in (dict(), dict(flags=3), dict(img0=None, tag0=9), dict(img0=None, tag0=9, img1=None, tag1=10),
               dict(win_radius=15, levels=8, max_iters=100, max_err=3.0)):
        rc, msg, _ = _call(**kw)
        assert rc == _lib.VO_ERR_ARG and "null vo_ctx" in msg


def test_no_points_is_ok_without_a_device():
    rc, _, good = _call(n=0, pts0=None)
    assert rc == _lib.VO_OK and good == 0


@pytest.mark.parametrize("h, w", [(163, 241), (160, 240), (376, 1241), (22, 40), (1, 1), (47, 46)])
@pytest.mark.parametrize("r", [1, 7, 10, 15])
def test_layout_matches_the_restatement(h, w, r):
    from visualodometry_amd import klt

    for levels in (1, 3, 8):
        sizes = R.level_sizes(h, w, levels, r)
        L, nbytes, lv = klt.layout(h, w, levels, r)
        assert L == len(sizes) and [(a, b) for a, b, _ in lv] == sizes
        offs = np.concatenate([[0], np.cumsum([a * b for a, b in sizes])])
        assert [o for _, _, o in lv] == offs[:-1].tolist() and nbytes == offs[-1]


def test_layout_refuses_bad_arguments_and_writes_no_more_than_asked():
    lib = _lib.load()
    out = np.full(8, -1, np.int64)
    p = out.ctypes.data_as(C.POINTER(C.c_int64))
    for args in ((0, 10, 3, 5), (10, 0, 3, 5), (10, 10, 0, 5), (10, 10, 9, 5), (10, 10, 3, -1), (10, 10, 3, 16)):
        assert lib.vo_klt_layout(*args, p, 8) == _lib.VO_ERR_ARG
        assert lib.vo_last_error().decode().startswith("vo_klt_layout:")
    assert lib.vo_klt_layout(163, 241, 8, 10, p, 3) == 2 + 3 * 3  # the count it has, three values written
    assert out.tolist() == [3, 163 * 241 + 82 * 121 + 41 * 61, 163, -1, -1, -1, -1, -1]


def test_python_wrapper_checks_shapes_before_the_library():
    from visualodometry_amd import klt

    class NoCtx:  # a context whose library must not be reached
        device = 0

    with pytest.raises(ValueError, match="2-D uint8"):
        klt.track(IMG.astype(np.float32), IMG, PTS, ctx=NoCtx())
    with pytest.raises(ValueError, match="differ in shape"):
        klt.track(IMG, IMG[:-1], PTS, ctx=NoCtx())
    with pytest.raises(ValueError, match=r"pts0 must be \(N, 2\)"):
        klt.track(IMG, IMG, np.zeros((4, 3)), ctx=NoCtx())
    with pytest.raises(ValueError, match="guess has 3 rows"):
        klt.track(IMG, IMG, PTS, guess=PTS[:3], ctx=NoCtx())
    with pytest.raises(ValueError, match="None without a tag"):
        klt.track(None, IMG, PTS, ctx=NoCtx())
    with pytest.raises(ValueError, match="winSize"):
        klt.calcOpticalFlowPyrLK(IMG, IMG, PTS, winSize=(21, 15), ctx=NoCtx())
    assert "not its bits" in klt.calcOpticalFlowPyrLK.__doc__
