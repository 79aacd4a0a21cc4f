"""GPU parity of the SIFT selection stage alone (``sift_keys_kernel``, the batch-wide sort and
``sift_select_kernel``, through the test entry ``vo_sift_testing_select``) against
``oracle/sift_ref.select_keypoints`` on caller-made records (tests/sift_select_cases.py).

Real images produce almost only equal-(x, y) runs of one or two records and untied responses, so
the image tests (tests/test_gpu_sift.py) never reach the register sort of runs of 3..8, the
insertion sort of longer ones, the rescan when more than 2048 long runs are queued, duplicates
inside such runs, ties at the retainBest threshold or most edges of the radix select; these cases
do.  Every comparison is exact: per image the kept count equals the reference's, the selected
record indices are distinct and lie in the image's filled slots, and the six fields of the
selected records equal the reference survivors' bit for bit, in order (records, not indices:
which of several records identical in all six fields stays cannot be observed in the product).
"""

import ctypes as C

import numpy as np
import pytest

from tests import sift_select_cases as G
from visualodometry_amd import _lib, sift

pytestmark = pytest.mark.gpu


def _check(name, okp, counts, cap_img, sel, sel_count):
    ref = G.reference(name)
    flat = okp.reshape(-1, 8)[:, :6].view(np.uint32)
    assert sel.shape == (len(counts), cap_img)
    for b in range(len(counts)):
        assert sel_count[b] == len(ref[b]), f"{name} image {b}: kept {sel_count[b]}, reference {len(ref[b])}"
        s = sel[b, :sel_count[b]].astype(np.int64)
        assert len(np.unique(s)) == len(s), f"{name} image {b}: a record selected twice"
        assert ((s >= b * cap_img) & (s < b * cap_img + counts[b])).all(), f"{name} image {b}: index outside its slots"
        np.testing.assert_array_equal(flat[s], flat[b * cap_img + ref[b]], err_msg=f"{name} image {b}")


@pytest.mark.parametrize("name", G.NAMES)
def test_select_matches_reference(ctx, name):
    okp, counts, nfeatures, cap_img = G.case(name)
    sel, sel_count = sift.select_records(okp, counts, nfeatures, ctx=ctx)
    _check(name, okp, counts, cap_img, sel, sel_count)


def test_overflow_reports_the_count(ctx):
    okp, counts, nfeatures, cap_img = G.overflow()
    _, sel_count = sift.select_records(okp, counts, nfeatures, ctx=ctx)
    assert sel_count[1] == -G.OVERFLOW_COUNTS[1]


def test_repeat_on_one_context(ctx):
    """The same call twice, with a larger one in between (the workspace grows and is reused)."""
    okp, counts, nfeatures, cap_img = G.case("dups_insertion")
    first = sift.select_records(okp, counts, nfeatures, ctx=ctx)
    big = G.case("long_queue_2100")
    _check("long_queue_2100", big[0], big[1], big[3], *sift.select_records(big[0], big[1], big[2], ctx=ctx))
    again = sift.select_records(okp, counts, nfeatures, ctx=ctx)
    _check("dups_insertion", okp, counts, cap_img, *again)
    np.testing.assert_array_equal(first[1], again[1])
    np.testing.assert_array_equal(first[0][0, :first[1][0]], again[0][0, :again[1][0]])


def test_arguments_are_validated(ctx):
    okp = np.zeros((1, 16, 8), np.float32)
    counts = np.zeros(1, np.int32)
    sel = np.zeros((1, 16), np.uint32)
    sc = np.zeros(1, np.int32)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    good = [ctx.handle, P(okp, C.c_float), P(counts, C.c_int32), 1, 16, 0, P(sel, C.c_uint32), P(sc, C.c_int32)]
    assert ctx.lib.vo_sift_testing_select(*good) == _lib.VO_OK and sc[0] == 0
    for pos, bad in ((0, None), (1, None), (2, None), (6, None), (7, None), (3, 0), (3, 257), (4, 0), (4, 131073), (5, -1)):
        args = list(good)
        args[pos] = bad
        assert ctx.lib.vo_sift_testing_select(*args) == _lib.VO_ERR_ARG, f"argument {pos} = {bad}"
    counts[0] = -1
    assert ctx.lib.vo_sift_testing_select(*good) == _lib.VO_ERR_ARG
