"""The two ends of a GN step against the parent build's own results, bit for bit.

K1's cross-chunk combine (ba_lin_wave_kernel, segments of several chunks) is started by the waves
of chunks 0..3 before the segment's barrier and finished with chunks 4/5 after it; the banded
solver's tail leaves the update in LDS and every thread stores contiguous 16-byte pieces of
pose_next and dc; the G blocks of the bottom side's pseudo rows are formed under the
separator's back substitution.  None of this changes a floating-point operation or its order,
so the reference is what the commit before computed (tests/golden/ba_step_ends_parent.npz,
recorded by tests/golden/make_ba_step_ends.py from that build) and every comparison is exact.
"""

import importlib.util
from pathlib import Path

import numpy as np
import pytest

from visualodometry_amd import _lib

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
_spec = importlib.util.spec_from_file_location("make_ba_step_ends", GOLDEN / "make_ba_step_ends.py")
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(GOLDEN / "ba_step_ends_parent.npz"))
    assert len(str(g["parent"])) >= 7  # the commit the reference build was made from
    assert g["k1_window"].tolist() == [gen.K1_WINDOW[k] for k in ("n_poses", "n_points", "seed")]
    return g


def _same(got: dict, g: dict, prefix: str):
    for k, a in got.items():
        ref = g[f"{prefix}_{k}"]
        if np.asarray(a).dtype.kind == "U":
            assert str(a) == str(ref), f"{prefix} {k}"
        else:
            np.testing.assert_array_equal(a, ref, err_msg=f"{prefix} {k}")


def test_k1_window_has_every_combine_case():
    """The host planner's six-chunk plan of the K1 window keeps all four cases of the combine (a
    planner change must not silently empty the tests below): a segment with fewer than four
    non-empty chunks, one with a slot held only by chunks 4/5 (nothing summed before the
    barrier), one with a slot held only by chunks 0..3, one with all six chunks non-empty."""
    segs, (short, late_only, early_only, full) = gen.combine_cases(gen.k1_window(), 6)
    assert segs > 1 and short > 0 and late_only > 0 and early_only > 0 and full > 0, (segs, short, late_only,
                                                                                      early_only, full)


@pytest.mark.parametrize("variant", gen.K1_VARIANTS)
def test_k1_variants_equal_parent(ctx, golden, variant):
    """Every one-wave K1 (vo_ba_testing_k1 1..6 chunks per segment, and the default): costs, poses
    and landmarks after three GN iterations."""
    st, got = gen.run_k1(ctx, variant)
    want = variant if variant else 6  # the default plan of a one-round window: six chunks
    assert st["seg_obs"] == 1 and st["chunks"] == want * st["segments"], st
    if want == 6:  # the plan the host check above walked
        assert st["segments"] == gen.combine_cases(gen.k1_window(), 6)[0]
    assert got["rc"] == _lib.VO_OK and np.all(np.isfinite(got["costs"]))
    _same(gen.record(got, gen.K1_FULL), golden, f"k1_{variant}")


@pytest.mark.parametrize("name,n_poses,max_track,n_fixed,mode", gen.TAIL_CASES)
def test_tail_equals_parent(ctx, golden, name, n_poses, max_track, n_fixed, mode):
    """The solver's tail on the full, split and ring layouts, one and two fixed poses, pose counts
    off a multiple of 16: dc and the poses of one exported step, then two more iterations."""
    st, got = gen.run_tail(ctx, n_poses, max_track, n_fixed)
    assert st["band_mode"] == mode, st
    assert got["rc"] == _lib.VO_OK and got["rc2"] == _lib.VO_OK
    assert np.abs(got["dc"]).max() > 0 and not np.array_equal(got["poses1"], got["poses"])
    _same(gen.record(got), golden, f"tail_{name}")


def test_failed_solve_keeps_poses(ctx, golden):
    """A solve that is not SPD: pose_next is pose_cur and dc is zero."""
    from visualodometry_amd.ba import poses_to_rt, rt_to_poses

    got = gen.run_not_spd(ctx)
    p, _ = gen.not_spd_window()
    assert got["rc"] == _lib.VO_ERR_NOT_SPD
    np.testing.assert_array_equal(got["dc"], np.zeros_like(got["dc"]))
    np.testing.assert_array_equal(got["poses"], rt_to_poses(poses_to_rt(p.poses_cw)))
    _same(gen.record(got, gen.NOTSPD_FULL), golden, "notspd")
