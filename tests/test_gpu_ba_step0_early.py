"""The fused solve launch's prologue at its edge shapes, and the six-chunk K1's priority slicing.

In a fused launch (K2's reducers inside the banded solver's launch, full layout) the prologue
columns are dealt to the eight waves and polled column by column.  The split launches (K2 on its
own, ``ba_split_reduce``) load them in one sweep behind a kernel boundary: an independent
reference with the same operations in the same order, so every comparison is exact.  The windows
are the edges of that dealing (one-sided, bandwidth 7 and 9, a side of fewer rows than w + 2);
they were chosen for a variant that factored step 0 before the prologue's barrier, which was
measured and not kept, and stay as the yardstick for the next attempt.

In K1 the waves of chunks 4 and 5 of a six-chunk segment hold raised priority until their
elimination is done, and the combine stores its slab rows write-through.  Neither changes an
operation: the results must stay what the build before computed
(tests/golden/ba_step_ends_parent.npz).
"""

import importlib.util
from pathlib import Path

import numpy as np
import pytest

from visualodometry_amd import _lib
from visualodometry_amd.ba import BASession, poses_to_rt, rt_to_poses
from visualodometry_amd.synthetic import make_ba_problem

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
_spec = importlib.util.spec_from_file_location("make_ba_step_ends", GOLDEN / "make_ba_step_ends.py")
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

# (n_poses, max_track, n_fixed): one-sided w = 1; a small two-sided window; F = 16, the first
# two-sided w = 7 window; w = 9, the widest dealing of prologue columns; one and two fixed poses
WINDOWS = [(4, 2, 2), (12, 3, 2), (18, 8, 2), (40, 10, 2), (50, 8, 1), (50, 8, 2)]
SMALL = (12, 3, 2)  # the failure paths' window


def _window(n_poses, max_track, n_fixed):
    return make_ba_problem(n_poses, 40 * n_poses, 31 + n_poses, max_track=max_track, n_fixed=n_fixed)


def _session(p, ctx, lam=1.0, cam=None):
    s = BASession(p.K, p.point_ptr, p.obs_cam if cam is None else cam, p.obs_uv, p.n_poses, p.n_fixed, lam, ctx)
    s.set_state(p.poses_cw, p.points)
    return s


def _run(ctx, p, split, iters=3):
    """``iters`` GN iterations with K2 fused (default) or launched on its own: results, kernel names."""
    _lib.ba_split_reduce(ctx, split)
    try:
        _lib.profile_enable(ctx, True)
        s = _session(p, ctx)
        st = s.plan_stats()
        rc, costs = s.run(iters)
        P, X = s.get_state()
        prof = _lib.profile_read(ctx)
        _lib.profile_enable(ctx, False)
    finally:
        _lib.ba_split_reduce(ctx, False)
    return st, rc, (costs, P, X), prof


@pytest.mark.parametrize("n_poses,max_track,n_fixed", WINDOWS)
def test_fused_prologue_equals_split_launches(ctx, n_poses, max_track, n_fixed):
    """Three GN iterations, fused against split launches: costs, poses and landmarks."""
    p = _window(n_poses, max_track, n_fixed)
    out = []
    for split in (False, True):
        st, rc, res, prof = _run(ctx, p, split)
        assert st["band_solver"] == 1 and st["band_mode"] == "full", st
        assert rc == _lib.VO_OK and np.all(np.isfinite(res[0]))
        assert ("ba_reduce" in prof) == split  # the default run is the fused launch
        out.append(res)
    assert not np.array_equal(out[0][1], rt_to_poses(poses_to_rt(p.poses_cw)))  # the poses moved
    for a, b in zip(out[0], out[1]):
        np.testing.assert_array_equal(a, b)


def test_windows_cover_the_dealing():
    """The windows above keep their shapes (host planner): a one-sided window, two-sided windows
    of bandwidth 7 and 9 (the widest: twenty-two prologue columns), a side of fewer rows than
    w + 2, an odd and an even count of free poses."""
    from visualodometry_amd.ba import plan_probe

    shapes = []
    for n_poses, max_track, n_fixed in WINDOWS:
        p = _window(n_poses, max_track, n_fixed)
        pr = plan_probe(p.K, p.point_ptr, p.obs_cam, p.obs_uv, p.n_poses, p.n_fixed, 1024)
        assert pr["band_solver"] == 1
        shapes.append((pr["band_top_rows"], pr["band_separator_rows"], pr["band_bottom_rows"]))
    assert shapes[0][1:] == (0, 0)  # one-sided
    seps = [s for _, s, _ in shapes]
    assert 7 in seps and 9 in seps  # the separator has w rows
    assert any(s == 7 and nb < s + 2 for _, s, nb in shapes)  # fewer bottom rows than w + 2
    assert {(m + s + nb) % 2 for m, s, nb in shapes} == {0, 1}


def test_not_spd_in_fused_launch(ctx):
    """A solve that is not SPD (a free camera without observations, no damping) in the fused
    launch: the status, dc == 0 and the poses kept; then a good window on the same context."""
    p = _window(*SMALL)
    cam = p.obs_cam.copy()
    last = p.n_poses - 1
    cam[cam == last] = last - 1
    s = _session(p, ctx, lam=0.0, cam=cam)
    assert s.plan_stats()["band_mode"] == "full"
    rc, _, _, dc, _ = s.gn_step()
    assert rc == _lib.VO_ERR_NOT_SPD
    np.testing.assert_array_equal(dc, np.zeros_like(dc))
    P, _ = s.get_state()
    np.testing.assert_array_equal(P, rt_to_poses(poses_to_rt(p.poses_cw)))
    # three launches, the last two behind the failed one (prior status set): the state stays at
    # the failed iteration's linearisation point
    s.set_state(p.poses_cw, p.points)
    assert s.run(3)[0] == _lib.VO_ERR_NOT_SPD
    P2, X2 = s.get_state()
    np.testing.assert_array_equal(P2, P)
    np.testing.assert_array_equal(X2, p.points)
    good = _window(*SMALL)
    a, b = _run(ctx, good, False)[2], _run(ctx, good, True)[2]
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_dropped_reducer_times_out_and_recovers(ctx):
    """One reducer workgroup left out of every launch: some wave's poll times out.  The run fails
    naming the timeout, the state stays at the failed iteration's linearisation point, and the
    next window on the context is exact again."""
    p = _window(*SMALL)
    s = _session(p, ctx)
    assert s.plan_stats()["band_mode"] == "full"
    _lib.ba_testing_drop_reducers(ctx, 1)
    try:
        with pytest.raises(_lib.VoError, match="timed out"):
            s.run(2)
    finally:
        _lib.ba_testing_drop_reducers(ctx, 0)
    P, X = s.get_state()
    np.testing.assert_array_equal(P, rt_to_poses(poses_to_rt(p.poses_cw)))
    np.testing.assert_array_equal(X, p.points)
    a, b = _run(ctx, p, False)[2], _run(ctx, p, True)[2]
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN / "ba_step_ends_parent.npz"))


@pytest.mark.parametrize("variant", [0, 5])
def test_k1_priority_slicing_equals_parent(ctx, golden, variant):
    """The default six-chunk K1 (waves 4 and 5 at raised priority) and the five-chunk one (wave 4
    only), both with write-through slab rows, on the K1 window, three iterations, against the
    parent build's recorded results."""
    st, got = gen.run_k1(ctx, variant)
    want = variant if variant else 6
    assert st["seg_obs"] == 1 and st["chunks"] == want * st["segments"], st
    assert got["rc"] == _lib.VO_OK and np.all(np.isfinite(got["costs"]))
    for k, a in gen.record(got, gen.K1_FULL).items():
        ref = golden[f"k1_{variant}_{k}"]
        if np.asarray(a).dtype.kind == "U":
            assert str(a) == str(ref), f"k1_{variant} {k}"
        else:
            np.testing.assert_array_equal(a, ref, err_msg=f"k1_{variant} {k}")
