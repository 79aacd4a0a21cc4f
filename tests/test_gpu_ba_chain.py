"""The chained GN loop against the split sequence, bit for bit.

A run of two or more iterations enqueues one stand-alone K1, then solve launches that each carry
the NEXT iteration's K1 segments behind a pose gate (ba_band.hip, the chained instantiation of
ba_band_kernel; ba_lin_wave.h lin_wave_body), then one plain fused launch.  The gated K1 runs the
stand-alone K1's body; only where its loads sit in time and how pose_new / dc reach it differ.  So
the split sequence of the same build (``vo_ba_testing_no_chain``) is the reference and every
comparison is ``array_equal``.  (That the split sequence itself still computes the parent build's
bits is tests/test_gpu_ba_step_ends.py's and test_gpu_ba_step0_early.py's business; their runs of
two iterations on the full layout are chained now, too.)
"""

import importlib.util
import threading
from pathlib import Path

import numpy as np
import pytest

from visualodometry_amd import _lib
from visualodometry_amd.ba import BASession

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
_spec = importlib.util.spec_from_file_location("make_ba_step_ends", GOLDEN / "make_ba_step_ends.py")
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

HUBER = 1.5  # pixels: inside the K1 window's residual range, so both Huber branches are taken


def _session(p, ctx, lam=1.0, cam=None, huber=0.0):
    s = BASession(p.K, p.point_ptr, p.obs_cam if cam is None else cam, p.obs_uv, p.n_poses, p.n_fixed, lam, ctx)
    s.set_state(p.poses_cw, p.points)
    if huber > 0.0:
        s.set_robust(huber)
    return s


def _run(ctx, p, iters, chain, **kw):
    """A fresh session's run(iters): (rc, costs, poses, landmarks, chained, launches)."""
    _lib.ba_testing_no_chain(ctx, not chain)
    try:
        s = _session(p, ctx, **kw)
        rc, costs = s.run(iters)
        chained, launches = _lib.ba_testing_last_run(ctx)
        P, X = s.get_state()
    finally:
        _lib.ba_testing_no_chain(ctx, False)
    return rc, costs, P, X, chained, launches


def _equal(a, b, what=""):
    assert a[0] == b[0], what
    for x, y, name in zip(a[1:4], b[1:4], ("costs", "poses", "landmarks")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what} {name}")


_ref_cache = {}


def _k1_reference(ctx, iters, huber):
    """The split sequence's results on the K1 window, computed once per (iters, huber)."""
    key = (iters, huber)
    if key not in _ref_cache:
        r = _run(ctx, gen.k1_window(), iters, False, huber=huber)
        assert r[0] == _lib.VO_OK and not r[4] and r[5] == 2 * iters, r[4:]
        _ref_cache[key] = r
    return _ref_cache[key]


@pytest.mark.parametrize("huber", [0.0, HUBER], ids=["plain", "huber"])
@pytest.mark.parametrize("iters", [1, 2, 3, 5])
def test_k1_window_chained_equals_split(ctx, iters, huber):
    """The smallest window with every combine case (8 poses, 1300 landmarks, seed 3: 16 six-chunk
    segments), plain and Huber cost: costs, poses and landmarks after 1, 2, 3 and 5 iterations.
    Runs of two or more iterations are chained (k + 1 launches), a single iteration is not."""
    st = _session(gen.k1_window(), ctx).plan_stats()
    assert st["seg_obs"] == 1 and st["chunks"] == 6 * st["segments"] and st["band_mode"] == "full", st
    ref = _k1_reference(ctx, iters, huber)
    got = _run(ctx, gen.k1_window(), iters, True, huber=huber)
    assert got[4] == (iters >= 2) and got[5] == (iters + 1 if iters >= 2 else 2), got[4:]
    assert np.all(np.isfinite(got[1])) and not np.array_equal(got[2], gen.k1_window().poses_cw)
    _equal(got, ref, f"{iters} iterations")
    if huber > 0.0:  # the Huber cost is a different problem, not the plain one again
        assert not np.array_equal(got[1], _k1_reference(ctx, iters, 0.0)[1])


@pytest.mark.parametrize("name,n_poses,max_track,n_fixed,mode", gen.TAIL_CASES)
def test_layout_windows(ctx, name, n_poses, max_track, n_fixed, mode):
    """The full layout's tail windows (50 / 53 poses): chained equals split.  The split and ring
    layouts never chain (the gate needs the fused full-layout launch)."""
    p = gen.tail_window(n_poses, max_track, n_fixed)
    got = _run(ctx, p, 3, True)
    assert got[0] == _lib.VO_OK
    if mode != "full":
        assert not got[4] and got[5] == 6, (name, got[4:])
        return
    assert got[4] and got[5] == 4, (name, got[4:])
    _equal(got, _run(ctx, p, 3, False), name)


def test_run_twice_equals_split(ctx):
    """run(2); run(2): the second run's stand-alone K1 applies the first run's pending step."""
    out = []
    for chain in (True, False):
        _lib.ba_testing_no_chain(ctx, not chain)
        try:
            s = _session(gen.k1_window(), ctx)
            rc1, c1 = s.run(2)
            rc2, c2 = s.run(2)
            assert rc1 == _lib.VO_OK and rc2 == _lib.VO_OK
            assert _lib.ba_testing_last_run(ctx)[0] == chain
            out.append((c1, c2) + tuple(s.get_state()))
        finally:
            _lib.ba_testing_no_chain(ctx, False)
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)


def test_set_state_between_runs(ctx):
    """run(2); set_state; run(2) equals a fresh session's run(2): nothing of the first run (a
    publish word, a pending step) reaches the second."""
    p = gen.k1_window()
    s = _session(p, ctx)
    assert s.run(2)[0] == _lib.VO_OK
    s.set_state(p.poses_cw, p.points)
    rc, costs = s.run(2)
    assert _lib.ba_testing_last_run(ctx) == (True, 3)
    got = (rc, costs) + tuple(s.get_state())
    _equal(got, _run(ctx, p, 2, True), "after set_state")
    _equal(got, _k1_reference(ctx, 2, 0.0), "after set_state, split")


def test_run_async_equals_run(ctx):
    """run_async(3) + get_state equals run(3)."""
    s = _session(gen.k1_window(), ctx)
    s.run_async(3)
    assert _lib.ba_testing_last_run(ctx) == (True, 4)
    P, X = s.get_state()
    ref = _k1_reference(ctx, 3, 0.0)
    np.testing.assert_array_equal(P, ref[2])
    np.testing.assert_array_equal(X, ref[3])


def test_profiled_run_is_not_chained(ctx):
    """With kernel profiling on every iteration keeps its own ba_lin launch (profile_read shows
    it once per iteration) and the results are the same."""
    _lib.profile_enable(ctx, True)
    try:
        s = _session(gen.k1_window(), ctx)
        rc, costs = s.run(3)
        chained, launches = _lib.ba_testing_last_run(ctx)
        P, X = s.get_state()
        prof = _lib.profile_read(ctx)
    finally:
        _lib.profile_enable(ctx, False)
    assert not chained and launches == 6
    assert prof["ba_lin"][1] == 3 + 1 and prof["ba_solve"][1] == 3, prof  # (+ the read-out's back substitution)
    _equal((rc, costs, P, X), _k1_reference(ctx, 3, 0.0), "profiled")


def test_run_lm_ignores_the_switch(ctx):
    """vo_ba_run_lm never chains: its results do not depend on the switch."""
    out = []
    for off in (False, True):
        _lib.ba_testing_no_chain(ctx, off)
        try:
            s = _session(gen.k1_window(), ctx)
            r = s.run_lm(3)
            out.append(tuple(r) + tuple(s.get_state()))
        finally:
            _lib.ba_testing_no_chain(ctx, False)
    assert out[0][0] == _lib.VO_OK
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)


def test_not_spd_inside_a_chained_run(ctx):
    """A solve that is not SPD in a chained run of 3: VO_ERR_NOT_SPD, and the gated K1 workgroups
    of that launch and of the later ones apply nothing -- poses and landmarks as the split run's."""
    p, cam = gen.not_spd_window()
    got = _run(ctx, p, 3, True, lam=0.0, cam=cam)
    ref = _run(ctx, p, 3, False, lam=0.0, cam=cam)
    assert got[4] and not ref[4]
    assert got[0] == _lib.VO_ERR_NOT_SPD and ref[0] == _lib.VO_ERR_NOT_SPD
    np.testing.assert_array_equal(got[1], ref[1])  # (NaN from the failed iteration on, in both)
    np.testing.assert_array_equal(got[2], ref[2])
    np.testing.assert_array_equal(got[3], ref[3])
    np.testing.assert_array_equal(got[3], p.points)


def test_reducer_timeout_inside_a_chained_run(ctx):
    """The solver's bounded wait for its reducers (vo_ba_testing_drop_reducers) in a chained run
    of 3: VO_ERR_HIP naming the timeout; the solver publishes its failed verdict, so the gated K1
    workgroups return and the state stays as the split run leaves it."""
    p = gen.k1_window()
    states = []
    # (every launch short of a reducer waits its bound out, most of a second: the split reference
    # is a run of 1 -- a timed-out iteration freezes the state, so its later launches change nothing)
    for chain, iters in ((True, 3), (False, 1)):
        _lib.ba_testing_no_chain(ctx, not chain)
        _lib.ba_testing_drop_reducers(ctx, 1)
        try:
            s = _session(p, ctx)
            with pytest.raises(_lib.VoError, match="timed out") as e:
                s.run(iters)
            assert e.value.code == _lib.VO_ERR_HIP
            assert _lib.ba_testing_last_run(ctx)[0] == chain
        finally:
            _lib.ba_testing_drop_reducers(ctx, 0)
            _lib.ba_testing_no_chain(ctx, False)
        states.append(s.get_state())
    np.testing.assert_array_equal(states[0][0], states[1][0])
    np.testing.assert_array_equal(states[0][1], states[1][1])
    np.testing.assert_array_equal(states[0][1], p.points)
    # the context recovers: the next chained run is exact
    _equal(_run(ctx, p, 2, True), _k1_reference(ctx, 2, 0.0), "after the timeout")


def test_handoff_with_a_warm_consumer(ctx):
    """The hand-off under repetition and uneven load.  The pose buffers ping-pong, so each K1
    workgroup re-reads, as pose_new, lines its CU read as pose_old one launch earlier: a stale L1
    line would show as a different result.  Twenty chained runs of 5 in one process, every one
    bitwise equal to the first and to the split sequence; then once more while another stream of
    the process keeps the memory system busy (large triangulation batches on a second context)."""
    from visualodometry_amd import triangulate
    from visualodometry_amd.synthetic import triangulation_case

    p = gen.k1_window()
    ref = _k1_reference(ctx, 5, 0.0)
    s = _session(p, ctx)
    for i in range(20):
        s.set_state(p.poses_cw, p.points)
        rc, costs = s.run(5)
        assert _lib.ba_testing_last_run(ctx) == (True, 6)
        _equal((rc, costs) + tuple(s.get_state()), ref, f"run {i}")

    other = _lib.Context(0)
    T1, T2, q1, q2, K, _, _ = triangulation_case(400000, 0)
    stop, started, err = threading.Event(), threading.Event(), []

    def load():
        try:
            while not stop.is_set():
                triangulate.triangulate_all(T1, T2, q1, q2, K, 0.001, 6.0, other)
                started.set()
        except Exception as ex:  # noqa: BLE001
            err.append(ex)
            started.set()

    th = threading.Thread(target=load)
    th.start()
    try:
        started.wait()
        for i in range(5):
            s.set_state(p.poses_cw, p.points)
            rc, costs = s.run(5)
            _equal((rc, costs) + tuple(s.get_state()), ref, f"loaded run {i}")
    finally:
        stop.set()
        th.join()
    assert not err, err
