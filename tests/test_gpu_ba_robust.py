"""The Huber-robust BA cost and the per-observation residual read-out on the MI355X, against the
CPU restatement (tests/ba_robust_ref.py) on windows with 5 % gross outliers.

Inputs: ``make_ba_problem(n, L, seed)`` with ``ba_robust_ref.with_outliers``; lambda = 1 and
delta = 2 px unless a test says otherwise.  The step tests run at two states: the initial guess
(nearly every observation beyond delta) and the state after five reference iterations (about a
tenth beyond it), so both branches of the scale carry weight (tests/test_ba_robust_ref.py).
The robust cost is not monotone under the fixed lambda; nothing here asserts that it is.
"""

import functools
import threading

import numpy as np
import pytest

from oracle import ba_ref
from tests import ba_robust_ref as rr
from visualodometry_amd import _lib
from visualodometry_amd._lib import VoError
from visualodometry_amd.ba import BASession, BAWindow, SlidingWindowBA
from visualodometry_amd.shard import shard
from visualodometry_amd.synthetic import make_ba_problem

pytestmark = pytest.mark.gpu

LAM, DELTA = 1.0, 2.0
REL = 1e-5  # the project's tolerance for a whole solve
SMALL, WIDE = (8, 300, 21), (12, 600, 3)


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300)


@functools.lru_cache(maxsize=None)
def _case(case):
    p = make_ba_problem(*case)
    uv = rr.with_outliers(p, case[2])
    return p, uv, rr.structure(p, uv), ba_ref.BAState.from_poses(p.poses_cw, p.points)


@functools.lru_cache(maxsize=None)
def _ref_solve(case, iters, delta):
    """The restatement's solve from the initial guess (computed once, never modified)."""
    _, _, s, st0 = _case(case)
    return rr.solve(st0, s, iters, LAM, delta)


def _session(case, ctx, huber=DELTA, state=None):
    p, uv, _, st0 = _case(case)
    s = BASession(p.K, p.point_ptr, p.obs_cam, uv, p.n_poses, p.n_fixed, LAM, ctx, huber=huber)
    st = state or st0
    s.set_state(st.poses_cw(), st.X)
    return s


def _gpu_solve(case, ctx, iters, huber=DELTA):
    s = _session(case, ctx, huber)
    rc, costs = s.run(iters)
    assert rc == _lib.VO_OK
    P, X = s.get_state()
    return costs, P, X


def _check_step(s, ref):
    """gn_step against the restatement at test_step_matches_numpy_oracle's tolerances."""
    rc, S, b, dc, cost = s.gn_step()
    assert rc == _lib.VO_OK
    P, X = s.get_state()
    figs = dict(cost=abs(cost - ref.system.cost) / ref.system.cost, S=_rel(S, ref.system.S), b=_rel(b, ref.system.b),
                dc=_rel(dc, ref.dc), P=_rel(P, ref.state.poses_cw()), X=_rel(X, ref.state.X))
    print("step errors:", {k: f"{v:.2e}" for k, v in figs.items()})
    assert np.isfinite(S).all() and np.isfinite(dc).all() and np.isfinite(X).all()
    assert figs["cost"] <= 1e-12
    assert figs["S"] < 1e-11
    assert figs["b"] < 1e-10
    assert figs["dc"] < 1e-8
    assert figs["P"] < 1e-8
    assert figs["X"] < 1e-8


@pytest.mark.parametrize("which", ["initial", "after5"])
def test_step_parity(ctx, which):
    _, _, struct, st0 = _case(SMALL)
    st = st0 if which == "initial" else _ref_solve(SMALL, 5, DELTA)[0]
    _check_step(_session(SMALL, ctx, DELTA, st), rr.gn_step(st, struct, LAM, DELTA))


@pytest.mark.parametrize("case", [SMALL, WIDE])
def test_solve_parity(ctx, case):
    p, _, struct, st0 = _case(case)
    iters = 8
    costs, P, X = _gpu_solve(case, ctx, iters)
    ref, ref_costs = _ref_solve(case, iters, DELTA)
    print("solve errors:", f"{_rel(costs, ref_costs):.2e} {_rel(P, ref.poses_cw()):.2e} {_rel(X, ref.X):.2e}")
    assert _rel(costs, ref_costs) < REL
    assert _rel(P, ref.poses_cw()) < REL
    assert _rel(X, ref.X) < REL
    plain, _ = _ref_solve(case, iters, 0.0)
    e_plain, e_gpu = rr.max_translation_error(plain.poses_cw(), p), rr.max_translation_error(P, p)
    print(f"translation error: plain {e_plain:.3f} m, Huber on the GPU {e_gpu:.3f} m")
    assert e_gpu < 0.25 * e_plain


def test_every_k1_variant(ctx):
    """The robust solve under each K1: the four-wave kernel (-1) and the one-wave kernel with 1, 2
    and 6 chunks per segment -- against the restatement, against each other (only the summation
    order differs) and bitwise against itself."""
    iters = 8
    ref, ref_costs = _ref_solve(SMALL, iters, DELTA)
    runs = {}
    try:
        for v in (-1, 1, 2, 6):
            _lib.ba_testing_k1(ctx, v)
            a = _gpu_solve(SMALL, ctx, iters)
            b = _gpu_solve(SMALL, ctx, iters)
            for x, y in zip(a, b):
                np.testing.assert_array_equal(x, y)
            runs[v] = a
    finally:
        _lib.ba_testing_k1(ctx, 0)
    for v, (costs, P, X) in runs.items():
        assert _rel(costs, ref_costs) < REL and _rel(P, ref.poses_cw()) < REL and _rel(X, ref.X) < REL, v
        for w, (costs2, P2, X2) in runs.items():
            assert _rel(costs, costs2) < 1e-8 and _rel(P, P2) < 1e-8 and _rel(X, X2) < 1e-8, (v, w)


def test_huge_delta_equals_off(ctx):
    """delta = 1e9: every scale is exactly 1, the robust kernels compute the plain step."""
    iters = 3
    c0, P0, X0 = _gpu_solve(SMALL, ctx, iters, huber=0.0)
    c1, P1, X1 = _gpu_solve(SMALL, ctx, iters, huber=1e9)
    print("huge delta vs off:", f"{_rel(c1, c0):.2e} {_rel(P1, P0):.2e} {_rel(X1, X0):.2e}")
    assert _rel(c1, c0) < 1e-12
    assert _rel(P1, P0) < 1e-10
    assert _rel(X1, X0) < 1e-10


def test_set_then_cleared_is_bitwise_off(ctx):
    """delta = 2 and then 0 before the first run: the plain kernels on the same bits as a session
    that never set it."""
    c0, P0, X0 = _gpu_solve(SMALL, ctx, 4, huber=0.0)
    s = _session(SMALL, ctx, huber=0.0)
    s.set_robust(DELTA)
    s.set_robust(0.0)
    rc, c1 = s.run(4)
    assert rc == _lib.VO_OK
    P1, X1 = s.get_state()
    np.testing.assert_array_equal(c1, c0)
    np.testing.assert_array_equal(P1, P0)
    np.testing.assert_array_equal(X1, X0)


@pytest.mark.parametrize("pending", [False, True])
def test_mid_run_switch(ctx, pending):
    """Two plain iterations, then delta = 2 for three more.  pending: the first two are enqueued
    without a synchronisation, so the switch finds a pose step whose landmark update is still
    to be applied -- under the old delta (0), before the new one holds."""
    _, _, struct, st0 = _case(SMALL)
    ref, (rc0, rc1) = rr.solve_schedule(st0, struct, [(2, 0.0), (3, DELTA)], LAM)
    s = _session(SMALL, ctx, huber=0.0)
    if pending:
        s.run_async(2)
    else:
        rc, c0 = s.run(2)
        assert rc == _lib.VO_OK and _rel(c0, rc0) < REL
    s.set_robust(DELTA)
    rc, c1 = s.run(3)
    assert rc == _lib.VO_OK
    P, X = s.get_state()
    assert _rel(c1, rc1) < REL
    assert _rel(P, ref.poses_cw()) < REL
    assert _rel(X, ref.X) < REL


def test_tiny_delta_step(ctx):
    """delta = 1e-3 px: every observation beyond delta, scales of ~0.01-0.03; the step stays
    finite and matches at the step tolerances."""
    _, _, struct, st0 = _case(SMALL)
    r, _ = ba_ref.residuals(st0, struct)
    assert rr.huber_scale(r, 1e-3)[2].all()
    _check_step(_session(SMALL, ctx, 1e-3), rr.gn_step(st0, struct, LAM, 1e-3))


def test_bad_delta_and_stale_session(ctx):
    s = _session(SMALL, ctx, huber=0.0)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(VoError) as e:
            s.set_robust(bad)
        assert e.value.code == _lib.VO_ERR_ARG
    s.set_robust(DELTA)  # still usable
    s.residuals()
    _session(SMALL, ctx, huber=0.0)  # another vo_ba_setup on the context replaces the problem
    with pytest.raises(VoError) as e:
        s.set_robust(DELTA)
    assert e.value.code == _lib.VO_ERR_STATE
    with pytest.raises(VoError) as e:
        s.residuals()
    assert e.value.code == _lib.VO_ERR_STATE


def _check_residuals(err2, depth, P, X, struct):
    """Against the oracle's residuals at (P, X): squared norm to 1e-10 relative and depth to 1e-12
    relative, per observation, no absolute term.  Measured on the MI355X at the states these tests
    visit: 1.1e-11 and 7e-16 at most (DESIGN.md §Robust cost)."""
    r, pc = ba_ref.residuals(ba_ref.BAState.from_poses(P, X), struct)
    e2 = (r * r).sum(-1)
    print("read-out errors:", f"{(np.abs(err2 - e2) / e2).max():.2e} {(np.abs(depth - pc[:, 2]) / pc[:, 2]).max():.2e}")
    np.testing.assert_allclose(err2, e2, rtol=1e-10, atol=0)
    np.testing.assert_allclose(depth, pc[:, 2], rtol=1e-12, atol=0)


def test_residual_readout(ctx):
    _, _, struct, st0 = _case(SMALL)
    s = _session(SMALL, ctx)
    _check_residuals(*s.residuals(), st0.poses_cw(), st0.X, struct)  # right after set_state
    rc, _ = s.run(3)
    assert rc == _lib.VO_OK
    err2, depth = s.residuals()
    _check_residuals(err2, depth, *s.get_state(), struct)
    # the outliers are what the solve ends up disagreeing with
    moved = np.abs(struct.obs_uv - _case(SMALL)[0].obs_uv).max(-1) > 0
    assert np.median(err2[moved]) > 100 * np.median(err2[~moved])
    s.run_async(1)  # a pose step whose landmark update is pending
    err2, depth = s.residuals()
    _check_residuals(err2, depth, *s.get_state(), struct)


def test_optimize_returns_residuals_in_window_order(ctx):
    p, uv, _, _ = _case(SMALL)
    perm = np.random.default_rng(7).permutation(p.obs_cam.size)
    obs_pt = np.repeat(np.arange(p.n_points), np.diff(p.point_ptr))[perm]
    w = BAWindow(p.poses_cw, p.points, uv[perm], p.obs_cam[perm], obs_pt, p.n_fixed)
    ba = SlidingWindowBA(p.K, None, iters=4, lam=LAM, huber=DELTA)
    res = ba.optimize(w, return_residuals=True)
    assert res.status == "ok" and res.obs_err2.shape == (perm.size,)
    struct = rr.structure(p, uv)
    struct.obs_cam, struct.obs_uv, struct.obs_pt = p.obs_cam[perm], uv[perm], obs_pt
    _check_residuals(res.obs_err2, res.obs_depth, res.poses_cw, res.points, struct)
    assert ba.optimize(w).obs_err2 is None
    cfg = type("Cfg", (), {"ba_huber": 1.5, "ba_iters": 2})()
    assert SlidingWindowBA(p.K, cfg).huber == 1.5 and SlidingWindowBA(p.K).huber == 0.0


def test_sharded_robust_matches_unsharded():
    """Two loopback ranks (tests/test_gpu_sharded_loopback.py), each setting delta on its own
    landmark shard, against the unsharded robust run on a context of its own.  Each rank's read-out
    is its own observations in its shard's order (landmark indices are shard-local there): checked
    against the oracle over the shard's structure at the state that rank returned, and against the
    unsharded read-out restricted to the shard's observations."""
    p, uv, _, _ = _case(WIDE)
    iters, nranks = 5, 2
    s0 = BASession(p.K, p.point_ptr, p.obs_cam, uv, p.n_poses, p.n_fixed, LAM, _lib.Context(0), huber=DELTA)
    s0.set_state(p.poses_cw, p.points)
    rc0, c0 = s0.run(iters)
    P0, X0 = s0.get_state()
    err2_0, depth_0 = s0.residuals()
    out, errors = [None] * nranks, []

    def worker(r):
        try:
            ctx = _lib.Context(0)
            _lib.comm_init_loopback(ctx, nranks, r, b"vo-loopback-robust")
            (p0, p1), ptr, cam, suv, pts = shard(p.point_ptr, p.obs_cam, uv, p.points, nranks, r)
            s = BASession(p.K, ptr, cam, suv, p.n_poses, p.n_fixed, LAM, ctx, huber=DELTA)
            s.set_state(p.poses_cw, pts)
            rc, costs = s.run(iters)
            poses, q = s.get_state()
            out[r] = (rc, costs, poses, q, s.residuals(), (p0, p1, ptr, cam, suv))
        except Exception as e:  # surfaced below
            errors.append(e)

    th = [threading.Thread(target=worker, args=(r,)) for r in range(nranks)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in th), "loopback group deadlocked"
    if errors:
        raise errors[0]
    assert rc0 == _lib.VO_OK and all(o[0] == rc0 for o in out)
    np.testing.assert_array_equal(out[1][1], out[0][1])
    np.testing.assert_array_equal(out[1][2], out[0][2])
    np.testing.assert_allclose(out[0][1], c0, rtol=1e-9)
    np.testing.assert_allclose(out[0][2], P0, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(np.concatenate([o[3] for o in out]), X0, rtol=1e-8, atol=1e-10)
    o1 = 0
    for rc, _, poses, q, (err2, depth), (p0, p1, ptr, cam, suv) in out:
        o0 = int(p.point_ptr[p0])
        assert o0 == o1  # the shards follow one another
        o1 = int(p.point_ptr[p1])
        assert err2.shape == depth.shape == (o1 - o0,)
        _check_residuals(err2, depth, poses, q, ba_ref.BAStructure(p.K, ptr, cam, suv, p.n_fixed, p.n_poses))
        # The same observations of the unsharded run.  The two states agree to 1e-8 relative
        # (above): landmarks up to ~60 m away move by <= 6e-7 m, a projection (focal length ~700 px,
        # depth >= 1 m) by <= 5e-4 px, the depth by <= 1e-6 relative.  On the gross outliers
        # (|r| >= 20 px) that is <= 5e-5 relative in r.r.
        big = err2_0[o0:o1] > 400.0
        assert big.sum() >= 10
        np.testing.assert_allclose(err2[big], err2_0[o0:o1][big], rtol=1e-4)
        np.testing.assert_allclose(depth, depth_0[o0:o1], rtol=1e-6)
    assert o1 == p.obs_cam.size  # the shards' read-outs cover every observation once
