"""GPU parity of the essential-matrix initialisation (``vo_essential_ransac`` /
``vo_recover_pose``, reference ``src/modules/vo.py:87-101``) against the CPU restatement in
tests/essential_ref.py: success flags, inlier masks and ``good`` identical, E (up to sign), R and
t within 1e-5.  The kernels run essential_math.h's + - * / sqrt in the restatement's operation
order without FMA contraction, so they agree to the bit in practice; only log and pow of the
iteration update are device libm, and they go through rint.  Planted outliers sit 30-100 px
across their epipolar line, noise is 0.3 px, threshold 1.0 and prob 0.999 (the reference's
config) unless stated."""

import functools
import types

import numpy as np
import pytest

from tests import essential_ref as R
from visualodometry_amd import essential
from visualodometry_amd.dropin import hooks
from visualodometry_amd.synthetic import two_view_case

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(n, seed, frac, motion="forward", max_iters=1000, prob=0.999):
    """(inputs, the reference's result): computed once, shared, never modified."""
    p1, p2, K, Rt, t, out = two_view_case(n, seed, noise_px=0.3, outlier_frac=frac, motion=motion)
    ref = R.find_essential_ransac(p1, p2, K, prob=prob, max_iters=max_iters)
    for a in (p1, p2, K, Rt, t, out, ref[1], ref[2]):
        a.setflags(write=False)
    return (p1, p2, K, Rt, t, out), ref


def _same_E(E, rE):
    return min(np.abs(E - rE).max(), np.abs(E + rE).max()) <= 1e-5


def _check_ransac(ctx, n, seed, frac, motion="forward", max_iters=1000, prob=0.999):
    (p1, p2, K, _, _, out), (rok, rE, rmask, info) = _case(n, seed, frac, motion, max_iters, prob)
    ok, E, mask = essential.find_essential_ransac(p1, p2, K, 1.0, prob, max_iters, ctx=ctx)
    assert ok == rok
    np.testing.assert_array_equal(mask, rmask)
    assert _same_E(E, rE)
    if ok:
        assert abs(np.linalg.norm(E) - 1.0) < 1e-12
    if max_iters == 1000 and prob == 0.999:  # a loop cut short may stop at a model of outliers
        assert not (mask & out).any(), "a planted outlier is in the inlier mask"
    return E, info


def _check_pose(ctx, E, p1, p2, K):
    good, Rm, t, mask = essential.recover_pose(E, p1, p2, K, ctx=ctx)
    rgood, rR, rt, rmask = R.recover_pose(E, p1, p2, K)
    assert good == rgood
    np.testing.assert_array_equal(mask, rmask)
    np.testing.assert_allclose(Rm, rR, rtol=0, atol=1e-5)
    np.testing.assert_allclose(t, rt, rtol=0, atol=1e-5)
    return good, Rm, t


# both sides of the wave (64) and workgroup (256 / 1024) edges; each motion at least once
SIZES = [(5, 1, 0.0, "forward"), (6, 2, 0.0, "sideways"), (8, 3, 0.0, "turn"), (63, 4, 0.2, "forward"),
         (64, 5, 0.2, "sideways"), (65, 6, 0.2, "turn"), (400, 7, 0.25, "forward"), (1025, 8, 0.3, "sideways"),
         (2000, 9, 0.3, "turn")]


@pytest.mark.parametrize("n,seed,frac,motion", SIZES)
def test_ransac_and_pose_match_reference(ctx, n, seed, frac, motion):
    """find_essential_ransac against the reference, then recover_pose on its E and on -E (the
    candidate order: the same pose must win from either sign)."""
    E, _ = _check_ransac(ctx, n, seed, frac, motion)
    p1, p2, K = _case(n, seed, frac, motion)[0][:3]
    a = _check_pose(ctx, E, p1, p2, K)
    b = _check_pose(ctx, -E, p1, p2, K)
    if n >= 63:  # a handful of points can tie two candidates, and -E swaps R1 and R2
        assert a[0] == b[0]
        np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(a[2], b[2])


def test_loop_ends_inside_the_first_slice(ctx):
    """No outliers: the serial loop stops after a handful of iterations, inside the first slice
    of 64 hypotheses; the rest is never solved."""
    _, info = _check_ransac(ctx, 400, 10, 0.0)
    assert info["iters"] < 64


def test_loop_needs_the_tail(ctx):
    """45 % outliers: the loop runs past the first slice, so the second pair of launches does
    the work and the replay crosses the slice boundary."""
    _, info = _check_ransac(ctx, 400, 11, 0.45)
    assert 64 < info["iters"] < 1000


@pytest.mark.parametrize("max_iters,prob", [(1, 0.999), (20, 0.999), (1000, 0.5)])
def test_iterations_and_confidence(ctx, max_iters, prob):
    _check_ransac(ctx, 400, 9, 0.4, "forward", max_iters, prob)


def test_edge_cases(ctx):
    """n in {0, 4} and a set without any model fail with zero masks; random correspondences
    follow the reference (a five-point model always has its own five inliers)."""
    p1, p2, K = _case(63, 4, 0.2)[0][:3]
    for n in (0, 4):
        ok, E, mask = essential.find_essential_ransac(p1[:n], p2[:n], K, ctx=ctx)
        assert not ok and not E.any() and mask.shape == (n,) and not mask.any()
    same = np.repeat(p1[:1], 30, 0)
    ok, E, mask = essential.find_essential_ransac(same, same, K, max_iters=50, ctx=ctx)
    assert not ok and not E.any() and not mask.any()
    assert essential.findEssentialMat(same, same, K, method=essential.RANSAC, ctx=ctx) == (None, None)
    rng = np.random.default_rng(0)
    a = np.stack([rng.uniform(0, 1240, 100), rng.uniform(0, 370, 100)], 1).astype(np.float32)
    b = np.stack([rng.uniform(0, 1240, 100), rng.uniform(0, 370, 100)], 1).astype(np.float32)
    ok, E, mask = essential.find_essential_ransac(a, b, K, max_iters=100, ctx=ctx)
    rok, rE, rmask, _ = R.find_essential_ransac(a, b, K, max_iters=100)
    assert ok == rok and _same_E(E, rE)
    np.testing.assert_array_equal(mask, rmask)
    good, _, _, pm = essential.recover_pose(np.eye(3), p1[:0], p2[:0], K, ctx=ctx)
    assert good == 0 and pm.shape == (0,)


@pytest.mark.parametrize("motion", ["forward", "sideways", "turn"])
def test_pose_of_the_true_E(ctx, motion):
    p1, p2, K, Rt, t, out = two_view_case(400, 12, noise_px=0.3, outlier_frac=0.2, motion=motion)
    Et = R.essential_from_pose(Rt, t)
    for s in (1.0, -1.0):
        good, Rm, tv = _check_pose(ctx, s * Et, p1, p2, K)
        assert good > 200 and R.rotation_angle(Rm, Rt) < 1e-6 and R.direction_angle(tv, t) < 1e-6


def test_cv2_signature_wrappers(ctx):
    (p1, p2, K, *_), (rok, rE, rmask, _) = _case(400, 7, 0.25)
    E, mask = essential.findEssentialMat(p1, p2, K, method=essential.RANSAC, prob=0.999, threshold=1.0, ctx=ctx)
    assert E.shape == (3, 3) and E.dtype == np.float64 and mask.shape == (400, 1) and mask.dtype == np.uint8
    assert set(np.unique(mask)) <= {0, 1} and _same_E(E, rE)
    np.testing.assert_array_equal(mask[:, 0].astype(bool), rmask)
    good, Rm, t, pm = essential.recoverPose(E, p1, p2, K, ctx=ctx)
    assert isinstance(good, int) and Rm.shape == (3, 3) and t.shape == (3, 1) and pm.shape == (400, 1)
    assert pm.dtype == np.uint8 and set(np.unique(pm)) <= {0, 255} and int((pm == 255).sum()) == good
    assert essential.findEssentialMat(p1[:4], p2[:4], K, ctx=ctx) == (None, None)
    with pytest.raises(ValueError):
        essential.findEssentialMat(p1, p2, K, method=4, ctx=ctx)
    with pytest.raises(ValueError):
        essential.recoverPose(E, p1, p2, K, mask=pm, ctx=ctx)


def test_proxy_runs_the_initialisation_sequence(ctx):
    """The reference's initialisation lines (vo.py:87-101) through Cv2Proxy with the flag on:
    the pose equals recover_pose's on the reference's E."""
    (p1, p2, K, *_), (rok, rE, rmask, _) = _case(400, 7, 0.25)

    def never(*a, **k):
        raise AssertionError("the host cv2 was called")

    cv2 = hooks.Cv2Proxy(types.SimpleNamespace(RANSAC=8, findEssentialMat=never, recoverPose=never),
                         lambda: True, lambda: True)
    E, mask = cv2.findEssentialMat(p1, p2, K, method=cv2.RANSAC, prob=0.999, threshold=1.0)
    assert E is not None
    _, Rm, t, _ = cv2.recoverPose(E, p1, p2, K)
    T_cw = np.eye(4)
    T_cw[:3, :3] = Rm
    T_cw[:3, 3] = t.flatten() * 20.0
    rgood, rR, rt, _ = R.recover_pose(rE, p1, p2, K)
    np.testing.assert_allclose(T_cw[:3, :3], rR, rtol=0, atol=1e-5)
    np.testing.assert_allclose(T_cw[:3, 3], rt * 20.0, rtol=0, atol=2e-4)
    assert _same_E(E, rE)
    np.testing.assert_array_equal(mask[:, 0].astype(bool), rmask)
