"""The covariance restatement against itself (CPU): the Schur route the library follows (A) and the
dense inverse of the full normal matrix (B) agree, and the properties a covariance must have."""

import functools

import numpy as np
import pytest

from oracle import ba_ref
from tests import ba_cov_ref as cr
from visualodometry_amd.synthetic import make_ba_problem

ROUTES_TOL = 1e-9  # every input of the GPU parity test must meet it (its tolerance is 100 x eps_ref)


@functools.lru_cache(maxsize=None)
def _problem(name):
    n, l, seed, kw = cr.INPUTS[name]
    return make_ba_problem(n, l, seed, **kw)


def _state(p):
    return (ba_ref.BAState.from_poses(p.poses_cw, p.points),
            ba_ref.BAStructure(p.K, p.point_ptr, p.obs_cam, p.obs_uv, p.n_fixed, p.n_poses))


@pytest.mark.parametrize("lam", [0.0, 1.0])
@pytest.mark.parametrize("name", list(cr.INPUTS))
def test_routes_agree(name, lam):
    st, s = _state(_problem(name))
    eps, (cc, pp) = cr.routes_disagreement(st, s, lam)
    print(f"{name} lam={lam}: eps_ref {eps:.3g}")
    assert eps <= ROUTES_TOL
    np.testing.assert_array_equal(cc, cc.T)
    assert (np.diag(cc) > 0).all()
    np.testing.assert_array_equal(pp, pp.transpose(0, 2, 1))
    assert (np.diagonal(pp, axis1=1, axis2=2) > 0).all()


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_damping_shrinks_the_variances(name):
    st, s = _state(_problem(name))
    cc0, pp0 = cr.route_a(st, s, 0.0)
    cc1, pp1 = cr.route_a(st, s, 1.0)
    assert (np.diag(cc1) <= np.diag(cc0)).all()
    assert (np.diagonal(pp1, axis1=1, axis2=2) <= np.diagonal(pp0, axis1=1, axis2=2)).all()


def test_routes_agree_under_huber():
    from tests import ba_robust_ref as rr

    p = _problem("small")
    uv = rr.with_outliers(p, 21)
    st = ba_ref.BAState.from_poses(p.poses_cw, p.points)
    s = ba_ref.BAStructure(p.K, p.point_ptr, p.obs_cam, uv, p.n_fixed, p.n_poses)
    eps, (cc, _) = cr.routes_disagreement(st, s, 1.0, 2.0)
    assert eps <= ROUTES_TOL
    plain = cr.route_a(st, s, 1.0)[0]
    assert cr.rel_err(cc, plain) > 1e-3  # the scale changes the answer


def test_narrow_band_has_correlations_outside_it():
    """S of the narrow input has a block row span of 3; its inverse is dense, with correlations
    above 0.9 outside the band (an implementation that inverts the band alone fails the parity)."""
    st, s = _state(_problem("narrow"))
    sys_ = ba_ref.build_system(st, s, 0.0)
    F = s.n_free
    nz = np.abs(sys_.S.reshape(F, 6, F, 6)).max(axis=(1, 3)) > 0
    span = max(i - np.nonzero(nz[i])[0].min() for i in range(F))
    assert span == 3
    cc, _ = cr.route_a(st, s, 0.0)
    d = np.sqrt(np.diag(cc))
    corr = np.abs(cc / d[:, None] / d[None, :]).reshape(F, 6, F, 6).max(axis=(1, 3))
    outside = np.abs(np.subtract.outer(np.arange(F), np.arange(F))) > span
    assert corr[outside].max() > 0.9


def test_frozen_and_fixed_only_landmarks():
    p = make_ba_problem(6, 120, 31)
    ptr2, cam2, uv2 = cr.degenerate_problem(p, duplicate=False)
    st = ba_ref.BAState.from_poses(p.poses_cw, p.points)
    s = ba_ref.BAStructure(p.K, ptr2, cam2, uv2, 2, p.n_poses)
    _, pp0 = cr.route_a(st, s, 0.0)
    assert np.isnan(pp0[0]).all()  # one observation, no damping: V is singular
    assert np.isfinite(pp0[1:]).all()
    _, pp1 = cr.route_a(st, s, 1.0)
    assert np.isfinite(pp1).all()
    for lam, pp in ((0.0, pp0), (1.0, pp1)):  # fixed cameras only: V^-1, no pose term
        sys_ = ba_ref.build_system(st, s, lam)
        np.testing.assert_array_equal(pp[2], 0.5 * (sys_.Vinv[2] + sys_.Vinv[2].T))


def test_wide_problem_is_wide_and_usable_at_lambda_1():
    """The wide input of the GPU parity: a block column with more than 256 rows below its
    diagonal block, and routes that agree at lambda = 1."""
    p, cam, uv = cr.wide_problem()
    st = ba_ref.BAState.from_poses(p.poses_cw, p.points)
    s = ba_ref.BAStructure(p.K, p.point_ptr, cam, uv, p.n_fixed, p.n_poses)
    F = s.n_free
    nz = np.abs(ba_ref.build_system(st, s, 1.0).S.reshape(F, 6, F, 6)).max(axis=(1, 3)) > 0
    first = np.array([np.nonzero(nz[i])[0].min() for i in range(F)])
    last = np.array([max(i for i in range(F) if first[i] <= k) for k in range(F)])
    assert 6 * (last - np.arange(F)).max() > 256
    eps, _ = cr.routes_disagreement(st, s, 1.0)
    print(f"wide lam=1: eps_ref {eps:.3g}")
    assert eps <= ROUTES_TOL
