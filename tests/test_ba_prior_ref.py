"""The pose-prior restatement (tests/ba_prior_ref.py) against itself and the oracle, on the CPU: the
log inverts the oracle's exp map, the prior's b term is its cost's gradient, and a prior built by
``marginalize`` makes the reduced window take the step the full window takes."""

import functools

import numpy as np
import pytest

from oracle import ba_ref
from tests import ba_prior_ref as pr
from visualodometry_amd.synthetic import make_ba_problem

SMALL, NARROW = (8, 300, 21, ()), (16, 400, 5, (("max_track", 4),))
IDENTITY = 1e-9  # the two routes' own disagreement must stay below this, scaled by max |dc|


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300)


@functools.lru_cache(maxsize=None)
def _case(case):
    n, L, seed, kw = case
    p = make_ba_problem(n, L, seed, **dict(kw))
    s = ba_ref.BAStructure(p.K, p.point_ptr, p.obs_cam, p.obs_uv, p.n_fixed, p.n_poses)
    return p, s, ba_ref.BAState.from_poses(p.poses_cw, p.points)


@pytest.mark.parametrize("scale", [1e-7, 0.5 * ba_ref.EXP_TAYLOR_THETA, 2.0 * ba_ref.EXP_TAYLOR_THETA, 1e-2, 0.4, 0.6, 1.5])
def test_log_inverts_exp_on_both_sides_of_the_series_thresholds(scale):
    """Rotation angles around the oracle's threshold (1e-4) and the device's (0.5)."""
    rng = np.random.default_rng(3)
    d = rng.normal(size=(64, 6))
    d[:, 3:] *= scale / np.linalg.norm(d[:, 3:], axis=1, keepdims=True)
    R, t = ba_ref.se3_exp(d)
    err = np.abs(pr.se3_log(R, t) - d).max()
    print(f"|phi| = {scale:g}: log(exp(d)) - d = {err:.2e}")
    assert err < 1e-12


def _synthetic_prior(s, st0, k, seed=0):
    rng = np.random.default_rng(seed)
    n = 6 * k
    A = rng.normal(size=(n, n))
    info = A.T @ A + np.eye(n)
    return pr.Prior(info, info @ (0.01 * rng.normal(size=n)), st0.poses_cw()[s.n_fixed:s.n_fixed + k], 2.0)


def test_prior_gradient_against_finite_differences():
    """At xi = 0 (poses0 = the state) the b term eta - Lambda xi is minus half the gradient of
    E_prior along the solver's own update, and S's term its Gauss-Newton Hessian."""
    _, s, st0 = _case(SMALL)
    k = 3
    prior = _synthetic_prior(s, st0, k)
    Sa, ba, e0 = pr.prior_terms(st0, s, prior)
    # (R R^T is the identity to rounding only)
    assert abs(e0 - prior.cost0) < 1e-12 and np.abs(pr.twists(st0, s, prior)).max() < 1e-14
    h = 1e-6
    g = np.zeros(6 * s.n_free)
    for i in range(6 * k):
        d = np.zeros(6 * s.n_free)
        d[i] = h
        ep = pr.prior_cost(pr.twists(ba_ref.apply_update(st0, s, d, 0 * st0.X), s, prior), prior)
        em = pr.prior_cost(pr.twists(ba_ref.apply_update(st0, s, -d, 0 * st0.X), s, prior), prior)
        g[i] = (ep - em) / (2 * h)
    err = _rel(-0.5 * g, ba)
    print(f"prior gradient against central differences: {err:.2e}")
    assert err < 1e-7
    assert (ba[6 * k:] == 0).all() and (Sa[6 * k:] == 0).all() and (Sa[:, 6 * k:] == 0).all()
    np.testing.assert_array_equal(Sa[:6 * k, :6 * k], prior.info)


def _full_and_reduced(s, st, n_drop, prior=None):
    err, _, new, k, mask, info, s2, st2 = pr.slide_identity(st, s, n_drop, prior)
    return err, new, k, mask, info, s2, st2


@pytest.mark.parametrize("case", [SMALL, NARROW])
@pytest.mark.parametrize("n_drop", [1, 3])
def test_marginalisation_identity(case, n_drop):
    """One GN step of the full window and one of the reduced window with the prior from
    ``marginalize`` at the same state give the remaining poses the same update.  n_drop = 1 <=
    n_fixed eliminates no pose (m = 0), n_drop = n_fixed + 1 one."""
    p, s, st0 = _case(case)
    st = pr.gn_step(st0, s, 1.0, None).state  # a state off the initial guess
    err, new, k, mask, info, s2, _ = _full_and_reduced(s, st, n_drop)
    print(f"{case[:3]} n_drop {n_drop}: K {k}, {int(mask.sum())} landmarks marginalised, "
          f"routes' disagreement {err:.2e} of max |dc|")
    assert err < IDENTITY
    assert s2.n_fixed == max(0, s.n_fixed - n_drop) and 0 < k <= s2.n_free and 0 < mask.sum() < mask.size
    np.testing.assert_array_equal(info, info.T)
    assert (info[6 * k:] == 0).all() and np.abs(info[6 * k - 6:6 * k]).max() > 0
    # cost0 is the marginalised factors' cost at the state: xi = 0 there
    assert abs(pr.prior_cost(np.zeros(6 * k), new) - new.cost0) == 0 and new.cost0 > 0


def test_second_slide_folds_the_first_prior_in():
    p, s, st0 = _case(NARROW)
    st = pr.gn_step(st0, s, 1.0, None).state
    err1, prior1, k1, mask1, _, s2, st2 = _full_and_reduced(s, st, 1)
    st2 = pr.gn_step(st2, s2, 1.0, prior1).state  # the reduced window moves on, then slides again
    err2, prior2, k2, mask2, _, s3, _ = _full_and_reduced(s2, st2, 1, prior1)
    print(f"two slides: K {k1} -> {k2}, n_fixed {s.n_fixed} -> {s2.n_fixed} -> {s3.n_fixed}, "
          f"disagreements {err1:.2e} {err2:.2e}")
    assert max(err1, err2) < IDENTITY
    assert (s2.n_fixed, s3.n_fixed) == (1, 0) and prior2 is not None and prior2.cost0 > 0


def test_a_prior_replaces_the_gauge():
    """n_fixed = 0 at lambda = 0: singular without a prior, solvable with one."""
    p, s, st0 = _case(SMALL)
    s0 = ba_ref.BAStructure(p.K, p.point_ptr, p.obs_cam, p.obs_uv, 0, p.n_poses)
    with pytest.raises(np.linalg.LinAlgError):
        ba_ref.gn_step(st0, s0, 0.0)
    step = pr.gn_step(st0, s0, 0.0, _synthetic_prior(s0, st0, 2))
    assert np.isfinite(step.dc).all()
