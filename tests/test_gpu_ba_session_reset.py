"""A new ``vo_ba_setup`` leaves nothing of the context's previous session behind, whether that
session's window was larger or smaller: its robust cost, observation weights, LM termination
criteria, LM log and lazily uploaded tables (the problem-order observation arrays, the covariance
tables, the weight tables) are gone, and the new session computes bit for bit what it computes
on a context that never saw the other window.

Windows: ``make_ba_problem(8, 200, 11)`` and ``make_ba_problem(12, 800, 5)``, each in both roles,
so a stale table would be too short once and too long once.  Every comparison is exact: the
kernels are deterministic, and a plan built over a previous one is the plan a scratch setup builds.
"""

import functools

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from visualodometry_amd import _lib
from visualodometry_amd._lib import VoError
from visualodometry_amd.ba import BASession
from visualodometry_amd.synthetic import make_ba_problem

pytestmark = pytest.mark.gpu

LAM = 1.0
A, B = (8, 200, 11), (12, 800, 5)


@functools.lru_cache(maxsize=None)
def _problem(window):
    return make_ba_problem(*window)


def _session(window, ctx):
    p = _problem(window)
    return BASession(p.K, p.point_ptr, p.obs_cam, p.obs_uv, p.n_poses, p.n_fixed, LAM, ctx)


def _record(s, p):
    """Everything a plain session computes: a GN run, the read-outs at its state, an LM run."""
    out = {}
    s.set_state(p.poses_cw, p.points)
    rc, out["costs"] = s.run(3)
    assert rc == _lib.VO_OK
    out["poses"], out["points"] = s.get_state()
    out["err2"], out["depth"] = s.residuals()
    out["pose_cov"], out["point_cov"] = s.covariance(0.0)
    s.set_state(p.poses_cw, p.points)
    rc, out["lm_cost"], out["lm_lambda"], out["lm_trial"], out["lm_accepted"] = s.run_lm(3)
    assert rc == _lib.VO_OK
    out["lm_stop_info"] = np.array(s.lm_stop_info())
    out["lm_poses"], out["lm_points"] = s.get_state()
    return out


def _state_error(call):
    with pytest.raises(VoError) as e:
        call()
    assert e.value.code == _lib.VO_ERR_STATE


@pytest.mark.parametrize("first,second", [(A, B), (B, A)], ids=["small_then_large", "large_then_small"])
def test_setup_resets_the_session(ctx, first, second):
    p1, p2 = _problem(first), _problem(second)
    want = _record(_session(second, ctx), p2)  # 1: the second window on its own

    old = _session(first, ctx)  # 2: the first window, everything switched on
    old.set_state(p1.poses_cw, p1.points)
    old.set_robust(1.5)
    old.set_obs_weights(np.random.default_rng(7).choice([0.0, 0.5, 1.0, 2.0], size=len(p1.obs_cam)))
    old.set_lm_stop(ftol=1e-3)
    rc = old.run_lm(3)[0]
    assert rc == _lib.VO_OK
    old.residuals()
    old.covariance(0.0)
    old.cull(max_chi2=9.0)

    new = _session(second, ctx)  # 3: the second window again, a new session of the same context
    assert new.session != old.session
    _state_error(lambda: old.lm_log(0))  # 4
    _state_error(old.residuals)
    _state_error(old.obs_weights)
    _state_error(lambda: new.lm_log(0))  # no LM run on this session yet
    assert_array_equal(new.obs_weights(), np.ones(len(p2.obs_cam)))
    got = _record(new, p2)
    for k, v in want.items():
        assert_array_equal(got[k], v, err_msg=k)
    assert tuple(got["lm_stop_info"]) == (3, _lib.BA_LM_RAN_ALL)
