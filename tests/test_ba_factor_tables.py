"""The pose factors' host tables (csrc/ba_tables.h ``pose_factor_error`` / ``factor_free_cams`` /
``factor_lower_first`` / ``factor_marginalised``, csrc/ba_plan.h ``build_profile``'s factor rows) checked
on the host by ``ba_tables_check <window> <seg_chunks> factors``: an empty factor list leaves every
profile array and the plan digest as they are; a chain over all cameras keeps the bandwidth; a factor
between the first and the last free pose spans the profile; every factor's slab and rhs rows lie
behind K1's sources and ahead of the prior's, in factor order.  No GPU needed."""

import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

from visualodometry_amd.synthetic import make_ba_problem

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "visualodometry_amd" / "lib" / "ba_tables_check"

SMALL, NARROW = ((8, 300, 21), {}), ((16, 400, 5), {"max_track": 4})


@pytest.fixture(scope="module")
def exe():
    subprocess.run(["make", "-s", "-C", str(ROOT / "visualodometry_amd" / "csrc"), "../lib/ba_tables_check"], check=True)
    return EXE


def check(exe, p, seg_chunks):
    with tempfile.TemporaryDirectory() as d:
        fi = os.path.join(d, "in")
        with open(fi, "wb") as f:
            np.array([p.n_poses, len(p.point_ptr) - 1, len(p.obs_cam), p.n_fixed, 1], np.int32).tofile(f)
            np.asarray(p.point_ptr, np.int32).tofile(f)
            np.asarray(p.obs_cam, np.int32).tofile(f)
            np.asarray(p.obs_uv, np.float32).tofile(f)
        out = subprocess.run([str(exe), fi, str(seg_chunks), "factors"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("factors ok"), out.stdout + out.stderr
    return [int(v) for v in out.stdout.split()[2:]]


@pytest.mark.parametrize("seg_chunks", [1, 6])
@pytest.mark.parametrize("window", [SMALL, NARROW, ((3, 40, 2), {}), ((30, 3000, 11), {})])
def test_factor_tables(exe, window, seg_chunks):
    args, kw = window
    p = make_ba_problem(*args, **kw)
    F, w, w_chain, w_far, rows = check(exe, p, seg_chunks)
    assert F == p.n_poses - p.n_fixed
    assert w_chain == w, "a chain of consecutive keyframes widened the profile"
    assert w_far == max(F - 1, 0)
    # the chain (n_poses - 1 pairs), the duplicate of its last pair and the unary factor: three slab
    # rows per factor between two free poses, one per other factor with a free endpoint
    if F >= 2:
        assert rows == 3 * F + 2


def test_narrow_far_factor_spans_13(exe):
    """A factor between free poses 0 and 13 of NARROW, whose own bandwidth the banded solver holds,
    gives span 13: beyond the banded solver's 9."""
    args, kw = NARROW
    F, w, w_chain, w_far, _ = check(exe, make_ba_problem(*args, **kw), 6)
    assert (F, w_far) == (14, 13) and w_chain == w <= 9


def test_plan_digests_unchanged():
    """The digests of tests/golden/plan_digests.json are still what the planner gives."""
    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    try:
        import make_plan_digests
    finally:
        sys.path.pop(0)
    want = json.loads((ROOT / "tests" / "golden" / "plan_digests.json").read_text())
    assert make_plan_digests.digests() == want
