"""Golden for tests/test_gpu_ba_step_ends.py: what the build of commit ``PARENT`` computes at the
two ends of a GN step, recorded once on the GPU box and compared bit for bit from then on.

The three changes the test guards (K1's cross-chunk combine started early by the waves that are
done, the banded solver's pose update stored as contiguous rows by every thread, the G blocks
of the bottom side's pseudo rows formed under the separator's back substitution) move work
between waves and in time; none changes a floating-point operation or its order.  So the
results of the commit before them are the reference, and equality is exact.

    python tests/golden/make_ba_step_ends.py --search        # CPU: the smallest K1 window (below)
    VO_LIB_PATH=<parent build's libvo_hip.so> python tests/golden/make_ba_step_ends.py --parent <hash>

``--search`` walks ``make_ba_problem(n_poses, n_points, seed)`` by n_points (steps of 100), then
n_poses (4..8), then seed (0..3) and prints the first window whose six-chunk plan (host planner,
``ba_plan_check ... 6 combine``) has all four of the combine's cases: a segment with fewer than
four non-empty chunks, one with a slot held only by chunks 4/5, one with a slot held only by
chunks 0..3, and one with all six chunks non-empty.  ``K1_WINDOW`` is that window.

The fixture keeps the costs (and the small windows' poses) in full and the larger arrays (the
landmarks, the layout windows' poses and dc) as SHA-256 digests of their bytes: equality of a
digest is equality of every bit, in a few KB.
"""

from __future__ import annotations

import hashlib
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
OUT = ROOT / "tests" / "golden" / "ba_step_ends_parent.npz"
PLAN_CHECK = ROOT / "visualodometry_amd" / "lib" / "ba_plan_check"

K1_WINDOW = dict(n_poses=8, n_points=1300, seed=3)  # 16 six-chunk segments: 4 short, 1 late-only, 4 early-only, 11 full
K1_VARIANTS = (1, 2, 3, 4, 5, 6, 0)
K1_ITERS = 3
K1_FULL = ("rc", "costs", "poses")  # kept in full in the fixture (the rest as digests)
NOTSPD_FULL = ("rc", "dc", "poses")
# the solver's tail: (name, n_poses, max_track, n_fixed, layout) at test_band_layout_modes' sizes,
# every pose count off a multiple of 16, and one odd count
TAIL_CASES = (("full50_f2", 50, 8, 2, "full"), ("full50_f1", 50, 8, 1, "full"), ("full53_f1", 53, 8, 1, "full"),
              ("split100_f2", 100, 8, 2, "split"), ("split100_f1", 100, 8, 1, "split"),
              ("ring200_f2", 200, 8, 2, "ring"), ("ring200_f1", 200, 8, 1, "ring"))


def digest(a) -> np.ndarray:
    return np.array(hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).hexdigest())


def record(r: dict, full=("rc", "rc2", "costs", "cost0")) -> dict:
    """A run's results as the fixture keeps them: ``full`` as they are, the rest as digests."""
    return {k: (a if k in full else digest(a)) for k, a in r.items()}


def combine_cases(p, seg_chunks: int = 6):
    """(segments, [short, late-only, early-only, full]) of the window's wave plan (host only)."""
    with tempfile.TemporaryDirectory() as d:
        fi = os.path.join(d, "in")
        with open(fi, "wb") as f:
            np.array([p.n_poses, len(p.point_ptr) - 1, len(p.obs_cam), p.n_fixed, 1], np.int32).tofile(f)
            np.asarray(p.point_ptr, np.int32).tofile(f)
            np.asarray(p.obs_cam, np.int32).tofile(f)
            np.asarray(p.obs_uv, np.float32).tofile(f)
        out = subprocess.run([str(PLAN_CHECK), fi, str(seg_chunks), "combine"], capture_output=True, text=True)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and len(lines) == 2 and lines[0].startswith("ok") and lines[1].startswith("combine"), \
        out.stdout + out.stderr
    return int(lines[0].split()[2]), [int(v) for v in lines[1].split()[1:]]


def k1_window():
    from visualodometry_amd.synthetic import make_ba_problem

    return make_ba_problem(K1_WINDOW["n_poses"], K1_WINDOW["n_points"], K1_WINDOW["seed"])


def tail_window(n_poses, max_track, n_fixed):
    from visualodometry_amd.synthetic import make_ba_problem

    return make_ba_problem(n_poses, 30 * n_poses, 5 + n_poses, max_track=max_track, n_fixed=n_fixed)


def not_spd_window():
    """tests/test_gpu_ba.py test_not_spd_reported's: a free camera without observations, no damping."""
    from visualodometry_amd.synthetic import make_ba_problem

    p = make_ba_problem(6, 100, 41)
    cam = p.obs_cam.copy()
    cam[cam == 5] = 4
    return p, cam


def _session(p, ctx, lam=1.0, cam=None):
    from visualodometry_amd.ba import BASession

    s = BASession(p.K, p.point_ptr, p.obs_cam if cam is None else cam, p.obs_uv, p.n_poses, p.n_fixed, lam, ctx)
    s.set_state(p.poses_cw, p.points)
    return s


def run_k1(ctx, variant: int):
    """K1 variant (vo_ba_testing_k1) on the K1 window: plan stats and costs, poses, landmarks."""
    from visualodometry_amd import _lib

    _lib.ba_testing_k1(ctx, variant)
    try:
        s = _session(k1_window(), ctx)
        st = s.plan_stats()
        rc, costs = s.run(K1_ITERS)
        P, X = s.get_state()
    finally:
        _lib.ba_testing_k1(ctx, 0)
    return st, {"rc": np.int64(rc), "costs": costs, "poses": P, "points": X}


def run_tail(ctx, n_poses, max_track, n_fixed):
    """One exported GN step (dc) and two more iterations on a layout window."""
    s = _session(tail_window(n_poses, max_track, n_fixed), ctx)
    st = s.plan_stats()
    rc, _, _, dc, cost = s.gn_step()
    P1, _ = s.get_state()
    rc2, costs = s.run(2)
    P, X = s.get_state()
    return st, {"rc": np.int64(rc), "rc2": np.int64(rc2), "dc": dc, "cost0": np.float64(cost), "poses1": P1,
                "costs": costs, "poses": P, "points": X}


def run_not_spd(ctx):
    p, cam = not_spd_window()
    s = _session(p, ctx, lam=0.0, cam=cam)
    rc, _, _, dc, _ = s.gn_step()
    P, X = s.get_state()
    return {"rc": np.int64(rc), "dc": dc, "poses": P, "points": X}


def search() -> None:
    from visualodometry_amd.synthetic import make_ba_problem

    for n_points in range(100, 4001, 100):
        for n_poses in range(4, 9):
            for seed in range(4):
                segs, cases = combine_cases(make_ba_problem(n_poses, n_points, seed))
                if all(c > 0 for c in cases):
                    print(f"n_poses {n_poses} n_points {n_points} seed {seed}: {segs} segments, "
                          f"short/late-only/early-only/full {cases}")
                    return
    print("no window found")


def main() -> None:
    if "--search" in sys.argv:
        search()
        return
    if "--parent" not in sys.argv:
        raise SystemExit(__doc__)
    parent = sys.argv[sys.argv.index("--parent") + 1]
    from visualodometry_amd import _lib

    ctx = _lib.context(0)
    out = {"parent": np.array(parent), "k1_window": np.array([K1_WINDOW[k] for k in ("n_poses", "n_points", "seed")])}
    for v in K1_VARIANTS:
        st, r = run_k1(ctx, v)
        print("k1 variant", v, "chunks/segments", st["chunks"], st["segments"], "costs", r["costs"])
        for k, a in record(r, K1_FULL).items():
            out[f"k1_{v}_{k}"] = a
    for name, n_poses, max_track, n_fixed, mode in TAIL_CASES:
        st, r = run_tail(ctx, n_poses, max_track, n_fixed)
        assert st["band_mode"] == mode and r["rc"] == _lib.VO_OK and r["rc2"] == _lib.VO_OK, (name, st, r["rc"])
        print("tail", name, st["band_mode"], "costs", r["costs"])
        for k, a in record(r).items():
            out[f"tail_{name}_{k}"] = a
    r = run_not_spd(ctx)
    assert r["rc"] == _lib.VO_ERR_NOT_SPD, r["rc"]
    print("not SPD: dc", np.abs(r["dc"]).max())
    for k, a in record(r, NOTSPD_FULL).items():
        out[f"notspd_{k}"] = a
    dst = Path(sys.argv[sys.argv.index("--out") + 1]) if "--out" in sys.argv else OUT
    dst.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(dst, **out)
    print(f"wrote {dst} ({dst.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
