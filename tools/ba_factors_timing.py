"""Cost of pose factors (vo_ba_setup_factors) on a BASELINE config: one GN iteration of a session
without factors (the chained launch where the window qualifies), the same with chaining switched off
(a K1 launch and a solve launch per iteration: what a session with factors or a prior makes, less
their kernel), with the chain of factors over all consecutive cameras, with the chain and a prior
over K poses, and with that prior alone.
Usage on the GPU box: python tools/ba_factors_timing.py [--configs cfg3] [--steps 4000] [--k 10]
                                                        [--out profiles/ba_factors.json]
An existing --out file keeps its other keys."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from visualodometry_amd import _lib  # noqa: E402
from visualodometry_amd.ba import BASession, PoseFactor, PosePrior  # noqa: E402
from visualodometry_amd.synthetic import make_ba_config  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--configs", nargs="+", default=["cfg3"])
ap.add_argument("--steps", type=int, default=4000)  # about a quarter of a second per timed window at cfg3
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()

ctx = _lib.context(0)
LAM = 1.0


def make_prior(p, k):
    """tools/ba_prior_timing.py's prior: Lambda = A^T A + I scaled to a diagonal of about 1e5."""
    rng = np.random.default_rng(11)
    n = 6 * k
    A = rng.normal(size=(n, n)) * np.sqrt(1e5 / n)
    info = A.T @ A + np.eye(n)
    return PosePrior(info, info @ (0.01 * rng.normal(size=n)), p.poses_cw[p.n_fixed:p.n_fixed + k].copy(), 0.0)


def make_chain(p):
    """One between factor per consecutive pair of cameras: the true relative pose, Lambda = 1e5 I."""
    T = p.poses_cw
    return [PoseFactor(k, k + 1, T[k] @ np.linalg.inv(T[k + 1]), 1e5 * np.eye(6)) for k in range(p.n_poses - 1)]


def iteration_us(p, prior, factors, no_chain=False):
    """(run_async(steps) + synchronize) / steps from the initial guess over --repeats timed windows:
    (median, min, max) in us, whether the last run was chained and its K1 + solve launches per
    iteration (the prior's / factors' kernel not counted), whether the banded solver ran."""
    _lib.ba_testing_no_chain(ctx, no_chain)
    try:
        s = BASession(p.K, p.point_ptr, p.obs_cam, p.obs_uv, p.n_poses, p.n_fixed, LAM, ctx, prior=prior, factors=factors)
        t = []
        for k in range(args.repeats + 1):  # the first is the warm-up
            s.set_state(p.poses_cw, p.points)
            s.run_async(100)
            s.synchronize()
            t0 = time.perf_counter()
            s.run_async(args.steps)
            s.synchronize()
            t.append((time.perf_counter() - t0) / args.steps * 1e6)
            chained, launches = _lib.ba_testing_last_run(ctx)
            assert s.run(0)[0] == _lib.VO_OK
        t = t[1:]
        return ([round(float(f(t)), 2) for f in (np.median, np.min, np.max)], bool(chained), launches / args.steps,
                bool(s.plan_stats()["band_solver"]))
    finally:
        _lib.ba_testing_no_chain(ctx, False)


results = {}
for cfg in args.configs:
    p = make_ba_config(cfg)
    chain, prior = make_chain(p), make_prior(p, args.k)
    row = {"observations": int(p.obs_cam.size), "landmarks": int(p.n_points), "free_poses": int(p.n_poses - p.n_fixed),
           "factors": len(chain), "prior_poses": args.k}
    sessions = (("no_factors", None, None, False), ("no_factors_unchained", None, None, True), ("chain", None, chain, False),
                ("chain_prior", prior, chain, False), ("prior", prior, None, False))
    for name, pr_, fs, nc in sessions:
        (us, lo, hi), chained, launches, banded = iteration_us(p, pr_, fs, nc)
        row[name + "_iteration_us"] = us
        row[name + "_iteration_us_min_max"] = [lo, hi]
        row[name + "_chained"] = chained
        row[name + "_k1_and_solve_launches_per_iteration"] = round(launches, 3)
        row[name + "_extra_kernel_launches_per_iteration"] = 0 if (pr_ is None and fs is None) else 1
        row[name + "_banded"] = banded
    row["chain_over_unchained_us"] = round(row["chain_iteration_us"] - row["no_factors_unchained_iteration_us"], 2)
    row["chain_over_no_factors_us"] = round(row["chain_iteration_us"] - row["no_factors_iteration_us"], 2)
    row["chain_prior_over_prior_us"] = round(row["chain_prior_iteration_us"] - row["prior_iteration_us"], 2)
    row["prior_over_unchained_us"] = round(row["prior_iteration_us"] - row["no_factors_unchained_iteration_us"], 2)
    row["iteration_window"] = {"steps": args.steps, "repeats": args.repeats,
                               "note": "the four shares above are differences of medians of whole timed windows, not kernel-trace figures"}
    results[cfg] = row
out = {}
if args.out and Path(args.out).exists():
    out = json.loads(Path(args.out).read_text())
out["factors_timing"] = results
text = json.dumps(out, indent=1)
if args.out:
    Path(args.out).write_text(text + "\n")
print(text)
