"""Cost of the pose prior and of the marginalisation (vo_ba_setup_prior, vo_ba_marginalize) on a
BASELINE config: one GN iteration of a session without a prior (the chained launch where the window
qualifies), the same with chaining switched off (a K1 launch and a solve launch per iteration: what
a session with a prior makes, less the prior's kernel), and with a prior over K poses; one
synchronous vo_ba_marginalize(n_drop = 1); and one SlidingWindowBA.optimize with and without
marginalize = 1.
Usage on the GPU box: python tools/ba_prior_timing.py [--configs cfg3] [--steps 4000] [--k 10]
                                                      [--out profiles/ba_prior.json]
An existing --out file keeps its other keys."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from visualodometry_amd import _lib  # noqa: E402
from visualodometry_amd.ba import BASession, BAWindow, PosePrior, SlidingWindowBA  # noqa: E402
from visualodometry_amd.synthetic import make_ba_config  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--configs", nargs="+", default=["cfg3"])
ap.add_argument("--steps", type=int, default=4000)  # about a quarter of a second per timed window at cfg3
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()

ctx = _lib.context(0)
LAM = 1.0


def make_prior(p, k):
    """Lambda = A^T A + I scaled to a diagonal of about 1e5 (the order of S's own at these sizes),
    eta = Lambda * 0.01 noise, poses0 the initial poses."""
    rng = np.random.default_rng(11)
    n = 6 * k
    A = rng.normal(size=(n, n)) * np.sqrt(1e5 / n)
    info = A.T @ A + np.eye(n)
    return PosePrior(info, info @ (0.01 * rng.normal(size=n)), p.poses_cw[p.n_fixed:p.n_fixed + k].copy(), 0.0)


def iteration_us(p, prior, no_chain=False):
    """(run_async(steps) + synchronize) / steps from the initial guess over --repeats timed windows:
    (median, min, max) in us, whether the last run was chained, whether the banded solver ran."""
    _lib.ba_testing_no_chain(ctx, no_chain)
    try:
        s = BASession(p.K, p.point_ptr, p.obs_cam, p.obs_uv, p.n_poses, p.n_fixed, LAM, ctx, prior=prior)
        t = []
        for k in range(args.repeats + 1):  # the first is the warm-up
            s.set_state(p.poses_cw, p.points)
            s.run_async(100)
            s.synchronize()
            t0 = time.perf_counter()
            s.run_async(args.steps)
            s.synchronize()
            t.append((time.perf_counter() - t0) / args.steps * 1e6)
            chained = _lib.ba_testing_last_run(ctx)[0]
            assert s.run(0)[0] == _lib.VO_OK
        t = t[1:]
        return [round(float(f(t)), 2) for f in (np.median, np.min, np.max)], bool(chained), bool(s.plan_stats()["band_solver"])
    finally:
        _lib.ba_testing_no_chain(ctx, False)


results = {}
for cfg in args.configs:
    p = make_ba_config(cfg)
    row = {"observations": int(p.obs_cam.size), "landmarks": int(p.n_points), "free_poses": int(p.n_poses - p.n_fixed),
           "prior_poses": args.k}
    for name, prior, nc in (("no_prior", None, False), ("no_prior_unchained", None, True), ("prior", make_prior(p, args.k), False)):
        (us, lo, hi), chained, banded = iteration_us(p, prior, nc)
        row[name + "_iteration_us"] = us
        row[name + "_iteration_us_min_max"] = [lo, hi]
        row[name + "_chained"] = chained
        row[name + "_banded"] = banded
    row["unchained_launches_us"] = round(row["no_prior_unchained_iteration_us"] - row["no_prior_iteration_us"], 2)
    row["prior_kernel_us"] = round(row["prior_iteration_us"] - row["no_prior_unchained_iteration_us"], 2)
    row["iteration_window"] = {"steps": args.steps, "repeats": args.repeats,
                               "note": "the two shares above are differences of medians of whole timed windows, not kernel-trace figures"}
    s = BASession(p.K, p.point_ptr, p.obs_cam, p.obs_uv, p.n_poses, p.n_fixed, LAM, ctx)
    s.set_state(p.poses_cw, p.points)
    assert s.run(5)[0] == _lib.VO_OK
    t = []
    for k in range(12):
        t0 = time.perf_counter()
        prior, mask = s.marginalize(1, LAM)
        t.append((time.perf_counter() - t0) * 1e6)
    row["marginalize_call_us_median"] = round(float(np.median(t[2:])), 1)
    row["marginalize_call_us_min_max"] = [round(float(min(t[2:])), 1), round(float(max(t[2:])), 1)]
    row["marginalize_prior_poses"] = 0 if prior is None else prior.n_poses
    row["marginalize_landmarks"] = int(mask.sum())
    obs_pt = np.repeat(np.arange(p.n_points), np.diff(p.point_ptr))
    win = BAWindow(p.poses_cw, p.points, p.obs_uv, p.obs_cam, obs_pt, n_fixed=p.n_fixed)
    ba = SlidingWindowBA(p.K, iters=args.iters, lam=LAM)
    plain, marg = [], []
    for k in range(args.repeats + 1):
        for n, acc in ((0, plain), (1, marg)):
            t0 = time.perf_counter()
            res = ba.optimize(win, marginalize=n)
            acc.append((time.perf_counter() - t0) * 1e3)
            assert res.status == "ok" and (n == 0 or res.prior is not None)
    row["optimize_ms_median"] = round(float(np.median(plain[1:])), 3)
    row["optimize_marginalize_ms_median"] = round(float(np.median(marg[1:])), 3)
    row["optimize_ms_min_max"] = [round(float(min(plain[1:])), 3), round(float(max(plain[1:])), 3)]
    row["optimize_marginalize_ms_min_max"] = [round(float(min(marg[1:])), 3), round(float(max(marg[1:])), 3)]
    row["optimize_iters"] = args.iters
    results[cfg] = row
out = {}
if args.out and Path(args.out).exists():
    out = json.loads(Path(args.out).read_text())
out["prior_timing"] = results
text = json.dumps(out, indent=1)
if args.out:
    Path(args.out).write_text(text + "\n")
print(text)
