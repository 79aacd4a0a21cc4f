"""Cost of observation weights and device-side culling (vo_ba_set_obs_weights, vo_ba_cull) on BASELINE
configs: one GN iteration without weights (the chained launch where the window qualifies), the
same with a Huber cost, with weights (always a K1 launch of its own) and with weights and Huber;
one synchronous vo_ba_cull; and the schedule "R + 1 solves with a cull between them" end to end,
on the device (run_async / cull_async, one synchronisation at the end) against the same schedule
through the host: residual read-out, mask in numpy, a new vo_ba_setup on the surviving observations.
Usage on the GPU box: python tools/ba_weights_timing.py [--configs cfg3 cfg4] [--steps 200]
                                                        [--out profiles/ba_weights.json]
An existing --out file keeps its other keys."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from visualodometry_amd import _lib  # noqa: E402
from visualodometry_amd.ba import BASession  # noqa: E402
from visualodometry_amd.synthetic import make_ba_config  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--configs", nargs="+", default=["cfg3", "cfg4"])
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--chi2", type=float, default=9.0)
ap.add_argument("--huber", type=float, default=2.0)
ap.add_argument("--out", default=None)
args = ap.parse_args()

ctx = _lib.context(0)
LAM = 1.0


def iteration_us(p, huber, w):
    """Median over --repeats of (run_async(steps) + synchronize) / steps from the initial guess."""
    s = BASession(p.K, p.point_ptr, p.obs_cam, p.obs_uv, p.n_poses, p.n_fixed, LAM, ctx, huber=huber)
    if w is not None:
        s.set_obs_weights(w)
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
    return round(float(np.median(t[1:])), 2), bool(chained)


def host_mask(err2, z, ptr, chi2):
    """vo_ba_cull's rule for unit weights and min_track = 2, in numpy."""
    keep = np.isfinite(err2) & np.isfinite(z) & (z > 0.0) & ~(err2 > chi2)
    obs_pt = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    n = np.bincount(obs_pt[keep], minlength=ptr.size - 1)
    return keep & (n >= 2)[obs_pt]


def schedule_device(p):
    s = BASession(p.K, p.point_ptr, p.obs_cam, p.obs_uv, p.n_poses, p.n_fixed, LAM, ctx, huber=args.huber)
    s.set_state(p.poses_cw, p.points)
    t0 = time.perf_counter()
    for k in range(args.rounds + 1):
        s.run_async(args.iters)
        if k < args.rounds:
            s.cull_async(args.chi2, 0.0, 2)
    P, X = s.get_state()
    t = (time.perf_counter() - t0) * 1e3
    return t, int((s.obs_weights() > 0).sum())


def schedule_host(p):
    ptr, cam, uv = np.asarray(p.point_ptr), p.obs_cam, p.obs_uv
    P, X = p.poses_cw, p.points
    s = BASession(p.K, ptr, cam, uv, p.n_poses, p.n_fixed, LAM, ctx, huber=args.huber)
    s.set_state(P, X)
    t0 = time.perf_counter()
    for k in range(args.rounds + 1):
        s.run_async(args.iters)
        if k < args.rounds:
            err2, z = s.residuals()
            P, X = s.get_state()
            keep = host_mask(err2, z, ptr, args.chi2)
            obs_pt = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))[keep]
            live = np.bincount(obs_pt, minlength=ptr.size - 1) > 0  # landmarks without a track leave the window
            cam, uv, X = cam[keep], uv[keep], X[live]
            ptr = np.concatenate([[0], np.cumsum(np.bincount(obs_pt, minlength=live.size)[live])]).astype(np.int32)
            s = BASession(p.K, ptr, cam, uv, p.n_poses, p.n_fixed, LAM, ctx, huber=args.huber)
            s.set_state(P, X)
    P, X = s.get_state()
    return (time.perf_counter() - t0) * 1e3, int(cam.size)


results = {}
for cfg in args.configs:
    p = make_ba_config(cfg)
    M = p.obs_cam.size
    w = np.random.default_rng(3).uniform(0.25, 4.0, M)
    row = {"observations": int(M), "landmarks": int(p.n_points), "free_poses": int(p.n_poses - p.n_fixed)}
    for name, hub, ww in (("unweighted", 0.0, None), ("huber", args.huber, None), ("weighted", 0.0, w),
                          ("weighted_huber", args.huber, w)):
        us, chained = iteration_us(p, hub, ww)
        row[name + "_iteration_us"] = us
        row[name + "_chained"] = chained
    s = BASession(p.K, p.point_ptr, p.obs_cam, p.obs_uv, p.n_poses, p.n_fixed, LAM, ctx)
    s.set_state(p.poses_cw, p.points)
    assert s.run(5)[0] == _lib.VO_OK
    t = []
    for k in range(12):  # nothing is culled (every rule off but finiteness): the same kernels, a repeatable state
        t0 = time.perf_counter()
        n_culled, _ = s.cull(0.0, -1e30, 0)
        t.append((time.perf_counter() - t0) * 1e6)
        assert n_culled == 0
        s.set_obs_weights(np.ones(M))  # (keeps the session weighted, so every call makes the same launches)
    row["cull_call_us_median"] = round(float(np.median(t[2:])), 1)
    dev, host = [], []
    for k in range(args.repeats + 1):
        td, nd = schedule_device(p)
        th, nh = schedule_host(p)
        dev.append(td)
        host.append(th)
    row["schedule"] = {"rounds": args.rounds, "iters": args.iters, "chi2": args.chi2, "huber": args.huber,
                       "device_ms_median": round(float(np.median(dev[1:])), 3),
                       "host_ms_median": round(float(np.median(host[1:])), 3),
                       "active_after_device": nd, "active_after_host": nh}
    results[cfg] = row
out = {}
if args.out and Path(args.out).exists():
    out = json.loads(Path(args.out).read_text())
out["weights_timing"] = results
text = json.dumps(out, indent=1)
if args.out:
    Path(args.out).write_text(text + "\n")
print(text)
