"""Call time of the covariance read-out (vo_ba_covariance) on BASELINE configs, next to one GN
iteration of the same build: the median of warm calls for poses only (no landmark output) and for
poses plus landmarks, after a few GN iterations from the initial guess.
Usage on the GPU box: python tools/ba_cov_timing.py [--configs cfg3 cfg4] [--calls 24] [--lam 1.0]
                                                    [--out profiles/ba_covariance.json]
An existing --out file keeps its other keys (the parent-versus-branch bench values recorded there)."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from visualodometry_amd import _lib  # noqa: E402
from visualodometry_amd._lib import check, ptr  # noqa: E402
from visualodometry_amd.ba import BASession  # noqa: E402
from visualodometry_amd.synthetic import make_ba_config  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--configs", nargs="+", default=["cfg3", "cfg4"])
ap.add_argument("--calls", type=int, default=24)
ap.add_argument("--lam", type=float, default=1.0)  # the bench's damping; 0 is the GN covariance
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.calls >= 22, "two warm-up calls and a median of at least 20"

ctx = _lib.context(0)
results = {}
for cfg in args.configs:
    p = make_ba_config(cfg)
    s = BASession(p.K, p.point_ptr, p.obs_cam, p.obs_uv, p.n_poses, p.n_fixed, 1.0, ctx)
    s.set_state(p.poses_cw, p.points)
    F = p.n_poses - p.n_fixed
    pose, pts = np.empty((F, 6, 6)), np.empty((p.n_points, 3, 3))
    # one GN iteration of this build: run_async timed between synchronisations, after a warm-up
    s.run_async(100)
    s.synchronize()
    t0 = time.perf_counter()
    s.run_async(args.steps)
    s.synchronize()
    gn_us = (time.perf_counter() - t0) / args.steps * 1e6
    assert s.run(0)[0] == _lib.VO_OK
    s.set_state(p.poses_cw, p.points)
    assert s.run(5)[0] == _lib.VO_OK

    def call(with_points):
        t = time.perf_counter()
        check(ctx.lib.vo_ba_covariance(ctx.handle, s.session, args.lam, ptr(pose, C.c_double), None,
                                       ptr(pts, C.c_double) if with_points else None), "vo_ba_covariance")
        return (time.perf_counter() - t) * 1e3

    t_pose = [call(False) for _ in range(args.calls)]
    t_both = [call(True) for _ in range(args.calls)]
    sd = np.sqrt(np.diagonal(pts, axis1=1, axis2=2).max(axis=1))
    results[cfg] = {
        "free_poses": F, "landmarks": int(p.n_points), "observations": int(p.obs_cam.size), "lambda": args.lam,
        "calls": args.calls - 2,
        "gn_iteration_us": round(gn_us, 2),
        "covariance_poses_first_call_ms": round(t_pose[0], 3),
        "covariance_poses_ms_median": round(float(np.median(t_pose[2:])), 3),
        "covariance_poses_and_landmarks_ms_median": round(float(np.median(t_both[2:])), 3),
        "frozen_landmarks": int(np.isnan(sd).sum()),
        "landmark_sd_median": round(float(np.nanmedian(sd)), 4),
        "landmark_sd_max": round(float(np.nanmax(sd)), 4),
    }
out = {}
if args.out and Path(args.out).exists():
    out = json.loads(Path(args.out).read_text())
out["covariance_timing"] = results
text = json.dumps(out, indent=1)
if args.out:
    Path(args.out).write_text(text + "\n")
print(text)
