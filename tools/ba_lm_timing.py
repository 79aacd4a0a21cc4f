"""What a Levenberg-Marquardt trial costs: microseconds per LM iteration (run_lm_async between
synchronisations) against microseconds per GN iteration (run_async) of the same build on a
BASELINE config, regions alternating in one process, every region from the same state; then the
per-kernel event times of both (vo_profile_read), in a region of their own (the events add
launch overhead).
Usage on the GPU box: python tools/ba_lm_timing.py [config] [steps] [regions] [lam0] > out.json"""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from visualodometry_amd import _lib  # noqa: E402
from visualodometry_amd.ba import BASession  # noqa: E402
from visualodometry_amd.synthetic import make_ba_config  # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg3"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
regions = int(sys.argv[3]) if len(sys.argv) > 3 else 3
lam0 = float(sys.argv[4]) if len(sys.argv) > 4 else 1.0

p = make_ba_config(cfg)
ctx = _lib.context(0)
s = BASession(p.K, p.point_ptr, p.obs_cam, p.obs_uv, p.n_poses, p.n_fixed, 1.0, ctx)


def region(lm: bool, n: int) -> float:
    """Seconds of n iterations enqueued at once, from the initial state, after a warm-up of 50."""
    run = (lambda k: s.run_lm_async(k, lam0=lam0)) if lm else s.run_async
    s.set_state(p.poses_cw, p.points)
    run(50)
    s.synchronize()
    s.set_state(p.poses_cw, p.points)
    s.synchronize()
    t0 = time.perf_counter()
    run(n)
    s.synchronize()
    return time.perf_counter() - t0


us = {"gn": [], "lm": []}
status = []  # of every timed region: after a failed solve the later kernels return at once
accepted = 0
for r in range(regions + 1):  # region 0 warms every kernel up
    for lm in (False, True):
        dt = region(lm, steps)
        if lm:
            rc, _, _, _, acc = s.lm_log(steps)
            accepted = int(acc.sum())
        else:
            rc = s.run(0)[0]
        status.append(int(rc))
        if r:
            us["lm" if lm else "gn"].append(dt / steps * 1e6)

kernels = {}
for lm in (False, True):
    _lib.profile_enable(ctx, True)
    region(lm, 50)
    prof = _lib.profile_read(ctx)
    _lib.profile_enable(ctx, False)
    # the warm-up's launches are in the records too: times per launch, launches per iteration
    kernels["lm" if lm else "gn"] = {k: {"us_per_launch": round(ms / cnt * 1e3, 2), "launches_per_iteration": round(cnt / 100, 2)}
                                     for k, (ms, cnt) in prof.items()}

gn, lmu = float(np.median(us["gn"])), float(np.median(us["lm"]))
print(json.dumps({
    "config": cfg, "observations": int(p.obs_cam.size), "steps": steps, "lambda0": lam0, "region_status": status,
    "gn_us_per_iteration": [round(v, 2) for v in us["gn"]],
    "lm_us_per_iteration": [round(v, 2) for v in us["lm"]],
    "lm_over_gn": round(lmu / gn, 3),
    "lm_trials_accepted_of_steps": accepted,
    "kernel_events": kernels,
    "kernel_events_note": "under lm, ba_reduce is ba_lm_decide (timed under K2's id; K2 itself runs inside the "
                          "fused K3 launch when the window fuses, as cfg3 does) and ba_lin is the accumulate and the "
                          "back-substitute-only K1 together",
}))
