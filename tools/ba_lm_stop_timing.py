"""What a trial behind a device-side stop costs: microseconds per live LM trial (no termination
criterion: every enqueued trial runs) against microseconds per dead trial (ftol = 0.999 stops the
loop at its first accepted step; the trials enqueued behind it leave at their first test of the
status word) of the same build on a BASELINE config, regions alternating in one process, every
region from the same state; then the per-kernel event times of a stopped region (vo_profile_read),
in a region of their own (the events add launch overhead).
Usage on the GPU box: python tools/ba_lm_stop_timing.py [config] [steps] [regions] [lam0] > out.json"""
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
FTOL = 0.999

p = make_ba_config(cfg)
ctx = _lib.context(0)
s = BASession(p.K, p.point_ptr, p.obs_cam, p.obs_uv, p.n_poses, p.n_fixed, 1.0, ctx)


def region(stop: bool, n: int) -> float:
    """Seconds of n trials enqueued at once, from the initial state, after a warm-up of 50."""
    s.set_lm_stop(FTOL if stop else 0.0)
    s.set_state(p.poses_cw, p.points)
    s.run_lm_async(50, lam0=lam0)
    s.synchronize()
    s.set_state(p.poses_cw, p.points)
    s.synchronize()
    t0 = time.perf_counter()
    s.run_lm_async(n, lam0=lam0)
    s.synchronize()
    return time.perf_counter() - t0


sec = {"live": [], "stopped": []}
infos = []  # (trials, reason) of every timed region
for r in range(regions + 1):  # region 0 warms every kernel up
    for stop in (False, True):
        dt = region(stop, steps)
        infos.append(list(s.lm_stop_info()))
        if r:
            sec["stopped" if stop else "live"].append(dt)
trials = infos[-1][0]  # of a stopped region: the same in every one (same state, same schedule)

_lib.profile_enable(ctx, True)
region(True, 50)
prof = _lib.profile_read(ctx)
_lib.profile_enable(ctx, False)
profiled_trials = s.lm_stop_info()[0]
# the warm-up's launches are in the records too: 100 trials, all but 2 * profiled_trials of them dead
kernels = {k: {"us_per_launch": round(ms / cnt * 1e3, 2), "launches_per_trial": round(cnt / 100, 2)}
           for k, (ms, cnt) in prof.items()}

live_us = float(np.median(sec["live"])) / steps * 1e6
# a stopped region: `trials` live trials, then steps - trials dead ones
dead_us = (float(np.median(sec["stopped"])) * 1e6 - trials * live_us) / max(1, steps - trials)
print(json.dumps({
    "config": cfg, "observations": int(p.obs_cam.size), "steps": steps, "lambda0": lam0, "ftol": FTOL,
    "region_trials_reason": infos,
    "live_region_us": [round(v * 1e6, 1) for v in sec["live"]],
    "stopped_region_us": [round(v * 1e6, 1) for v in sec["stopped"]],
    "live_us_per_trial": round(live_us, 2),
    "dead_us_per_trial": round(dead_us, 2),
    "dead_over_live": round(dead_us / live_us, 3),
    "stopped_kernel_events": kernels,
    "stopped_kernel_events_note": f"100 trials enqueued (warm-up and region), {2 * profiled_trials} of them live; "
                                  "ba_reduce is ba_lm_decide and the run's one ba_lm_finish (timed under K2's id; K2 "
                                  "itself runs inside the fused K3 launch when the window fuses, as cfg3 does), ba_lin "
                                  "the accumulate and the back-substitute-only K1 together",
}))
