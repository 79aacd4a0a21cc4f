"""GN-iterations/s of the BA under the Huber cost and the call time of the residual read-out, on a
BASELINE config with 5 % gross outliers (5 % of the measurements moved 30-100 px): run_async
timed between synchronisations, delta = 0 and delta > 0 regions alternating in one process.
Usage on the GPU box: python tools/ba_robust_timing.py [config] [delta] [steps] [regions] > out.json"""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from visualodometry_amd import _lib  # noqa: E402
from visualodometry_amd.ba import BASession  # noqa: E402
from visualodometry_amd.synthetic import BA_CONFIGS, make_ba_config  # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg3"
delta = float(sys.argv[2]) if len(sys.argv) > 2 else 2.0
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 200
regions = int(sys.argv[4]) if len(sys.argv) > 4 else 3

p = make_ba_config(cfg)
rng = np.random.default_rng(100 + BA_CONFIGS[cfg][2])
uv = p.obs_uv.copy()
k = int(0.05 * uv.shape[0])
idx = rng.permutation(uv.shape[0])[:k]
ang, mag = rng.uniform(0, 2 * np.pi, k), rng.uniform(30, 100, k)
uv[idx] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], -1).astype(np.float32)

ctx = _lib.context(0)
s = BASession(p.K, p.point_ptr, p.obs_cam, uv, p.n_poses, p.n_fixed, 1.0, ctx)
rate = {0.0: [], delta: []}
status = []  # of every timed region: after a failed solve the later kernels return at once
for r in range(regions + 1):  # region 0 warms both kernels up
    for d in (0.0, delta):
        s.set_state(p.poses_cw, p.points)  # every region iterates from the same state
        s.set_robust(d)
        s.run_async(100)
        s.synchronize()
        t0 = time.perf_counter()
        s.run_async(steps)
        s.synchronize()
        dt = time.perf_counter() - t0
        status.append(int(s.run(0)[0]))
        if r:
            rate[d].append(steps / dt)
readout = []
for r in range(12):
    t0 = time.perf_counter()
    err2, depth = s.residuals()
    readout.append((time.perf_counter() - t0) * 1e3)
print(json.dumps({
    "config": cfg, "observations": int(uv.shape[0]), "outliers": k, "steps": steps, "region_status": status,
    "gn_iters_per_s_plain": [round(v, 1) for v in rate[0.0]],
    f"gn_iters_per_s_huber_{delta:g}": [round(v, 1) for v in rate[delta]],
    "residuals_first_call_ms": round(readout[0], 3),
    "residuals_call_ms_median": round(float(np.median(readout[2:])), 3),
    "observations_beyond_delta": int((err2 > delta * delta).sum()),
}))
