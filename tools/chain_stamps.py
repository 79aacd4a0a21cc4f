"""Diagnostic: realtime stamps of a chained solve launch (stamped build): when the solver publishes
and where the next iteration's K1 workgroups are at that time.

Build the stamped library first (CPU container):
  make -C visualodometry_amd/csrc OUT=../lib/libvo_hip_stamps.so OBJDIR=../lib/obj_stamps \
       EXTRA=-DVO_BA_STAMPS=1 ../lib/libvo_hip_stamps.so
then on the GPU box: ``python tools/chain_stamps.py [cfg] [replicas]`` (replicas: 1 or 8 publish
words; default both).  Values are the last chained launch's of a run of 3, in ns (s_memrealtime,
100 MHz); stamps perturb the schedule a little.  A stamped build chains only here
(vo_ba_testing_chain_stamps): tools/band_stamps.py and tools/ba_phase_stamps.py keep the split sequence.
"""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
os.environ.setdefault("VO_LIB_PATH", str(ROOT / "visualodometry_amd" / "lib" / "libvo_hip_stamps.so"))

from visualodometry_amd import _lib  # noqa: E402
from visualodometry_amd.ba import BASession  # noqa: E402
from visualodometry_amd.synthetic import make_ba_config  # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg3"
reps = [int(sys.argv[2])] if len(sys.argv) > 2 else [1, 8]
p = make_ba_config(cfg)
ctx = _lib.context(0)
_lib.ba_testing_chain_stamps(ctx, True)
for r in reps:
    _lib.ba_testing_chain_poll(ctx, r)
    s = BASession(p.K, p.point_ptr, p.obs_cam, p.obs_uv, p.n_poses, p.n_fixed, 1.0, ctx)
    s.set_state(p.poses_cw, p.points)
    nseg = s.plan_stats()["segments"]
    s.run_async(5)  # warm
    s.synchronize()
    rows = []
    for _ in range(5):
        s.run_async(3)
        s.synchronize()
        chained, launches = _lib.ba_testing_last_run(ctx)
        st = _lib.ba_testing_chain_stamps(ctx, True, 2 + 4 * nseg).astype(np.int64)
        if not chained or len(st) < 2 + 4 * nseg:
            print(cfg, "not chained (or not a stamped build): chained", chained, "stamps", len(st))
            sys.exit(0)
        pub, t0 = st[0], st[1]
        k1 = st[2:].reshape(nseg, 4)
        rows.append([(pub - t0) * 10, np.median(k1[:, 0] - t0) * 10, np.median(k1[:, 1] - t0) * 10,
                     np.max(k1[:, 1] - t0) * 10, np.median(k1[:, 2] - pub) * 10, np.max(k1[:, 2] - pub) * 10,
                     np.median(k1[:, 3] - pub) * 10, np.max(k1[:, 3] - pub) * 10, np.max(k1[:, 3] - t0) * 10])
    late = np.nonzero(k1[:, 0] - t0 > 1000)[0]  # (last launch) workgroups that started > 10 us in
    print(f"  last launch: K1 start p50/p90/p99/max {[int(np.percentile(k1[:, 0] - t0, q)) * 10 for q in (50, 90, 99, 100)]} ns,"
          f" {len(late)} started late: {late[:16].tolist()} at {((k1[late, 0] - t0) * 10)[:16].tolist()}")
    m = np.median(np.array(rows), axis=0)
    print(f"{cfg} {nseg} K1 workgroups, {r} publish word(s), medians over 5 launches (ns; K1 figures: median / max over workgroups)")
    print(f"  solver published, from the solver's start   {m[0]:8.0f}")
    print(f"  K1 start, from the solver's start           {m[1]:8.0f}")
    print(f"  K1 prefix done, from the solver's start     {m[2]:8.0f} / {m[3]:.0f}")
    print(f"  K1 gate passed, from published              {m[4]:8.0f} / {m[5]:.0f}")
    print(f"  K1 end, from published                      {m[6]:8.0f} / {m[7]:.0f}")
    print(f"  launch span (last K1 end, from the solver's start) {m[8]:8.0f}")
