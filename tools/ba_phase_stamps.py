"""Diagnostic: per-phase shader-cycle shares of the BA K1 kernel (stamped build).

Run on the GPU box: ``VO_BA_STAMPS=1 python tools/ba_phase_stamps.py [cfg]``.
Phase shares come from a separate stamped instantiation of K1; read the shares,
not the absolute time (the stamps themselves perturb the schedule).
"""
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
os.environ.setdefault("VO_LIB_PATH", str(Path(__file__).resolve().parents[1] / "visualodometry_amd" / "lib" /
                                         "libvo_hip_stamps.so"))

from visualodometry_amd import _lib  # noqa: E402
from visualodometry_amd.ba import BASession  # noqa: E402
from visualodometry_amd.synthetic import make_ba_config  # noqa: E402

PHASES = ["load", "backsub", "lin_obs", "reduce", "eliminate", "schur_pairs", "write(rhs)", "schur_cams(U)", "-", "-",
          "n_obs", "n_te", "n_pts", "n_pairs", "n_slots", "n_cams"]
NPH = len(PHASES)
K3 = ["k3_setup", "k3_side_chol", "k3_backsub", "k3_tail", "k3_side_barrier", "k3_side_midbar", "k3_merge",
      "k3_separator", "k3_side_tasks", "k3_side_panel"]

cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg3"
p = make_ba_config(cfg)
ctx = _lib.context(0)
s = BASession(p.K, p.point_ptr, p.obs_cam, p.obs_uv, p.n_poses, p.n_fixed, 1.0, ctx)
s.set_state(p.poses_cw, p.points)
s.run_async(3)
s.synchronize()
out = np.zeros(len(PHASES) + len(K3), dtype=np.uint64)
n = _lib.check(ctx.lib.vo_ba_debug_stamps(ctx.handle, out.ctypes.data_as(_lib.C.POINTER(_lib.C.c_uint64)),
                                           len(out)))
tot = float(out[:8].sum())
print(cfg, s.plan_stats())
for k in range(min(n, 8)):
    print(f"{PHASES[k]:18s} {int(out[k]):14d} cycles (sum over WGs)  {100 * out[k] / tot:5.1f} %")
t3 = float(out[len(PHASES):].sum())
for k in range(len(PHASES), n):
    print(f"{K3[k - len(PHASES)]:18s} {int(out[k]):14d} cycles (one WG)  {100 * out[k] / max(t3, 1):5.1f} %")

# per-workgroup timeline of the last K1 launch (start/end absolute stamps)
st_ = s.plan_stats()
nseg = st_["chunks"] if st_["seg_obs"] == 1 else st_["segments"]  # rows: chunks of the one-wave K1
raw = np.zeros(nseg * NPH, dtype=np.uint64)
k = ctx.lib.vo_ba_debug_stamps(ctx.handle, raw.ctypes.data_as(_lib.C.POINTER(_lib.C.c_uint64)), -raw.size)
if k > 0:
    r = raw[:k].reshape(-1, NPH).astype(np.int64)
    xcc = (r[:, 15] >> 24) & 0xFF  # the stamping lane's XCD (s_memtime counts per XCD)
    simd = (r[:, 15] >> 32) & 3  # and its wave's SIMD
    r[:, 15] &= 0xFFFFFF
    t0, t1 = r[:, 8], r[:, 9]
    dur = t1 - t0
    t0 = t0.copy()
    t1 = t1.copy()
    for x in np.unique(xcc):  # times relative to each XCD's first start
        m = xcc == x
        b = t0[m].min()
        t0[m] -= b
        t1[m] -= b
    base = 0
    print(f"K1 workgroups: {len(r)} over {len(np.unique(xcc))} XCDs; per XCD (start spread, end of last) cyc:",
          [(int(t0[xcc == x].max()), int(t1[xcc == x].max())) for x in np.unique(xcc)])
    print(f"  duration min/median/p90/max: {dur.min()} {int(np.median(dur))} {int(np.percentile(dur, 90))} {dur.max()}")
    order = np.argsort(t0)
    print("  first 5 starts", (t0[order[:5]] - base).tolist(), " last 5 starts", (t0[order[-5:]] - base).tolist())
    slow = np.argsort(dur)[-5:]
    print("  slowest segments", slow.tolist(), dur[slow].tolist())
    nw = st_["chunks"] // max(st_["segments"], 1)
    if st_["seg_obs"] == 1 and nw > 1 and len(r) == nw * st_["segments"]:
        # workgroups of nw waves (rows = chunks, segment-major): the workgroup's duration, and what
        # follows the point where its last wave has only the rhs rows, the cost butterfly, the
        # barrier and the cross-chunk combine left (the row's start plus every phase but "write")
        g0 = r[:, 8].reshape(-1, nw)
        g1 = r[:, 9].reshape(-1, nw)
        pre = (r[:, 8] + r[:, :8].sum(axis=1) - r[:, 6]).reshape(-1, nw)
        wg = g1.max(axis=1) - g0.min(axis=1)
        after = g1.max(axis=1) - pre.max(axis=1)
        q = lambda v: f"{v.min()} {int(np.median(v))} {int(np.percentile(v, 90))} {v.max()}"
        print(f"K1 workgroups of {nw} waves: duration min/median/p90/max: {q(wg)}")
        print(f"  last wave's rhs start to the workgroup's end min/median/p90/max: {q(after)}")
        print("  waves' own work done (rhs start) after the workgroup's start, median per wave:",
              np.median(pre - g0.min(axis=1, keepdims=True), axis=0).astype(int).tolist())
        # which waves share a SIMD: the placements seen, and how often waves (0, 4) and (1, 5) pair up
        sw = simd.reshape(-1, nw)
        pats, cnt = np.unique(sw, axis=0, return_counts=True)
        top = np.argsort(-cnt)[:4]
        print("  SIMD of each wave, most frequent placements:",
              [(pats[i].tolist(), int(cnt[i])) for i in top], f"of {len(sw)} workgroups")
        if nw > 4:
            pair = np.all(sw[:, 4:] == sw[:, :nw - 4], axis=1)
            print(f"  waves 4.. on the SIMD of waves 0..: {int(pair.sum())} of {len(sw)} workgroups")
    if len(sys.argv) > 2:  # per-segment rows for cost-model fitting: duration, phases, counts
        np.savetxt(sys.argv[2], np.column_stack([dur, r[:, :8], r[:, 10:16]]), fmt="%d",
                   header="dur " + " ".join(PHASES[:8]) + " " + " ".join(PHASES[10:16]))
