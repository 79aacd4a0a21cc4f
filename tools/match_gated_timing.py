"""Latency of the projection-gated matcher (matcher.match_gated / vo_match_gated) at a frame-sized shape:
4000 landmarks against 4000 keypoints, dim 128, a KITTI-size image, radius 15 px.

Reports the host-array call and the device-pointer call (train descriptors and keypoints resident in
HBM) as the median of repeated timed regions, each region a run of calls that ends in the call's own
stream synchronise; the per-kernel HIP-event times come from a region of their own (the events slow
the host).  The dense matcher (match_knn2_ratio, same build, same descriptors) is timed the same way
for scale.  Results are checked against each other, not against the CPU restatement (tests do that).
Writes one JSON object to --out and prints it.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from visualodometry_amd import _lib, matcher  # noqa: E402
from visualodometry_amd._lib import C, ptr  # noqa: E402

SIZE = (1241, 376)


def scene(n0, n1, dim, seed, found=0.6, jitter=4.0):
    """SIFT-like integers: a share of the landmarks seen as jittered keypoints with noisy copies of
    their descriptors, the rest of the keypoints clutter."""
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(0, SIZE[0], n0), rng.uniform(0, SIZE[1], n0)], axis=1)
    d0 = rng.integers(0, 256, (n0, dim)).astype(np.float32)
    n_found = min(int(found * n0), n1)
    seen = rng.permutation(n0)[:n_found]
    kp = np.concatenate([pos[seen] + rng.normal(0, jitter, (n_found, 2)),
                         np.stack([rng.uniform(0, SIZE[0], n1 - n_found), rng.uniform(0, SIZE[1], n1 - n_found)], 1)])
    d1 = np.concatenate([np.clip(np.rint(d0[seen] + rng.normal(0, 8.0, (n_found, dim))), 0, 255),
                         rng.integers(0, 256, (n1 - n_found, dim))]).astype(np.float32)
    order = rng.permutation(n1)
    pred = (pos + rng.normal(0, 1.5, pos.shape)).astype(np.float32)
    return d0, pred, np.ascontiguousarray(d1[order]), np.ascontiguousarray(kp[order].astype(np.float32))


def regions(fn, calls, repeats):
    """Median and spread (ms per call) over `repeats` timed regions of `calls` synchronous calls."""
    out = []
    for _ in range(repeats):
        t = time.perf_counter()
        for _ in range(calls):
            fn()
        out.append((time.perf_counter() - t) / calls * 1e3)
    return {"median_ms": round(float(np.median(out)), 4), "min_ms": round(min(out), 4), "max_ms": round(max(out), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n0", type=int, default=4000)
    ap.add_argument("--n1", type=int, default=4000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--radius", type=float, default=15.0)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default="profiles/match_gated.json")
    a = ap.parse_args()
    ctx = _lib.context(0)
    d0, pred, d1, kp1 = scene(a.n0, a.n1, a.dim, 7)
    kw = dict(ratio=0.8, max_dist=300.0, unique=True, image_size=SIZE, ctx=ctx)

    def host():
        return matcher.match_gated(d0, pred, a.radius, d1, kp1, **kw)

    b, k = _lib.DeviceArray.from_numpy(ctx, d1), _lib.DeviceArray.from_numpy(ctx, kp1)
    opt = _lib.MatchGateOptionsC(pred=pred.ctypes.data, radius=None, kp1=k.ptr, radius0=a.radius, width=SIZE[0],
                                 height=SIZE[1], ratio=0.8, max_dist=300.0,
                                 flags=_lib.VO_MATCH_GATE_UNIQUE | _lib.VO_MATCH_DEVICE_PTRS, reserved=0)
    out = np.empty((a.n0, 2), np.int32)
    cnt = np.zeros(1, np.int32)

    def dev():
        _lib.check(ctx.lib.vo_match_gated(ctx.handle, C.c_void_p(d0.ctypes.data), a.n0, C.c_void_p(b.ptr), a.n1, a.dim,
                                          C.byref(opt), ptr(out, C.c_int32), None, ptr(cnt, C.c_int32)),
                   "vo_match_gated")
        return out[:cnt[0]].astype(np.int64)

    def dense():
        return matcher.match_knn2_ratio(d0, d1, 0.8, ctx=ctx, kind=matcher.DESC_SIFT)

    pairs = host()
    assert np.array_equal(pairs, dev()), "device-pointer route differs from the host route"
    res = {"shape": {"n0": a.n0, "n1": a.n1, "dim": a.dim, "image": list(SIZE), "radius_px": a.radius},
           "pairs": {"gated": int(len(pairs)), "dense": int(len(dense()))},
           "timed_regions": {"calls_per_region": a.calls, "regions": a.repeats}}
    for name, fn in (("gated_host_arrays", host), ("gated_device_ptrs", dev), ("dense_knn2_ratio_host_arrays", dense)):
        for _ in range(5):  # warm-up: code objects, workspace growth
            fn()
        res[name] = regions(fn, a.calls, a.repeats)
    # per-kernel event times, in a region of their own
    for name, fn in (("gated_kernels_us", dev), ("dense_kernels_us", dense)):
        _lib.profile_enable(ctx, True)
        for _ in range(a.calls):
            fn()
        prof = _lib.profile_read(ctx)
        _lib.profile_enable(ctx, False)
        res[name] = {kk: round(v[0] / v[1] * 1e3, 2) for kk, v in prof.items()}
    res["note"] = ("gated_kernels_us: match_pack = clears (cell counts, claims) + grid build (count, scan, fill), "
                   "match_f32 = gated search + unique filter; compact_pairs and the copies are not in either")
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
