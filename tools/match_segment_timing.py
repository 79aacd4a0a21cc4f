"""Latency of the segment-gated matcher (matcher.match_segment / vo_match_segment) at a frame-sized
shape: 4000 keypoints of one view against 4000 of the next, dim 128, a KITTI-size image, capsules of
radius 3 px around the epipolar segments of a two-view scene (depths 2 .. 1e4).

Reports the host-array call and the device-pointer call (train descriptors and keypoints resident in
HBM) as the median of repeated timed regions with min and max, each region a run of calls that ends
in the call's own stream synchronise; the per-kernel HIP-event times come from a region of their own
(the events slow the host).  In the same run, for scale: the circular gate (match_gated, radius 15 px
around the segments' midpoints) and the dense matcher (match_knn2_ratio, same descriptors).
Results are checked against each other, not against the CPU restatement (tests do that).
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
from visualodometry_amd.synthetic import KITTI_K  # noqa: E402

SIZE = (1241, 376)


def scene(n0, n1, dim, seed, found=0.6, noise_px=0.7):
    """Two views (a yaw of 0.03 rad, t = (-0.3, 0.02, -1)) of points at depths U(4, 60): a share of view
    0's keypoints seen in view 1 with pixel noise and a noisy copy of their SIFT-like descriptor, the
    rest of view 1's keypoints clutter.  -> d0, seg, d1, kp1"""
    rng = np.random.default_rng(seed)
    K = np.asarray(KITTI_K, np.float64)
    c, s = np.cos(0.03), np.sin(0.03)
    T1 = np.eye(4)
    T1[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    T1[:3, 3] = [-0.3, 0.02, -1.0]
    kp0 = np.stack([rng.uniform(0, SIZE[0], n0), rng.uniform(0, SIZE[1], n0)], axis=1).astype(np.float32)
    z = rng.uniform(4.0, 60.0, n0)
    X0 = np.stack([(kp0[:, 0] - K[0, 2]) / K[0, 0] * z, (kp0[:, 1] - K[1, 2]) / K[1, 1] * z, z], axis=1)
    X1 = X0 @ T1[:3, :3].T + T1[:3, 3]
    uv = np.stack([K[0, 0] * X1[:, 0] / X1[:, 2] + K[0, 2], K[1, 1] * X1[:, 1] / X1[:, 2] + K[1, 2]], axis=1)
    inside = (X1[:, 2] > 0.5) & (uv[:, 0] >= 0) & (uv[:, 0] <= SIZE[0]) & (uv[:, 1] >= 0) & (uv[:, 1] <= SIZE[1])
    n_found = min(int(found * n0), n1, int(inside.sum()))
    seen = rng.permutation(np.flatnonzero(inside))[:n_found]
    d0 = rng.integers(0, 256, (n0, dim)).astype(np.float32)
    kp = np.concatenate([uv[seen] + rng.normal(0, noise_px, (n_found, 2)),
                         np.stack([rng.uniform(0, SIZE[0], n1 - n_found), rng.uniform(0, SIZE[1], n1 - n_found)], 1)])
    d1 = np.concatenate([np.clip(np.rint(d0[seen] + rng.normal(0, 8.0, (n_found, dim))), 0, 255),
                         rng.integers(0, 256, (n1 - n_found, dim))]).astype(np.float32)
    order = rng.permutation(n1)
    seg, _ = matcher.epipolar_segments(kp0, np.eye(4), T1, K, SIZE, 2.0, 1e4)
    return d0, seg, np.ascontiguousarray(d1[order]), np.ascontiguousarray(kp[order].astype(np.float32))


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
    ap.add_argument("--radius", type=float, default=3.0)
    ap.add_argument("--gated-radius", type=float, default=15.0)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default="profiles/match_segment.json")
    a = ap.parse_args()
    ctx = _lib.context(0)
    d0, seg, d1, kp1 = scene(a.n0, a.n1, a.dim, 7)
    length = np.hypot(seg[:, 2] - seg[:, 0], seg[:, 3] - seg[:, 1])
    mid = np.ascontiguousarray((seg[:, :2] + seg[:, 2:]) / 2)  # NaN for a keypoint without a segment: inactive
    kw = dict(ratio=0.8, max_dist=300.0, unique=True, image_size=SIZE, ctx=ctx)

    def host():
        return matcher.match_segment(d0, seg, a.radius, d1, kp1, **kw)

    b, k = _lib.DeviceArray.from_numpy(ctx, d1), _lib.DeviceArray.from_numpy(ctx, kp1)
    flags = _lib.VO_MATCH_GATE_UNIQUE | _lib.VO_MATCH_DEVICE_PTRS
    opt = _lib.MatchSegmentOptionsC(seg=seg.ctypes.data, radius=None, kp1=k.ptr, radius0=a.radius, width=SIZE[0],
                                    height=SIZE[1], ratio=0.8, max_dist=300.0, flags=flags, reserved=0)
    gopt = _lib.MatchGateOptionsC(pred=mid.ctypes.data, radius=None, kp1=k.ptr, radius0=a.gated_radius, width=SIZE[0],
                                  height=SIZE[1], ratio=0.8, max_dist=300.0, flags=flags, reserved=0)
    out = np.empty((a.n0, 2), np.int32)
    cnt = np.zeros(1, np.int32)

    def dev():
        _lib.check(ctx.lib.vo_match_segment(ctx.handle, C.c_void_p(d0.ctypes.data), a.n0, C.c_void_p(b.ptr), a.n1, a.dim,
                                            C.byref(opt), ptr(out, C.c_int32), None, ptr(cnt, C.c_int32)),
                   "vo_match_segment")
        return out[:cnt[0]].astype(np.int64)

    def gated_dev():
        _lib.check(ctx.lib.vo_match_gated(ctx.handle, C.c_void_p(d0.ctypes.data), a.n0, C.c_void_p(b.ptr), a.n1, a.dim,
                                          C.byref(gopt), ptr(out, C.c_int32), None, ptr(cnt, C.c_int32)),
                   "vo_match_gated")
        return out[:cnt[0]].astype(np.int64)

    def gated_host():
        return matcher.match_gated(d0, mid, a.gated_radius, d1, kp1, **kw)

    def dense():
        return matcher.match_knn2_ratio(d0, d1, 0.8, ctx=ctx, kind=matcher.DESC_SIFT)

    pairs = host()
    assert np.array_equal(pairs, dev()), "device-pointer route differs from the host route"
    assert np.array_equal(gated_host(), gated_dev()), "match_gated: device-pointer route differs from the host route"
    ok = np.isfinite(length)
    res = {"shape": {"n0": a.n0, "n1": a.n1, "dim": a.dim, "image": list(SIZE), "radius_px": a.radius,
                     "gated_radius_px": a.gated_radius},
           "segments": {"active": int(ok.sum()), "median_px": round(float(np.median(length[ok])), 1),
                        "max_px": round(float(length[ok].max()), 1)},
           "pairs": {"segment": int(len(pairs)), "gated": int(len(gated_dev())), "dense": int(len(dense()))},
           "timed_regions": {"calls_per_region": a.calls, "regions": a.repeats}}
    timed = (("segment_host_arrays", host), ("segment_device_ptrs", dev), ("gated_host_arrays", gated_host),
             ("gated_device_ptrs", gated_dev), ("dense_knn2_ratio_host_arrays", dense))
    for name, fn in timed:
        for _ in range(5):  # warm-up: code objects, workspace growth
            fn()
        res[name] = regions(fn, a.calls, a.repeats)
    # per-kernel event times, in a region of their own
    for name, fn in (("segment_kernels_us", dev), ("gated_kernels_us", gated_dev), ("dense_kernels_us", dense)):
        _lib.profile_enable(ctx, True)
        for _ in range(a.calls):
            fn()
        prof = _lib.profile_read(ctx)
        _lib.profile_enable(ctx, False)
        res[name] = {kk: round(v[0] / v[1] * 1e3, 2) for kk, v in prof.items()}
    res["note"] = ("segment_kernels_us / gated_kernels_us: match_pack = clears (cell counts, claims) + grid build "
                   "(count, scan, fill), match_f32 = search + unique filter; compact_pairs and the copies are not in "
                   "either")
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
