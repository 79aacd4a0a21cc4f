"""Latency of the KLT tracker (klt.track / vo_klt_track) at a frame-sized shape, beside what it
replaces between two keyframes: detectAndCompute of the new frame plus the descriptor match against
the keyframe.

Shape: the (up to) 4000 SIFT keypoints of a 376 x 1241 ``sift_scene(texture=12)`` crop tracked into
the crop a few pixels further on, r = 10, 4 levels, with and without the forward-backward check.
The keyframe's pyramid is cached under its tag; the new frame's image is uploaded and its pyramid
built inside every call, as on the drive.  Every call is synchronous (host arrays in and out), so
a call is timed on the host clock and, bracketing it, by a pair of HIP events on the context's
stream; the figure reported is the median over ``--calls`` calls after ``--warmup`` warm-ups.
In the same run: ``sift.detect_and_compute`` of the new frame and ``matcher.match_knn2_ratio``
against the keyframe's cached descriptors, host arrays as well (the drop-in's torch route keeps the
descriptors on the device and is a little faster than that: README, per-frame table).
Writes one JSON object to --out and prints it.
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from visualodometry_amd import _lib, klt, matcher, sift  # noqa: E402
from visualodometry_amd.synthetic import sift_scene  # noqa: E402

H, W, MARGIN = 376, 1241, 16


class Events:
    """A start / stop pair of HIP events on the context's stream (the runtime the library loaded)."""

    def __init__(self, ctx):
        self.hip = C.CDLL("libamdhip64.so")
        self.stream = C.c_void_p(ctx.lib.vo_stream(ctx.handle))
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for e in (self.a, self.b):
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def time(self, fn) -> float:
        assert self.hip.hipEventRecord(self.a, self.stream) == 0
        fn()
        assert self.hip.hipEventRecord(self.b, self.stream) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float(0)
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return float(ms.value)


def timed(fn, ev, warmup, calls):
    for _ in range(warmup):
        fn()
    host, dev = [], []
    for _ in range(calls):
        t = time.perf_counter()
        dev.append(ev.time(fn))
        host.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": round(float(np.median(host)), 4), "min_ms": round(min(host), 4), "max_ms": round(max(host), 4),
            "events_median_ms": round(float(np.median(dev)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--shift", type=int, nargs=2, default=(6, 2))
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="profiles/klt_track.json")
    a = ap.parse_args()
    assert a.calls >= 20 and a.warmup >= 3
    ctx = _lib.context(0)
    ev = Events(ctx)
    base = sift_scene(H + 2 * MARGIN, W + 2 * MARGIN, seed=0, texture=12)
    sx, sy = a.shift
    img0 = np.ascontiguousarray(base[MARGIN:MARGIN + H, MARGIN:MARGIN + W])
    img1 = np.ascontiguousarray(base[MARGIN - sy:MARGIN - sy + H, MARGIN - sx:MARGIN - sx + W])
    sift_kw = dict(nfeatures=a.points, contrast=0.02, edge=2.0, sigma=1.6)

    def detect(img):
        return sift.detect_and_compute(img, sift_kw["nfeatures"], sift_kw["contrast"], sift_kw["edge"],
                                       sift_kw["sigma"], ctx=ctx)

    k0 = detect(img0)
    pts0, des0 = np.ascontiguousarray(k0["pt"], np.float32), np.ascontiguousarray(k0["descriptors"], np.float32)
    kw = dict(win_radius=10, levels=4, tags=(77, 0), ctx=ctx)
    state = {}

    def track_plain():
        state["plain"] = klt.track(img0, img1, pts0, **kw)

    def track_fb():
        state["fb"] = klt.track(img0, img1, pts0, fb_thresh=1.0, **kw)

    def detect_new():
        state["k1"] = detect(img1)

    def match():
        state["pairs"] = matcher.match_knn2_ratio(des0, state["des1"], kind=matcher.DESC_SIFT, cache_query=True,
                                                  ctx=ctx)

    res = {"shape": {"image": [H, W], "points": int(len(pts0)), "win_radius": 10, "levels": 4, "shift": [sx, sy]},
           "calls": a.calls, "warmup": a.warmup}
    res["klt_track"] = timed(track_plain, ev, a.warmup, a.calls)
    res["klt_track_fb"] = timed(track_fb, ev, a.warmup, a.calls)
    res["detect_and_compute"] = timed(detect_new, ev, a.warmup, a.calls)
    state["des1"] = np.ascontiguousarray(state["k1"]["descriptors"], np.float32)
    res["match_knn2_ratio"] = timed(match, ev, a.warmup, a.calls)
    res["detect_plus_match_median_ms"] = round(res["detect_and_compute"]["median_ms"] +
                                               res["match_knn2_ratio"]["median_ms"], 4)
    shift = np.float32((sx, sy))
    for name in ("plain", "fb"):
        p1, status, _ = state[name]
        ok = status == 0
        dev = np.abs(p1[ok] - pts0[ok] - shift).max(1)
        res["klt_track" + ("_fb" if name == "fb" else "")].update(
            tracked=int(ok.sum()), within_0p1_px=int((dev <= 0.1).sum()),
            status_counts=np.bincount(status, minlength=7).tolist())
    res["match_knn2_ratio"]["pairs"] = int(len(state["pairs"]))
    res["detect_and_compute"]["keypoints"] = int(len(state["k1"]["pt"]))
    res["note"] = ("median_ms: host clock around one synchronous call; events_median_ms: HIP events on the context "
                   "stream around the same call.  klt_track includes the new frame's upload and pyramid; the "
                   "keyframe's pyramid is a cache hit.")
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
