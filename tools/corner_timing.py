"""Latency of the corner detector (corners.good_features / vo_good_features) at a frame-sized
shape, beside what the KLT route's replenishment does without it: detectAndCompute of the keyframe's
image, the distance filter against the kept keypoints and the thinning, the last two on the host.

Shape: the 376 x 1241 test scene (``tests/klt_scene.py``: ``base_image`` seed 8), 2000 keep-away
points taken from a first ``good_features`` call, d = 8, room for 2000 corners, quality 0.01, 3 x 3
blocks.  ``good_features`` is timed with the image passed (uploaded inside every call) and with its
tag in the pyramid cache (nothing uploaded but the keep-away points).  Every call is synchronous
(host arrays in and out), so a call is timed on the host clock and, bracketing it, by a pair of HIP
events on the context's stream; the figure reported is the median over ``--calls`` calls after
``--warmup`` warm-ups.  Writes one JSON object to --out and prints it.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from klt_timing import Events, timed  # noqa: E402
from tests import klt_scene  # noqa: E402
from visualodometry_amd import _lib, corners, klt, sift  # noqa: E402
from visualodometry_amd.dropin import hooks  # noqa: E402

H, W, SEED, TAG = 376, 1241, 8, 0xC0A7E5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", type=int, default=2000)
    ap.add_argument("--room", type=int, default=2000)
    ap.add_argument("--distance", type=float, default=8.0)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="profiles/good_features.json")
    a = ap.parse_args()
    assert a.calls >= 20 and a.warmup >= 3
    ctx = _lib.context(0)
    ev = Events(ctx)
    img = klt_scene.crop(klt_scene.base_image(H, W, SEED), H, W)
    keep, _ = corners.good_features(img, a.keep, 0.01, a.distance, ctx=ctx)
    klt.track(img, img, keep[:4], tags=(TAG, 0), ctx=ctx)  # the keyframe's pyramid under its tag, as on the route
    state = {}

    def with_image():
        state["image"] = corners.good_features(img, a.room, 0.01, a.distance, keep=keep, ctx=ctx)

    def with_tag():
        state["tag"] = corners.good_features(None, a.room, 0.01, a.distance, keep=keep, tag=TAG, shape=img.shape,
                                             ctx=ctx)

    def no_keep_no_limit():
        state["free"] = corners.good_features(img, None, 0.01, a.distance, ctx=ctx)

    def detect():
        state["det"] = sift.detect_and_compute(img, 4000, 0.02, 2.0, 1.6, ctx=ctx)

    def today():  # klt_replenish without the switch
        detect()
        det = np.ascontiguousarray(state["det"]["pt"], np.float32)
        new = np.flatnonzero(hooks.far_from(keep, det, a.distance))
        if new.size > a.room:
            new = new[np.linspace(0, new.size - 1, a.room).round().astype(np.int64)]
        state["today"] = new

    res = {"shape": {"image": [H, W], "keep": int(len(keep)), "room": a.room, "min_distance": a.distance,
                     "quality": 0.01, "block_size": 3}, "calls": a.calls, "warmup": a.warmup}
    res["good_features_image"] = timed(with_image, ev, a.warmup, a.calls)
    res["good_features_image"].update(corners.last_stats(ctx))
    res["good_features_tag_cached"] = timed(with_tag, ev, a.warmup, a.calls)
    res["good_features_tag_cached"].update(corners.last_stats(ctx))
    res["good_features_no_keep_no_limit"] = timed(no_keep_no_limit, ev, a.warmup, a.calls)
    res["good_features_no_keep_no_limit"].update(corners.last_stats(ctx))
    res["detect_and_compute"] = timed(detect, ev, a.warmup, a.calls)
    res["detect_and_compute"]["keypoints"] = int(len(state["det"]["pt"]))
    res["replenish_today"] = timed(today, ev, a.warmup, a.calls)
    res["replenish_today"]["appended"] = int(state["today"].size)
    assert np.array_equal(state["image"][0], state["tag"][0]) and np.array_equal(state["image"][1], state["tag"][1])
    res["note"] = ("median_ms: host clock around one synchronous call; events_median_ms: HIP events on the context "
                   "stream around the same call.  replenish_today = detect_and_compute + hooks.far_from + thinning "
                   "(the last two on the host).  candidates / rounds / accepted / cell_side: vo_corner_stats of the "
                   "last call.")
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
