"""Latency of the steered BRIEF descriptor (brief.describe / vo_brief_describe) and of the Hamming
matcher (matcher.match_hamming / vo_match_hamming) at frame-sized shapes, beside the SIFT matcher on
as many rows.

Shape: the 376 x 1241 test scene (``tests/klt_scene.py``: ``base_image`` seed 8) and 4000 points: the
corners ``good_features`` finds at d = 4, filled up with uniform random positions.  ``describe`` is
timed with the image passed (uploaded inside every call) and with its tag in the pyramid cache.
``match_hamming`` is timed at 4000 x 4000 rows of 8 words, the second set the first with a tenth of
the rows replaced and ~10 bits flipped per row, plain and with the cross check, from host arrays and
from device arrays; ``match_knn2_ratio`` at 4000 x 4000 x 128 SIFT-like rows (host arrays) is the
comparison.  Every call is synchronous, so a call is timed on the host clock and, bracketing it, by a
pair of HIP events on the context's stream; the figure reported is the median over ``--calls`` calls
after ``--warmup`` warm-ups.  Writes one JSON object to --out and prints it.
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
from visualodometry_amd import _lib, brief, corners, klt, matcher  # noqa: E402
from visualodometry_amd.synthetic import sift_like_pair  # noqa: E402

H, W, SEED, TAG = 376, 1241, 8, 0xB21EF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="profiles/brief.json")
    a = ap.parse_args()
    assert a.calls >= 20 and a.warmup >= 3
    n = a.points
    ctx = _lib.context(0)
    ev = Events(ctx)
    rng = np.random.default_rng(0)
    img = klt_scene.crop(klt_scene.base_image(H, W, SEED), H, W)
    pts, _ = corners.good_features(img, n, 0.01, 4.0, ctx=ctx)
    n_corners = len(pts)
    fill = np.stack([rng.uniform(0, W - 1, n - n_corners), rng.uniform(0, H - 1, n - n_corners)], 1).astype(np.float32)
    pts = np.ascontiguousarray(np.concatenate([pts, fill]))
    klt.track(img, img, pts[:4], tags=(TAG, 0), ctx=ctx)  # the image's pyramid under its tag, as on the route
    state = {}

    def with_image():
        state["image"] = brief.describe(img, pts, ctx=ctx)

    def with_tag():
        state["tag"] = brief.describe(None, pts, tag=TAG, shape=img.shape, ctx=ctx)

    res = {"shape": {"image": [H, W], "points": n, "corners_among_them": int(n_corners), "words": 8},
           "calls": a.calls, "warmup": a.warmup}
    res["describe_image"] = timed(with_image, ev, a.warmup, a.calls)
    res["describe_tag_cached"] = timed(with_tag, ev, a.warmup, a.calls)
    assert all(np.array_equal(x, y) for x, y in zip(state["image"], state["tag"]))
    res["describe_image"]["status_ok"] = int((state["image"][2] == 0).sum())

    d0 = state["image"][0]
    d1 = d0.copy()
    flips = rng.integers(0, 256, (n, 10))
    for c in range(flips.shape[1]):
        d1[np.arange(n), flips[:, c] // 32] ^= (np.uint32(1) << (flips[:, c] % 32).astype(np.uint32))
    swap = rng.choice(n, n // 10, replace=False)
    d1[swap] = rng.integers(0, 1 << 32, (len(swap), 8), dtype=np.uint64).astype(np.uint32)
    d1 = np.ascontiguousarray(d1[rng.permutation(n)])
    dev0, dev1 = _lib.DeviceArray.from_numpy(ctx, d0), _lib.DeviceArray.from_numpy(ctx, d1)

    def hamming(x, y, mutual, key):
        def run():
            state[key] = matcher.match_hamming(x, y, ratio=0.8, max_dist=64, cross_check=mutual, ctx=ctx)
        return run

    for key, x, y, mutual in (("match_hamming_host", d0, d1, False), ("match_hamming_host_mutual", d0, d1, True),
                              ("match_hamming_device", dev0, dev1, False),
                              ("match_hamming_device_mutual", dev0, dev1, True)):
        res[key] = timed(hamming(x, y, mutual, key), ev, a.warmup, a.calls)
        res[key]["pairs"] = int(len(state[key]))
    assert np.array_equal(state["match_hamming_host"], state["match_hamming_device"])
    assert np.array_equal(state["match_hamming_host_mutual"], state["match_hamming_device_mutual"])

    s0, s1 = sift_like_pair(n, n, 0)

    def sift_match(mutual, key):
        def run():
            state[key] = matcher.match_knn2_ratio(s0, s1, kind=matcher.DESC_SIFT, cross_check=mutual, ctx=ctx)
        return run

    for key, mutual in (("match_knn2_ratio_sift_host", False), ("match_knn2_ratio_sift_host_mutual", True)):
        res[key] = timed(sift_match(mutual, key), ev, a.warmup, a.calls)
        res[key]["pairs"] = int(len(state[key]))
    res["note"] = ("median_ms: host clock around one synchronous call; events_median_ms: HIP events on the context "
                   "stream around the same call.  Host calls upload both descriptor sets inside the call "
                   "(2 x 4000 x 32 bytes for the Hamming rows, 2 x 4000 x 512 bytes for the SIFT rows); device calls "
                   "read them in place.  Every call copies the pairs back and synchronises.")
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
