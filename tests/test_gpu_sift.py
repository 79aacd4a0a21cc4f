"""GPU parity of SIFT detection (vo_sift_detect / vo_sift_pyramid) against the oracle
(reference ``src/modules/frontend.py:27-32,55``; oracle/sift_ref.py).

The kernels keep the oracle's float32 operation order with FMA contraction off, so
every Gaussian and DoG level must be bitwise equal, and the keypoints identical: the
same extrema in the same order, positions, responses, offsets and sizes bit for bit,
octave words exact (the size's 2^e is (float)exp2((double)e) on both sides).

detectAndCompute (orientation, removeDuplicatedSorted, retainBest, descriptors): the same
keypoints in the same order with every field bit for bit, and the descriptors (integers
0..255 stored as float32) identical.
"""

import ctypes as C

import numpy as np
import pytest

from oracle import sift_ref as S
from visualodometry_amd import _lib, sift
from visualodometry_amd.synthetic import sift_scene

pytestmark = pytest.mark.gpu


def _check_kp(got, ref):
    assert len(got["pt"]) == len(ref["pt"])
    np.testing.assert_array_equal(got["index"], ref["index"])
    np.testing.assert_array_equal(got["octave"], ref["octave"])
    np.testing.assert_array_equal(got["pt"], ref["pt"])
    np.testing.assert_array_equal(got["response"], ref["response"])
    np.testing.assert_array_equal(got["xi"], ref["xi"])
    np.testing.assert_array_equal(got["size"], ref["size"])


@pytest.mark.parametrize("h,w,seed", [(64, 80, 0), (120, 200, 1), (376, 1241, 2)])
def test_pyramid_bitwise(ctx, h, w, seed):
    img = sift_scene(h, w, seed=seed, n_blobs=max(20, h * w // 1200), n_boxes=10)
    G, D = sift.pyramid(img, 1.6, 3, ctx=ctx)
    rp = S.gaussian_pyramid(img, 1.6, 3)
    rd = S.dog_pyramid(rp)
    assert len(G) == len(rp)
    for o in range(len(rp)):
        for i in range(6):
            np.testing.assert_array_equal(G[o][i], rp[o][i], err_msg=f"G octave {o} level {i}")
        for i in range(5):
            np.testing.assert_array_equal(D[o][i], rd[o][i], err_msg=f"DoG octave {o} level {i}")


@pytest.mark.parametrize("contrast,edge,sigma", [(0.04, 10.0, 1.6), (0.02, 2.0, 1.6), (0.01, 2.0, 1.6),
                                                 (0.03, 1.0, 1.6)])  # OpenCV default, KITTI/Malaga SIFT, reference default
def test_keypoints_match_oracle(ctx, contrast, edge, sigma):
    img = sift_scene(376, 1241, seed=7)
    _check_kp(sift.detect(img, contrast, edge, sigma, ctx=ctx), S.detect(img, contrast, edge, sigma))


def test_odd_sizes_and_tiny_images(ctx):
    for h, w in ((23, 31), (11, 11), (5, 7), (100, 33)):
        img = sift_scene(h, w, seed=h * w, n_blobs=5, n_boxes=2)
        _check_kp(sift.detect(img, 0.02, 2.0, 1.6, ctx=ctx), S.detect(img, 0.02, 2.0, 1.6))
    flat = np.full((64, 64), 128, np.uint8)
    assert len(sift.detect(flat, ctx=ctx)["pt"]) == 0


def test_batch_matches_single(ctx):
    imgs = np.stack([sift_scene(188, 620, seed=s, n_blobs=100) for s in range(4)])
    cap = 1 << 15
    dI = _lib.DeviceArray.from_numpy(ctx, imgs)
    dF = _lib.DeviceArray(ctx, (cap, 8), np.float32)
    dK = _lib.DeviceArray(ctx, (cap, 8), np.int32)
    dC = _lib.DeviceArray(ctx, (1,), np.int32)
    sift.detect_device(dI, 0.02, 2.0, 1.6, 3, dF, dK, dC, ctx=ctx)
    n = int(dC.numpy()[0])
    F, K = dF.numpy()[:n], dK.numpy()[:n]
    for b in range(4):
        ref = S.detect(imgs[b], 0.02, 2.0, 1.6)
        sel = K[:, 0] == b
        order = np.lexsort((K[sel, 7], K[sel, 6], K[sel, 2], K[sel, 1] & 255))
        assert sel.sum() == len(ref["pt"])
        np.testing.assert_array_equal(F[sel][order][:, :2] * np.float32(0.5), ref["pt"])
        np.testing.assert_array_equal(F[sel][order][:, 3], ref["response"])


def _check_full(got, ref):
    assert len(got["pt"]) == len(ref["pt"])
    for k in ("pt", "size", "angle", "response", "octave", "descriptors"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)


@pytest.mark.parametrize("nfeatures,contrast,edge", [(0, 0.04, 10.0), (0, 0.02, 2.0), (150, 0.02, 2.0),
                                                     (2048, 0.03, 1.0)])
def test_detect_and_compute_matches_oracle(ctx, nfeatures, contrast, edge):
    img = sift_scene(188, 620, seed=11, n_blobs=150)
    got = sift.detect_and_compute(img, nfeatures, contrast, edge, 1.6, ctx=ctx)
    ref = S.detect_and_compute(img, nfeatures, contrast, edge, 1.6)
    _check_full(got, ref)


def test_detect_and_compute_kitti_size(ctx):
    # KITTI image_0 size with the reference's KITTI SIFT settings (config.py:64-66)
    img = sift_scene(376, 1241, seed=7)
    got = sift.detect_and_compute(img, 4000, 0.02, 2.0, 1.6, ctx=ctx)
    ref = S.detect_and_compute(img, 4000, 0.02, 2.0, 1.6)
    assert len(ref["pt"]) > 300
    _check_full(got, ref)
    # the nfeatures cut binds: 300 strongest (plus boundary ties)
    got = sift.detect_and_compute(img, 300, 0.02, 2.0, 1.6, ctx=ctx)
    ref = S.detect_and_compute(img, 300, 0.02, 2.0, 1.6)
    _check_full(got, ref)


def test_detect_and_compute_textured_kitti(ctx):
    # ~7.8k keypoints: the nfeatures = 4000 cut of the reference's KITTI config binds
    img = sift_scene(376, 1241, seed=200, texture=12.0)
    got = sift.detect_and_compute(img, 4000, 0.02, 2.0, 1.6, ctx=ctx)
    ref = S.detect_and_compute(img, 4000, 0.02, 2.0, 1.6)
    assert len(ref["pt"]) >= 4000
    _check_full(got, ref)


def test_detect_and_compute_low_contrast_capacity_retry(ctx):
    """The malaga / parking SIFT settings (contrast 0.01, edge 2, nfeatures 3000,
    config.py:80-85,92-96) on a textured 480 x 640 image, with a working capacity far below
    the oriented keypoint count: the call grows it instead of failing, to the
    capacity the overflowing pass reported, and the result equals the oracle and
    the large-capacity call.  The batch entry point reports that capacity as -count."""
    img = sift_scene(480, 640, seed=201, texture=14.0)
    ref = S.detect_and_compute(img, 3000, 0.01, 2.0, 1.6)
    assert len(ref["pt"]) >= 3000
    got = sift.detect_and_compute(img, 3000, 0.01, 2.0, 1.6, capacity=3072, ctx=ctx)
    _check_full(got, ref)
    _check_full(sift.detect_and_compute(img, 3000, 0.01, 2.0, 1.6, ctx=ctx), ref)
    d_img = _lib.DeviceArray.from_numpy(ctx, img[None])
    d_cnt = _lib.DeviceArray(ctx, (1,), np.int32)
    caps = [3072]
    while True:  # the reported capacity is taken as is: one retry, two when a guess fell short
        d_kp = _lib.DeviceArray(ctx, (1, caps[-1], 8), np.int32)
        d_desc = _lib.DeviceArray(ctx, (1, caps[-1], 128), np.float32)
        sift.detect_and_compute_device(d_img, 3000, 0.01, 2.0, 1.6, 3, d_kp, d_desc, d_cnt, ctx=ctx)
        n = int(d_cnt.numpy()[0])
        if n >= 0:
            break
        assert -n > caps[-1] and len(caps) < 3, caps
        caps.append(-n)
    assert len(caps) >= 2 and n == len(ref["pt"]), caps


@pytest.fixture(scope="module")
def textured_small():
    """A 96 x 128 textured image and the oracle's detectAndCompute of it for nfeatures 0 (116 keypoints) and 50,
    at contrast 0.02, edge 10."""
    img = sift_scene(96, 128, seed=41, texture=12.0)
    return img, {nf: S.detect_and_compute(img, nf, 0.02, 10.0, 1.6) for nf in (0, 50)}


@pytest.mark.parametrize("nfeatures", [0, 50])
def test_detect_and_compute_host_and_device_entries_agree(ctx, textured_small, nfeatures):
    """``vo_sift_detect_and_compute`` and ``vo_sift_detect_and_compute_dev`` (one host body, the
    first working capacity and the kind of the final copy apart), each with a capacity of twice
    the oracle's count: the counts, keypoint records and descriptors are byte-equal between the
    two entries and equal to the oracle's."""
    img, refs = textured_small
    ref = refs[nfeatures]
    h, w = img.shape
    cap = 2 * len(ref["pt"])
    assert cap > 0 and (nfeatures == 0 or len(ref["pt"]) >= nfeatures)
    kp, desc = sift._detect_and_compute_records(img, nfeatures, 0.02, 10.0, 1.6, 3, cap, ctx)
    d_kp = _lib.DeviceArray(ctx, (cap, 8), np.int32)
    d_desc = _lib.DeviceArray(ctx, (cap, 128), np.float32)
    cnt = C.c_int32(-1)
    _lib.check(ctx.lib.vo_sift_detect_and_compute_dev(
        ctx.handle, _lib.ptr(img, C.c_uint8), h, w, nfeatures, 0.02, 10.0, 1.6, 3, cap,
        C.c_void_p(d_kp.ptr), C.c_void_p(d_desc.ptr), C.byref(cnt)), "vo_sift_detect_and_compute_dev")
    n = cnt.value
    assert n == len(kp) == len(ref["pt"])
    assert d_kp.numpy()[:n].tobytes() == kp.tobytes()
    assert d_desc.numpy()[:n].tobytes() == desc.tobytes()
    _check_full(sift._kp_dict(kp, desc), ref)


def test_detect_and_compute_edge_cases(ctx):
    flat = np.full((64, 64), 128, np.uint8)
    r = sift.detect_and_compute(flat, ctx=ctx)
    assert len(r["pt"]) == 0 and r["descriptors"].shape == (0, 128)
    kps, des = sift.SIFT_create(nfeatures=10).detectAndCompute(flat, None)
    assert kps == () and des is None
    for h, w in ((23, 31), (11, 11), (100, 33)):
        img = sift_scene(h, w, seed=h * w, n_blobs=5, n_boxes=2)
        _check_full(sift.detect_and_compute(img, 0, 0.02, 2.0, 1.6, ctx=ctx), S.detect_and_compute(img, 0, 0.02, 2.0, 1.6))
    img = sift_scene(188, 620, seed=11, n_blobs=150)
    with pytest.raises(_lib.VoError):
        sift.detect_and_compute(img, 0, 0.02, 2.0, 1.6, capacity=8, ctx=ctx)
    # the context stays usable after the overflow
    _check_full(sift.detect_and_compute(img, 50, 0.02, 2.0, 1.6, ctx=ctx), S.detect_and_compute(img, 50, 0.02, 2.0, 1.6))


def test_sift_create_drop_in(ctx):
    img = sift_scene(188, 620, seed=5, n_blobs=120)
    det = sift.SIFT_create(nfeatures=4000, contrastThreshold=0.02, edgeThreshold=2.0, sigma=1.6)
    kps, des = det.detectAndCompute(img, None)
    ref = S.detect_and_compute(img, 4000, 0.02, 2.0, 1.6)
    pts = np.array([k.pt for k in kps], dtype=np.float32)  # frontend.py:59
    np.testing.assert_array_equal(pts, ref["pt"])
    np.testing.assert_array_equal(np.array(des, dtype=np.float32), ref["descriptors"])
    assert all(k.octave == o for k, o in zip(kps, ref["octave"]))


def test_detect_and_compute_batch(ctx):
    imgs = np.stack([sift_scene(188, 620, seed=s, n_blobs=100) for s in range(3)])
    cap = 4096
    dI = _lib.DeviceArray.from_numpy(ctx, imgs)
    dK = _lib.DeviceArray(ctx, (3, cap, 8), np.int32)
    dD = _lib.DeviceArray(ctx, (3, cap, 128), np.float32)
    dC = _lib.DeviceArray(ctx, (3,), np.int32)
    sift.detect_and_compute_device(dI, 200, 0.02, 2.0, 1.6, 3, dK, dD, dC, ctx=ctx)
    counts = dC.numpy()
    K = sift.unpack_device_keypoints(dK.numpy())
    D = dD.numpy()
    for b in range(3):
        ref = S.detect_and_compute(imgs[b], 200, 0.02, 2.0, 1.6)
        n = counts[b]
        assert n == len(ref["pt"])
        assert np.all(K[b, :n]["image"] == b)
        got = sift._kp_dict(K[b, :n], D[b, :n])
        _check_full(got, ref)


def test_batch_with_empty_image_and_repeat(ctx):
    """The descriptor kernel's keypoint counter (zeroed by the selection kernel each call)
    across images of a batch, one of them without keypoints, and again on the same buffers."""
    imgs = np.stack([sift_scene(188, 620, seed=21, n_blobs=100), np.full((188, 620), 90, np.uint8),
                     sift_scene(188, 620, seed=22, n_blobs=100)])
    cap = 4096
    dI = _lib.DeviceArray.from_numpy(ctx, imgs)
    dK = _lib.DeviceArray(ctx, (3, cap, 8), np.int32)
    dD = _lib.DeviceArray(ctx, (3, cap, 128), np.float32)
    dC = _lib.DeviceArray(ctx, (3,), np.int32)
    outs = []
    for _ in range(2):
        sift.detect_and_compute_device(dI, 300, 0.02, 2.0, 1.6, 3, dK, dD, dC, ctx=ctx)
        outs.append((dC.numpy().copy(), dK.numpy().copy(), dD.numpy().copy()))
    counts = outs[0][0]
    assert counts[1] == 0
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    for b in (0, 2):
        n = counts[b]
        np.testing.assert_array_equal(outs[0][1][b, :n], outs[1][1][b, :n])
        np.testing.assert_array_equal(outs[0][2][b, :n], outs[1][2][b, :n])
        ref = S.detect_and_compute(imgs[b], 300, 0.02, 2.0, 1.6)
        _check_full(sift._kp_dict(sift.unpack_device_keypoints(outs[0][1])[b, :n], outs[0][2][b, :n]), ref)


def test_overlapped_pyramid_equals_one_stream(ctx):
    """sift_run's second stream (each octave's last two levels and extrema test beside the next
    octave's chain) against the one-stream order the event profiler forces: the same keypoints
    and descriptors, over images of different octave counts on one context."""
    for h, w, seed in ((376, 1241, 31), (64, 80, 32), (240, 320, 33)):
        img = sift_scene(h, w, seed=seed, texture=12.0)
        a = sift.detect_and_compute(img, 1000, 0.02, 2.0, 1.6, ctx=ctx)
        _lib.profile_enable(ctx, True)
        try:
            b = sift.detect_and_compute(img, 1000, 0.02, 2.0, 1.6, ctx=ctx)
            _lib.profile_read(ctx)
        finally:
            _lib.profile_enable(ctx, False)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{h}x{w} {k}")


@pytest.mark.parametrize("order", ["flat_last", "flat_first"])
def test_flat_images_in_a_batch(ctx, order):
    """A constant image has constant DoG levels, and at contrastThreshold 0.02 (threshold 0)
    every pixel of such a level can pass the 26-neighbour test; those points are dropped as
    adjustLocalExtrema would reject them, so the other images of the batch keep their
    keypoints (the flooded candidate lists used to drop theirs) and nothing overflows."""
    a, c = sift_scene(188, 620, seed=21, n_blobs=100), sift_scene(188, 620, seed=22, n_blobs=100)
    flat = np.full((188, 620), 90, np.uint8)
    imgs = np.stack([a, c, flat] if order == "flat_last" else [flat, a, c])
    cap = 1 << 15
    dI = _lib.DeviceArray.from_numpy(ctx, imgs)
    dF = _lib.DeviceArray(ctx, (cap, 8), np.float32)
    dK = _lib.DeviceArray(ctx, (cap, 8), np.int32)
    dC = _lib.DeviceArray(ctx, (1,), np.int32)
    sift.detect_device(dI, 0.02, 2.0, 1.6, 3, dF, dK, dC, ctx=ctx)
    n = int(dC.numpy()[0])
    assert 0 <= n <= cap
    K = dK.numpy()[:n]
    for b in range(3):
        ref = S.detect(imgs[b], 0.02, 2.0, 1.6)
        assert int((K[:, 0] == b).sum()) == len(ref["pt"]), b
    r = sift.detect_and_compute(flat, 0, 0.02, 2.0, 1.6, ctx=ctx)
    assert len(r["pt"]) == 0
