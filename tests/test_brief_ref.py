"""The steered BRIEF contract on the CPU: the committed pattern table against its generator, the
library's copy and the restatement (``tests/brief_ref.py``), and two properties of the restatement
itself: a quarter turn of the image leaves the descriptors unchanged and shifts the bin by a
quarter of the bins, and grey-level noise moves a descriptor far less than a different patch does
(no GPU)."""

import importlib.util
from pathlib import Path

import numpy as np
import pytest

from tests import brief_ref as R
from visualodometry_amd import brief

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("make_brief_pattern", ROOT / "tools" / "make_brief_pattern.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_tool_the_library_and_the_restatement_hold_the_same_table(tool):
    P, C, S = R.tables()
    tP, tC, tS = tool.tables()
    lP, lC, lS = brief.pattern()
    for a, b, c in ((P, tP, lP), (C, tC, lC), (S, tS, lS)):
        assert a.dtype == b.dtype == c.dtype and a.shape == b.shape == c.shape
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)
    assert P.shape == (32, 256, 4) and P.dtype == np.int8
    assert tool.HEADER.read_text() == tool.render()  # the committed header is the tool's output


def test_every_coordinate_fits_the_box_sum_plane_and_a_quarter_turn_is_exact():
    P, C, S = R.tables()
    P = P.astype(np.int64)
    assert np.abs(P).max() <= 13  # what the kernel's LDS plane indices 13 + coordinate rest on
    assert np.abs(P).max() <= 12 and (P[..., 0] ** 2 + P[..., 1] ** 2).max() <= 148 \
        and (P[..., 2] ** 2 + P[..., 3] ** 2).max() <= 148
    for k in range(24):
        np.testing.assert_array_equal(P[k + 8][:, 0::2], -P[k][:, 1::2])
        np.testing.assert_array_equal(P[k + 8][:, 1::2], P[k][:, 0::2])
    assert len({tuple(t) for t in P[0]}) == 256 and not ((P[0][:, :2] == P[0][:, 2:]).all(1)).any()
    np.testing.assert_array_equal(C[:9], [16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196, 0])
    np.testing.assert_array_equal(S[:9], [0, 3196, 6270, 9102, 11585, 13623, 15137, 16069, 16384])


H, W, N = 96, 128, 60


@pytest.fixture(scope="module")
def scene():
    img = R.texture(H, W, seed=3)
    pts = R.interior_points(H, W, N, seed=4)
    return img, pts, R.describe(img, pts)


def test_a_quarter_turn_of_the_image_keeps_the_descriptor_and_shifts_the_bin(scene):
    img, pts, (des, bins, status) = scene
    assert (status == 0).all() and len(set(bins.tolist())) > 8  # many directions are present
    rot = np.ascontiguousarray(np.rot90(img))
    rpts = np.stack([pts[:, 1], W - 1 - pts[:, 0]], 1)
    rdes, rbins, rstatus = R.describe(rot, rpts)
    assert (rstatus == 0).all()
    np.testing.assert_array_equal(rdes, des)
    np.testing.assert_array_equal(rbins, (bins + 24) % 32)


def test_noise_moves_a_descriptor_far_less_than_another_patch_does(scene):
    img, pts, (des, _, _) = scene
    rng = np.random.default_rng(5)
    noisy = np.clip(img.astype(np.int64) + rng.integers(-6, 7, img.shape), 0, 255).astype(np.uint8)
    ndes, _, _ = R.describe(noisy, pts)
    d = R.hamming(des, ndes)
    true = np.diag(d)
    other = d[~np.eye(N, dtype=bool)]
    med, p95, far5 = float(np.median(true)), float(np.percentile(true, 95)), float(np.percentile(other, 5))
    print(f"true pairs: median {med}, 95th percentile {p95}; other pairs: 5th percentile {far5}")
    assert med < far5


def test_status_bins_and_bits_of_the_degenerate_cases():
    des, bins, status = R.describe(R.flat(40, 33), R.edge_points(40, 33))
    assert not des.any() and not bins.any()  # flat: zero moments, no strict inequality
    np.testing.assert_array_equal(status[:16], 0)
    # -0.5 and w - 0.5 = 32.5 round half to even onto the image; -0.51, w - 0.49, -1, (w, h) and the
    # non-finite and 2^24 points do not; 2^24 - 1 is finite but off the image; -0 is pixel 0
    np.testing.assert_array_equal(status[16:], [0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0])
    des, bins, status = R.describe(R.step_edge(40, 33), R.edge_points(40, 33))
    assert des[status == 0].any() and not des[status == 1].any()
    one = R.describe(np.array([[9]], np.uint8), [[0, 0], [0.5, -0.5], [1, 0]])
    assert not one[0].any() and one[2].tolist() == [0, 0, 1]
