"""The steered BRIEF arithmetic (csrc/brief_math.h: status, reflected patch, disc moments, bin, box
sums, bits), compiled for the host by ``brief_host_check`` and run on CPU, against
``tests/brief_ref.py``: descriptors, bins and status equal bit for bit (no GPU)."""

import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import brief_ref as R

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "visualodometry_amd" / "lib" / "brief_host_check"


def cases():
    big = R.texture(96, 128, seed=3)
    c = {
        "one_pixel": (np.array([[200]], np.uint8), np.array([[0, 0], [0.5, -0.5], [1, 0], [np.nan, 0]], np.float32)),
        "tiny_5x7": (R.texture(5, 7, seed=1, smooth=0), R.edge_points(5, 7)),
        "odd_40x33": (R.texture(40, 33, seed=2, smooth=1), R.edge_points(40, 33)),
        "flat": (R.flat(40, 33), R.edge_points(40, 33)),
        "step_edge": (R.step_edge(40, 33),
                      np.concatenate([R.edge_points(40, 33), R.interior_points(40, 33, 12, margin=3)])),
        "texture_interior": (big, R.interior_points(96, 128, 60, seed=4)),
        "texture_rot90": (np.ascontiguousarray(np.rot90(big)), R.interior_points(128, 96, 40, seed=6)),
        "texture_border": (big, R.edge_points(96, 128)),
    }
    return c


CASES = cases()


@pytest.fixture(scope="module")
def exe():
    if not EXE.exists():
        subprocess.run(["make", "-s", "-C", str(ROOT / "visualodometry_amd" / "csrc"), "../lib/brief_host_check"],
                       check=True)
    return EXE


@pytest.mark.parametrize("name", list(CASES))
def test_host_build_matches_the_restatement(exe, tmp_path, name):
    img, pts = CASES[name]
    h, w = img.shape
    n = len(pts)
    fi, fo = tmp_path / "in", tmp_path / "out"
    with open(fi, "wb") as f:
        np.array([h, w, n], np.int32).tofile(f)
        np.ascontiguousarray(img).tofile(f)
        np.ascontiguousarray(pts, np.float32).tofile(f)
    subprocess.run([str(exe), str(fi), str(fo)], check=True)
    raw = Path(fo).read_bytes()
    assert len(raw) == n * (32 + 4 + 1)
    des = np.frombuffer(raw, np.uint32, n * 8).reshape(n, 8)
    bins = np.frombuffer(raw, np.int32, n, 32 * n)
    status = np.frombuffer(raw, np.uint8, n, 36 * n)
    rdes, rbins, rstatus = R.describe(img, pts)
    np.testing.assert_array_equal(status, rstatus)
    np.testing.assert_array_equal(bins, rbins)
    np.testing.assert_array_equal(des, rdes)


def test_the_cases_are_informative():
    des, bins, status = R.describe(*CASES["step_edge"])
    assert (status == 0).sum() >= 20 and des[status == 0].any()
    des, bins, status = R.describe(*CASES["texture_interior"])
    assert len(set(bins.tolist())) > 8 and (np.unpackbits(des.view(np.uint8), axis=1).mean() > 0.3)
    assert R.describe(*CASES["texture_border"])[2].tolist().count(1) >= 10
