"""BASELINE config 5 through the drop-in: ``match_frames`` under ``extractor_type ==
"superpoint"`` with ``superpoint_bf_match`` on runs the MFMA brute-force matcher with the
cross check (one-to-one pairs, as LightGlue's are) -- bit-exact against ``tests/mutual_ref.py``.

Descriptors go in as numpy here; ``tests/superpoint_bf_check.py`` repeats the route in a fresh
process with torch initialised first and the dicts' ``(1, N, 256)`` tensors on the GPU, the way
``tests/test_gpu_torch_coexist.py`` arranges it.
"""

import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from tests import mutual_ref
from visualodometry_amd.dropin import hooks

pytestmark = pytest.mark.gpu
SCRIPT = Path(__file__).resolve().parent / "superpoint_bf_check.py"


class _Front:
    def __init__(self, **conf):
        self.conf = SimpleNamespace(**conf)

    def match_frames(self, f0, f1):
        return "original"


def _feats(d):
    return {"descriptors": d[None]}  # the feature dict's (1, N, D) layout (frontend.py:71)


@pytest.fixture(scope="module")
def sp_pair():
    d0, d1 = mutual_ref.superpoint_near_duplicates(700, 900, 3, 150)
    ref, n_forward = mutual_ref.mutual(d0, d1, 0.75, "c")
    assert mutual_ref.informative(ref, n_forward)
    return d0, d1, ref


def test_superpoint_route_is_bit_exact(ctx, sp_pair):
    d0, d1, ref = sp_pair
    patched = hooks._wrap_match_frames(_Front.match_frames)
    front = _Front(extractor_type="superpoint", superpoint_bf_match=True, superpoint_bf_ratio=0.75)
    got = patched(front, _feats(d0), _feats(d1))
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.ndim == 2 and got.shape[1] == 2
    np.testing.assert_array_equal(got, ref)
    assert len(set(got[:, 1].tolist())) == len(got)
    # the ratio field is honoured, and its default is the reference's 0.75
    got = patched(_Front(extractor_type="superpoint", superpoint_bf_match=True), _feats(d0), _feats(d1))
    np.testing.assert_array_equal(got, ref)
    ref1, n1 = mutual_ref.mutual(d0, d1, 1.0, "c")
    assert mutual_ref.informative(ref1, n1) and len(ref1) != len(ref)
    front.conf.superpoint_bf_ratio = 1.0
    np.testing.assert_array_equal(patched(front, _feats(d0), _feats(d1)), ref1)


def test_superpoint_route_empty_and_single_row_sides(ctx, sp_pair):
    d0, d1, _ = sp_pair
    patched = hooks._wrap_match_frames(_Front.match_frames)
    front = _Front(extractor_type="superpoint", superpoint_bf_match=True)
    e = np.zeros((0, 256), np.float32)
    for a, b in ((e, d1), (d0, e), (d0, d1[:1])):
        got = patched(front, _feats(a), _feats(b))
        assert got.shape == (0, 2) and got.dtype == np.int64


def test_switch_off_or_absent_goes_to_the_original(ctx, sp_pair):
    d0, d1, _ = sp_pair
    patched = hooks._wrap_match_frames(_Front.match_frames)
    assert patched(_Front(extractor_type="superpoint", superpoint_bf_match=False), _feats(d0), _feats(d1)) == "original"
    assert patched(_Front(extractor_type="superpoint"), _feats(d0), _feats(d1)) == "original"


def test_sift_branch_cross_check(ctx):
    d0, d1 = mutual_ref.sift_near_duplicates()
    ref, n_forward = mutual_ref.mutual(d0, d1)
    assert mutual_ref.informative(ref, n_forward)
    patched = hooks._wrap_match_frames(_Front.match_frames)
    got = patched(_Front(extractor_type="sift", match_on_gpu=True, match_cross_check=True), _feats(d0), _feats(d1))
    np.testing.assert_array_equal(got, ref)
    got = patched(_Front(extractor_type="sift", match_on_gpu=True), _feats(d0), _feats(d1))
    np.testing.assert_array_equal(got, mutual_ref.forward(d0, d1))  # off by default: today's pairs


def test_superpoint_route_with_torch_gpu_tensors():
    try:
        import torch  # noqa: F401
    except ImportError:
        pytest.skip("torch is not importable on this box")
    r = subprocess.run([sys.executable, str(SCRIPT)], capture_output=True, text=True, timeout=240)
    out = r.stdout + r.stderr
    if "SKIP:" in r.stdout:
        pytest.skip(r.stdout.strip())
    assert r.returncode == 0, out[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "OK", out[-4000:]
