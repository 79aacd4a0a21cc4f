"""``cfg.klt_tracking`` end to end on the MI355X (tests/klt_dropin_scene.py): the real frontend hooks
over a 4-frame crop sequence with a stub owner holding ``keyframe``.  Pair flows equal the planted
shifts within 0.1 px, a new keyframe is replenished, a frame that shares no content with the
keyframe falls back to detection and descriptor matching; with torch, tensors stay on the frame's
device (its own process, torch initialised first, as tests/test_gpu_torch_coexist.py arranges it)."""

import subprocess
import sys
from pathlib import Path

import pytest

from tests import klt_dropin_scene

pytestmark = pytest.mark.gpu
SCRIPT = Path(__file__).with_name("klt_dropin_check.py")


def test_route_over_a_crop_sequence_with_numpy_dicts(ctx):
    out = klt_dropin_scene.run(None)
    assert len(out["tracked"]) == 3 and out["replenished"] > 0 and out["fallback_keypoints"] > 0


def test_route_with_torch_gpu_tensors():
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
