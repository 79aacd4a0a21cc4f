"""Host-side pins of the essential-matrix drop-in: the ``Cv2Proxy`` routing of
``findEssentialMat`` / ``recoverPose``, the ``init_on_gpu`` switch and its ``VO_AMD_INIT``
environment variable, the C-ABI declarations, and the wrappers' argument checks -- no GPU."""

import dataclasses
import json
import re
import sys
import types

import numpy as np
import pytest

from tests.conftest import GOLDEN, ROOT
from visualodometry_amd import _lib, essential
from visualodometry_amd.dropin import hooks

sys.path.insert(0, str(ROOT / "visualodometry_amd" / "dropin"))
from config.config import VOConfig, get_config  # noqa: E402


def _fake_cv2():
    return types.SimpleNamespace(RANSAC=8, findEssentialMat=lambda *a, **k: ("cpu-E", a, k),
                                 recoverPose=lambda *a, **k: ("cpu-pose", a, k), Rodrigues=lambda r: "rodrigues")


def test_proxy_routes_only_when_the_flag_is_on(monkeypatch):
    calls = []
    monkeypatch.setattr(essential, "findEssentialMat", lambda *a, **k: calls.append(("E", a, k)) or ("gpu-E", None))
    monkeypatch.setattr(essential, "recoverPose", lambda *a, **k: calls.append(("pose", a, k)) or "gpu-pose")
    real, on = _fake_cv2(), [False]
    proxy = hooks.Cv2Proxy(real, lambda: True, lambda: on[0])
    p1, p2, K = np.zeros((8, 2), np.float32), np.ones((8, 2), np.float32), np.eye(3)
    # off: the real cv2 gets the call unchanged
    r = proxy.findEssentialMat(p1, p2, K, method=real.RANSAC, prob=0.9, threshold=2.0)
    assert r[0] == "cpu-E" and r[2] == {"method": 8, "prob": 0.9, "threshold": 2.0}
    assert proxy.recoverPose("E", p1, p2, K)[0] == "cpu-pose" and not calls
    assert proxy.Rodrigues(None) == "rodrigues"
    # on: the MI355X wrappers, prob and threshold passed through
    on[0] = True
    assert proxy.findEssentialMat(p1, p2, K, method=real.RANSAC, prob=0.9, threshold=2.0) == ("gpu-E", None)
    assert proxy.recoverPose("E", p1, p2, K) == "gpu-pose"
    (k0, a0, kw0), (k1, a1, kw1) = calls
    assert k0 == "E" and a0[0] is p1 and a0[1] is p2 and a0[2] is K
    assert kw0 == {"method": essential.RANSAC, "prob": 0.9, "threshold": 2.0}
    assert k1 == "pose" and a1[0] == "E" and a1[1] is p1 and a1[3] is K and not kw1
    # the default proxy (as older callers build it) leaves the initialisation on the host
    assert hooks.Cv2Proxy(real, lambda: True).findEssentialMat(p1, p2, K)[0] == "cpu-E"


def test_wrap_init_records_the_flag():
    class VO:
        def __init__(self, cfg):
            self.cfg = cfg
            self.map_points = {}

    old = hooks._INIT_ON_GPU[0], hooks._PNP_ON_GPU[0]
    try:
        VO.__init__ = hooks._wrap_init(VO.__init__)
        VO(types.SimpleNamespace(init_on_gpu=True, map_store_arrays=False))
        assert hooks._INIT_ON_GPU[0] is True
        VO(types.SimpleNamespace(map_store_arrays=False))
        assert hooks._INIT_ON_GPU[0] is False
    finally:
        hooks._INIT_ON_GPU[0], hooks._PNP_ON_GPU[0] = old


def test_config_switch_and_environment(monkeypatch):
    monkeypatch.delenv("VO_AMD_INIT", raising=False)
    assert VOConfig().init_on_gpu is False and get_config("kitti").init_on_gpu is False
    monkeypatch.setenv("VO_AMD_INIT", "1")
    assert get_config("kitti").init_on_gpu is True
    monkeypatch.setenv("VO_AMD_INIT", "0")
    assert get_config("kitti").init_on_gpu is False


@pytest.mark.parametrize("dataset", ["kitti", "malaga", "parking", "own", "unknown"])
def test_config_still_equals_the_reference(monkeypatch, dataset):
    for v in ("VO_AMD_INIT", "VO_AMD_BA", "VO_AMD_SP_BF", "VO_AMD_EXTRACTOR"):
        monkeypatch.delenv(v, raising=False)
    ref = json.loads((GOLDEN / "reference_config.json").read_text())
    ours = dataclasses.asdict(get_config(dataset))
    for k, v in ref["get_config"][dataset].items():
        assert ours[k] == v, k


def test_abi_declares_and_binds_the_entry_points():
    header = (ROOT / "include" / "vo_hip.h").read_text()
    for name in ("vo_essential_ransac", "vo_recover_pose"):
        assert re.search(rf"\bint {name}\(vo_ctx\* ctx,", header) and name in _lib.SIGNATURES
    n = int(re.search(r"#define VO_PROFILE_KERNELS (\d+)", header).group(1))
    assert n == len(_lib.KERNEL_NAMES) and _lib.KERNEL_NAMES[20:] == ["ess_hyp", "ess_score", "ess_decide",
                                                                      "ess_final", "ess_pose"]
    lib = _lib.load()
    assert hasattr(lib, "vo_essential_ransac") and hasattr(lib, "vo_recover_pose")


def test_wrappers_reject_what_the_reference_does_not_use():
    p, K = np.zeros((8, 2), np.float32), np.eye(3)
    with pytest.raises(ValueError):
        essential.findEssentialMat(p, p, K, method=4)  # LMEDS
    with pytest.raises(ValueError):
        essential.findEssentialMat(p, p, K, essential.RANSAC, 0.999, 1.0, 500)  # maxIters positional
    with pytest.raises(ValueError):
        essential.findEssentialMat(p, p, K, mask=np.ones(8, np.uint8))
    with pytest.raises(ValueError):
        essential.findEssentialMat(p, p, K, distCoeffs1=np.zeros(5))
    with pytest.raises(ValueError):
        essential.findEssentialMat(p, p)  # the focal / principal-point overload
    with pytest.raises(ValueError):
        essential.recoverPose(np.eye(3), p, p, K, mask=np.ones(8, np.uint8))
    with pytest.raises(ValueError):
        essential.recoverPose(np.eye(3), p, p, K, 50.0)  # distanceThresh
    with pytest.raises(ValueError):
        essential.find_essential_ransac(p, p[:5], K)
