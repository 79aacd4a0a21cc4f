"""Host-side pins of the mutual-check matcher: the expected-value helper itself, the C-ABI
declarations and bindings, the config switches and the drop-in routing without a GPU."""

import dataclasses
import inspect
import json
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from tests import mutual_ref
from tests.conftest import GOLDEN, ROOT
from visualodometry_amd import _lib, matcher
from visualodometry_amd.dropin import hooks

sys.path.insert(0, str(ROOT / "visualodometry_amd" / "dropin"))
from config.config import VOConfig, get_config  # noqa: E402


def _hand_case():
    """4 queries, 3 train rows on a line (dim 2).  Distances to train rows (t0, t1, t2) =
    ((0,0), (10,0), (100,0)):
      q0 = (1,0):   1, 9, 99    -> forward (0, 0); ratio 1/9
      q1 = (-1,0):  1, 11, 101  -> forward (1, 0); ratio 1/11  (many-to-one with q0 on t0)
      q2 = (12,0):  12, 2, 88   -> forward (2, 1); ratio 2/12
      q3 = (97,0):  97, 87, 3   -> forward (3, 2); ratio 3/87
    Reverse nearest: t0 has q0 and q1 both at distance 1 -- an exact query-side tie, the lower
    index q0 wins; t1 -> q2; t2 -> q3.  So the cross check drops (1, 0) only."""
    d0 = np.array([[1, 0], [-1, 0], [12, 0], [97, 0]], np.float32)
    d1 = np.array([[0, 0], [10, 0], [100, 0]], np.float32)
    return d0, d1


def test_helper_on_a_hand_built_case():
    d0, d1 = _hand_case()
    np.testing.assert_array_equal(mutual_ref.forward(d0, d1, 0.75, "c"), [[0, 0], [1, 0], [2, 1], [3, 2]])
    np.testing.assert_array_equal(mutual_ref.reverse_nearest(d0, d1, "c"), [0, 2, 3])
    kept, n_forward = mutual_ref.mutual(d0, d1, 0.75, "c")
    np.testing.assert_array_equal(kept, [[0, 0], [2, 1], [3, 2]])
    assert n_forward == 4 and mutual_ref.informative(kept, n_forward)
    # the integer oracle agrees on integer-valued rows (shifted into 0..255)
    s0, s1 = d0 + 1, d1 + 1
    kept_i, n_i = mutual_ref.mutual(s0, s1, 0.75, "int")
    np.testing.assert_array_equal(kept_i, kept)
    assert n_i == 4
    # empty sides
    e = np.zeros((0, 2), np.float32)
    assert mutual_ref.mutual(e, d1)[0].shape == (0, 2) and mutual_ref.mutual(d0, e)[0].shape == (0, 2)


def test_header_declares_and_lib_binds_the_entries():
    text = _lib.HEADER.read_text()
    assert re.search(r"\bint\s+vo_match_mutual\s*\(", text)
    assert re.search(r"\bint\s+vo_match_mutual_batch_async\s*\(", text)
    assert re.search(r"#define\s+VO_MATCH_DEVICE_PTRS\s+1\b", text)
    assert re.search(r"#define\s+VO_ABI_VERSION\s+1\b", text)  # additive: the ABI version stays
    assert _lib.VO_MATCH_DEVICE_PTRS == 1
    lib = _lib.load()
    for name in ("vo_match_mutual", "vo_match_mutual_batch_async"):
        assert name in _lib.SIGNATURES
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES["vo_match_mutual"][1]) == 11
    assert len(_lib.SIGNATURES["vo_match_mutual_batch_async"][1]) == 9


def test_python_entries_take_cross_check_defaulting_off():
    for fn in (matcher.match_knn2_ratio, matcher.match_batch_device):
        p = inspect.signature(fn).parameters["cross_check"]
        assert p.default is False


def test_config_defaults_are_off_and_equal_the_reference(monkeypatch):
    monkeypatch.delenv("VO_AMD_SP_BF", raising=False)
    c = VOConfig()
    assert c.match_cross_check is False and c.superpoint_bf_match is False and c.superpoint_bf_ratio == 0.75
    ref = json.loads((GOLDEN / "reference_config.json").read_text())
    ours = dataclasses.asdict(get_config("kitti"))
    for k, v in ref["get_config"]["kitti"].items():
        assert ours[k] == v, k
    assert ours["superpoint_bf_match"] is False and ours["match_cross_check"] is False


def test_env_switch_sets_the_field(monkeypatch):
    monkeypatch.setenv("VO_AMD_SP_BF", "1")
    assert get_config("kitti").superpoint_bf_match is True
    monkeypatch.setenv("VO_AMD_SP_BF", "0")
    assert get_config("kitti").superpoint_bf_match is False


class _Front:
    def __init__(self, **conf):
        self.conf = SimpleNamespace(**conf)

    def match_frames(self, f0, f1):
        return "original"


def test_routing():
    patched = hooks._wrap_match_frames(_Front.match_frames)
    assert patched(_Front(extractor_type="superpoint"), {}, {}) == "original"
    assert patched(_Front(extractor_type="superpoint", superpoint_bf_match=False), {}, {}) == "original"
    assert patched(_Front(extractor_type="other", superpoint_bf_match=True), {}, {}) == "original"
    from tests.conftest import gpu_available

    if gpu_available():
        return  # with a GPU the route itself is covered by tests/test_gpu_dropin_superpoint.py
    d = {"descriptors": np.zeros((1, 5, 256), np.float32)}
    with pytest.raises(_lib.VoError):  # the HIP library or nothing: never a CPU path
        patched(_Front(extractor_type="superpoint", superpoint_bf_match=True), d, d)
    d = {"descriptors": np.zeros((1, 5, 128), np.float32)}
    with pytest.raises(_lib.VoError):
        patched(_Front(extractor_type="sift", match_on_gpu=True, match_cross_check=True), d, d)
