"""Host-side surface of the LM loop's termination: the two C-ABI prototypes load from the built
library, the ctypes struct has the header's layout, and the drop-in configuration carries the three
criteria (all off by default) into SlidingWindowBA.  Field validation needs a session, so it is in
tests/test_gpu_ba_lm_stop.py.
"""

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import ba_lm_stop_ref as sr
from visualodometry_amd import _lib
from visualodometry_amd.ba import BAResult, BASession, SlidingWindowBA
from visualodometry_amd.dropin.config.config import VOConfig

HEADER = (Path(__file__).resolve().parents[1] / "include" / "vo_hip.h").read_text()


def test_prototypes_load():
    lib = _lib.load()
    for name in ("vo_ba_set_lm_stop", "vo_ba_lm_stop_info"):
        assert name in _lib.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SIGNATURES[name][1]
        assert re.search(rf"\bint {name}\(", HEADER)
    assert lib.vo_abi_version() == 1
    for m in ("set_lm_stop", "lm_stop_info"):
        assert callable(getattr(BASession, m))


def test_struct_has_the_headers_layout():
    m = re.search(r"typedef struct \{([^}]*)\} vo_ba_lm_stop;", HEADER)
    assert m, "vo_ba_lm_stop is not in the header"
    ctype = {"double": C.c_double, "int32_t": C.c_int32}
    fields = []
    for decl in m.group(1).split(";"):
        if decl.strip():
            t, names = decl.split(None, 1)
            fields += [(n.strip(), ctype[t]) for n in names.split(",")]
    assert fields == [("ftol", C.c_double), ("xtol", C.c_double), ("max_rejects", C.c_int32), ("reserved", C.c_int32)]
    assert [(n, t) for n, t in _lib.BALmStopC._fields_] == fields
    # two doubles and two 32-bit words, no padding
    assert C.sizeof(_lib.BALmStopC) == 24
    offsets = {n: getattr(_lib.BALmStopC, n).offset for n, _ in fields}
    assert offsets == {"ftol": 0, "xtol": 8, "max_rejects": 16, "reserved": 20}


def test_reason_codes_match_the_header_and_the_restatement():
    want = {"FAILED": _lib.BA_LM_FAILED, "RAN_ALL": _lib.BA_LM_RAN_ALL, "FTOL": _lib.BA_LM_FTOL,
            "XTOL": _lib.BA_LM_XTOL, "REJECTS": _lib.BA_LM_REJECTS}
    for name, value in want.items():
        m = re.search(rf"#define VO_BA_LM_{name}\s+\(?(-?\d+)\)?", HEADER)
        assert m and int(m.group(1)) == value, name
    assert (sr.FAILED, sr.RAN_ALL, sr.FTOL, sr.XTOL, sr.REJECTS) == (-1, 0, 1, 2, 3)
    assert {k: _lib.BA_LM_REASONS[k] for k in sr.REASONS} == sr.REASONS


def test_config_criteria_are_off_by_default_and_reach_the_ba():
    cfg = VOConfig()
    assert (cfg.ba_lm_ftol, cfg.ba_lm_xtol, cfg.ba_lm_max_rejects) == (0.0, 0.0, 0)
    K = np.eye(3)
    ba = SlidingWindowBA(K, cfg)
    assert (ba.lm_ftol, ba.lm_xtol, ba.lm_max_rejects) == (0.0, 0.0, 0)
    cfg.ba_lm, cfg.ba_lm_ftol, cfg.ba_lm_xtol, cfg.ba_lm_max_rejects = True, 1e-3, 1e-4, 3
    ba = SlidingWindowBA(K, cfg)
    assert ba.lm and (ba.lm_ftol, ba.lm_xtol, ba.lm_max_rejects) == (1e-3, 1e-4, 3)
    ba = SlidingWindowBA(K, lm=True, lm_ftol=1e-2, lm_max_rejects=2)
    assert (ba.lm_ftol, ba.lm_xtol, ba.lm_max_rejects) == (1e-2, 0.0, 2)
    for bad in (dict(lm_ftol=1.0), dict(lm_ftol=-1e-3), dict(lm_ftol=float("nan")), dict(lm_xtol=-1.0),
                dict(lm_xtol=float("inf")), dict(lm_max_rejects=-1)):
        with pytest.raises(ValueError):
            SlidingWindowBA(K, lm=True, **bad)
    r = BAResult(np.zeros((0, 4, 4)), np.zeros((0, 3)))
    assert r.lm_trials is None and r.lm_stop is None
