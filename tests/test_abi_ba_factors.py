"""The pose-factor entry point through the layers that need no GPU: declared in the product header
with the documented signature, exported, bound in ``_lib.SIGNATURES``; the struct has the header's
layout; every argument error that needs no device is VO_ERR_ARG before a context is touched; the
Python knobs default to off and check their shapes."""

import ctypes as C
import re

import numpy as np
import pytest

from visualodometry_amd import _lib
from visualodometry_amd.ba import BAWindow, PoseFactor, _factor_array, _problem_struct
from visualodometry_amd.dropin.config.config import VOConfig


def _header():
    return re.sub(r"/\*.*?\*/", "", _lib.HEADER.read_text(), flags=re.S)


def test_entry_point_is_declared_exported_and_bound():
    m = re.search(r"\bint\s+vo_ba_setup_factors\s*\(([^)]*)\)\s*;", _header())
    assert m, "vo_ba_setup_factors is not declared in include/vo_hip.h"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == [
        "vo_ctx* ctx", "const vo_ba_problem* prob", "const vo_ba_pose_prior* prior", "const vo_ba_pose_factor* factors",
        "int32_t n_factors", "uint64_t* session_out"]
    assert _lib.SIGNATURES["vo_ba_setup_factors"] == (
        C.c_int, [C.c_void_p, C.POINTER(_lib.BAProblemC), C.POINTER(_lib.BAPosePriorC), C.POINTER(_lib.BAPoseFactorC),
                  C.c_int32, C.POINTER(C.c_uint64)])
    assert hasattr(_lib.load(), "vo_ba_setup_factors"), "vo_ba_setup_factors not exported by libvo_hip.so"
    for header in (_lib.TEST_HEADER, _lib.TEST_HEADER.with_name("vo_hip_testing_chain.h")):
        assert "vo_ba_setup_factors" not in header.read_text()
    # the model stands ahead of the entry point
    text = _lib.HEADER.read_text()
    assert text.index("} vo_ba_pose_factor;") < text.index("int vo_ba_setup_factors")


def test_abi_version_and_profile_ids_unchanged():
    text = _lib.HEADER.read_text()
    m = re.search(r"#define\s+VO_ABI_VERSION\s+(\d+)", text)
    assert m and int(m.group(1)) == 1
    m = re.search(r"#define\s+VO_PROFILE_KERNELS\s+(\d+)", text)
    assert m and int(m.group(1)) == 25


def test_pose_factor_layout():
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*vo_ba_pose_factor\s*;", _header())
    assert m, "vo_ba_pose_factor is not declared"
    fields = [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == ["int32_t cam_i", "int32_t cam_j", "double meas[12]", "double info[36]"]
    assert [(n, t) for n, t in _lib.BAPoseFactorC._fields_] == [
        ("cam_i", C.c_int32), ("cam_j", C.c_int32), ("meas", C.c_double * 12), ("info", C.c_double * 36)]
    assert C.sizeof(_lib.BAPoseFactorC) == 392


def test_header_states_the_semantics():
    text = _lib.HEADER.read_text()
    doc = text[text.index("Pose factors."):text.index("int vo_ba_setup_factors")]
    for phrase in ("xi = log(A Z^-1)", "A = T_i T_j^-1", "first-order Jacobian", "xi' ~ xi + delta_i - G delta_j",
                   "G = Ad(A)", "S_ii += Lambda", "S_jj += G^T Lambda G", "S_ij (row i, column j) += -Lambda G",
                   "b_i  += -Lambda xi", "b_j += G^T Lambda xi", "n_factors == 0 is vo_ba_setup_prior",
                   "VO_BA_MAX_POSE_FACTORS"):
        assert phrase in doc, phrase
    m = re.search(r"#define\s+VO_BA_MAX_POSE_FACTORS\s+(\d+)", text)
    assert m and int(m.group(1)) >= 1024


def _problem(n_poses=4, n_fixed=1):
    ptr_ = np.array([0, 2, 4], dtype=np.int32)
    cam = np.array([0, 1, 2, 3], dtype=np.int32)
    uv = np.zeros((4, 2), dtype=np.float32)
    return _problem_struct(np.diag([500.0, 500.0, 1.0]), ptr_, cam, uv, n_poses, n_fixed, 1.0), (ptr_, cam, uv)


def _good():
    return [PoseFactor(1, 0, np.eye(4), np.eye(6)), PoseFactor(2, -1, np.eye(4), 2.0 * np.eye(6)),
            PoseFactor(1, 3, np.eye(4), np.eye(6))]


def _setup(prob, fa, n):
    sid = C.c_uint64(7)
    rc = _lib.load().vo_ba_setup_factors(None, C.byref(prob), None, fa, n, C.byref(sid))
    return rc, _lib.load().vo_last_error().decode()


def test_argument_errors_need_no_device():
    """A bad factor list is VO_ERR_ARG ahead of the context (here: none at all)."""
    prob, keep = _problem()

    def bad(change, n=None, null=False):
        fa, cnt = _factor_array(_good())
        change(fa)
        rc, msg = _setup(prob, None if null else fa, cnt if n is None else n)
        assert rc == _lib.VO_ERR_ARG, (rc, msg)
        assert "vo_ba_setup_factors" in msg

    bad(lambda fa: None, n=-1)
    bad(lambda fa: None, n=3, null=True)
    bad(lambda fa: setattr(fa[0], "cam_i", 4))
    bad(lambda fa: setattr(fa[0], "cam_i", -1))
    bad(lambda fa: setattr(fa[2], "cam_j", 4))
    bad(lambda fa: setattr(fa[1], "cam_j", -2))
    bad(lambda fa: setattr(fa[0], "cam_j", 1))  # cam_i == cam_j
    bad(lambda fa: fa[1].meas.__setitem__(10, float("nan")))
    bad(lambda fa: fa[1].meas.__setitem__(0, float("inf")))
    bad(lambda fa: fa[2].info.__setitem__(6 * 4 + 1, float("nan")))  # lower triangle
    bad(lambda fa: fa[2].info.__setitem__(35, float("-inf")))        # the diagonal
    # more factors than the documented cap
    cap = int(re.search(r"#define\s+VO_BA_MAX_POSE_FACTORS\s+(\d+)", _lib.HEADER.read_text()).group(1))
    many, n = _factor_array([_good()[0]] * (cap + 1))
    rc, msg = _setup(prob, many, n)
    assert rc == _lib.VO_ERR_ARG and "vo_ba_setup_factors" in msg
    # a good list passes these checks: what fails next is the missing context, not an argument of the factors
    fa, n = _factor_array(_good())
    rc, msg = _setup(prob, fa, n)
    assert rc != _lib.VO_OK and "vo_ba_setup_factors:" not in msg
    many, n = _factor_array([_good()[0]] * cap)
    rc, msg = _setup(prob, many, n)
    assert rc != _lib.VO_OK and "vo_ba_setup_factors:" not in msg
    # a NaN above the diagonal is not read
    fa, n = _factor_array(_good())
    fa[0].info[6 * 1 + 4] = float("nan")
    rc, msg = _setup(prob, fa, n)
    assert "vo_ba_setup_factors:" not in msg


def test_python_layer_defaults_and_shape_checks():
    w = BAWindow(np.zeros((1, 4, 4)), np.zeros((1, 3)), np.zeros((1, 2), np.float32), np.zeros(1, int), np.zeros(1, int))
    assert w.factors is None
    cfg = VOConfig()
    assert cfg.ba_motion_factors is False and cfg.ba_motion_sigma_t > 0 and cfg.ba_motion_sigma_r > 0
    for bad in (PoseFactor(0, 1, np.eye(3), np.eye(6)), PoseFactor(0, 1, np.eye(4), np.eye(5)),
                PoseFactor(0, -1, np.zeros(12), np.eye(6)), PoseFactor(0, 1, np.eye(4), np.zeros(36))):
        with pytest.raises(ValueError):
            _factor_array([bad])
    fa, n = _factor_array(_good())
    assert n == 3 and (fa[1].cam_i, fa[1].cam_j) == (2, -1) and fa[1].info[7] == 2.0 and fa[0].meas[0] == 1.0
