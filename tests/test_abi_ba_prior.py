"""The pose-prior entry point through the layers that need no GPU: declared in the product header
with the documented signature, exported, bound in ``_lib.SIGNATURES``; the struct has the header's
layout; every argument error that needs no device is VO_ERR_ARG before a context is touched; the
Python knobs default to off and check their shapes."""

import ctypes as C
import re

import numpy as np
import pytest

from visualodometry_amd import _lib
from visualodometry_amd.ba import BAWindow, PosePrior, _prior_struct, _problem_struct


def _header():
    return re.sub(r"/\*.*?\*/", "", _lib.HEADER.read_text(), flags=re.S)


def test_entry_point_is_declared_exported_and_bound():
    m = re.search(r"\bint\s+vo_ba_setup_prior\s*\(([^)]*)\)\s*;", _header())
    assert m, "vo_ba_setup_prior is not declared in include/vo_hip.h"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == [
        "vo_ctx* ctx", "const vo_ba_problem* prob", "const vo_ba_pose_prior* prior", "uint64_t* session_out"]
    assert _lib.SIGNATURES["vo_ba_setup_prior"] == (
        C.c_int, [C.c_void_p, C.POINTER(_lib.BAProblemC), C.POINTER(_lib.BAPosePriorC), C.POINTER(C.c_uint64)])
    m = re.search(r"\bint\s+vo_ba_marginalize\s*\(([^)]*)\)\s*;", _header())
    assert m, "vo_ba_marginalize is not declared in include/vo_hip.h"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == [
        "vo_ctx* ctx", "uint64_t session", "int n_drop", "double lambda", "int32_t* n_prior_out", "double* info_out",
        "double* rhs_out", "double* poses0_out", "double* cost0_out", "uint8_t* point_marg_out"]
    PD = C.POINTER(C.c_double)
    assert _lib.SIGNATURES["vo_ba_marginalize"] == (
        C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_double, C.POINTER(C.c_int32), PD, PD, PD, PD, C.POINTER(C.c_uint8)])
    for name in ("vo_ba_setup_prior", "vo_ba_marginalize"):
        assert hasattr(_lib.load(), name), f"{name} not exported by libvo_hip.so"
        for header in (_lib.TEST_HEADER, _lib.TEST_HEADER.with_name("vo_hip_testing_chain.h")):
            assert name not in header.read_text()


def test_abi_version_and_profile_ids_unchanged():
    text = _lib.HEADER.read_text()
    m = re.search(r"#define\s+VO_ABI_VERSION\s+(\d+)", text)
    assert m and int(m.group(1)) == 1
    m = re.search(r"#define\s+VO_PROFILE_KERNELS\s+(\d+)", text)
    assert m and int(m.group(1)) == 25


def test_pose_prior_layout():
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*vo_ba_pose_prior\s*;", _header())
    assert m, "vo_ba_pose_prior is not declared"
    fields = [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == ["int32_t n_poses", "int32_t reserved", "const double* info", "const double* rhs",
                      "const double* poses0", "double cost0"]
    PD = C.POINTER(C.c_double)
    assert [(n, t) for n, t in _lib.BAPosePriorC._fields_] == [
        ("n_poses", C.c_int32), ("reserved", C.c_int32), ("info", PD), ("rhs", PD), ("poses0", PD), ("cost0", C.c_double)]
    assert C.sizeof(_lib.BAPosePriorC) == 40


def test_header_states_the_semantics():
    text = _lib.HEADER.read_text()
    doc = text[text.index("Pose prior."):text.index("int vo_ba_setup_prior")]
    for phrase in ("cost0 - 2 eta^T xi + xi^T Lambda xi", "first-order Jacobian", "(S + Lambda^) dc = b + (eta^ - Lambda^ xi^)",
                   "prior == NULL is vo_ba_setup itself", "K <= 10"):
        assert phrase in doc, phrase


def _problem(n_poses=4, n_fixed=1):
    ptr_ = np.array([0, 2, 4], dtype=np.int32)
    cam = np.array([0, 1, 2, 3], dtype=np.int32)
    uv = np.zeros((4, 2), dtype=np.float32)
    return _problem_struct(np.diag([500.0, 500.0, 1.0]), ptr_, cam, uv, n_poses, n_fixed, 1.0), (ptr_, cam, uv)


def _good(k=2):
    return PosePrior(np.eye(6 * k), np.zeros(6 * k), np.tile(np.eye(4), (k, 1, 1)), 0.0)


def _setup(prob, pc):
    sid = C.c_uint64(7)
    rc = _lib.load().vo_ba_setup_prior(None, C.byref(prob), C.byref(pc) if pc is not None else None, C.byref(sid))
    return rc, _lib.load().vo_last_error().decode()


def test_argument_errors_need_no_device():
    """A bad prior is VO_ERR_ARG ahead of the context (here: none at all)."""
    prob, keep = _problem()

    def bad(change):
        pc, arrays = _prior_struct(_good())
        change(pc, arrays)
        rc, msg = _setup(prob, pc)
        assert rc == _lib.VO_ERR_ARG, (rc, msg)
        assert "vo_ba_setup_prior" in msg

    bad(lambda pc, a: setattr(pc, "n_poses", 0))
    bad(lambda pc, a: setattr(pc, "n_poses", -3))
    bad(lambda pc, a: setattr(pc, "n_poses", 4))  # n_poses - n_fixed = 3 free poses
    bad(lambda pc, a: setattr(pc, "reserved", 1))
    bad(lambda pc, a: setattr(pc, "info", None))
    bad(lambda pc, a: setattr(pc, "rhs", None))
    bad(lambda pc, a: setattr(pc, "poses0", None))
    bad(lambda pc, a: setattr(pc, "cost0", float("nan")))
    bad(lambda pc, a: setattr(pc, "cost0", float("inf")))
    bad(lambda pc, a: a[0].__setitem__((7, 3), np.nan))   # info, lower triangle
    bad(lambda pc, a: a[1].__setitem__(11, -np.inf))      # rhs
    bad(lambda pc, a: a[2].__setitem__((1, 9), np.nan))   # poses0
    # a good prior passes these checks: what fails next is the missing context, not an argument of the prior
    pc, arrays = _prior_struct(_good())
    rc, msg = _setup(prob, pc)
    assert rc != _lib.VO_OK and "vo_ba_setup_prior:" not in msg
    # a NaN above the diagonal is not read
    pc, arrays = _prior_struct(_good())
    arrays[0][3, 7] = np.nan
    rc, msg = _setup(prob, pc)
    assert "vo_ba_setup_prior:" not in msg


def test_python_layer_defaults_and_shape_checks():
    w = BAWindow(np.zeros((1, 4, 4)), np.zeros((1, 3)), np.zeros((1, 2), np.float32), np.zeros(1, int), np.zeros(1, int))
    assert w.prior is None
    assert _good(3).n_poses == 3
    for bad in (PosePrior(np.eye(12), np.zeros(11), np.tile(np.eye(4), (2, 1, 1))),
                PosePrior(np.eye(11), np.zeros(12), np.tile(np.eye(4), (2, 1, 1))),
                PosePrior(np.eye(12), np.zeros(12), np.zeros((2, 12)))):
        with pytest.raises(ValueError):
            _prior_struct(bad)
