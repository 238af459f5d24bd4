"""The public surface of interp_pose / transform, checked without a GPU: C ABI symbols, the host half (ouster_hip_pose_segments)
against the table of tests/pose_model.py on every fixture case, every validation error with the reference's message through
the C ABI, through Python and through C++ (tests/cpp/pose_snippet.cpp, compiled and linked against
include/ouster/core/pose_util.h), and the loud failure of the per-x work without a GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import cpp_tools
import pose_model as M
from conftest import ROOT, has_gpu
from ouster_sdk_amd import _capi as capi

sys.path.insert(0, os.path.join(ROOT, "ouster_sdk_amd", "compat"))

SYMBOLS = ["ouster_hip_pose_segments", "ouster_hip_pose_validate", "ouster_hip_interp_pose", "ouster_hip_interp_pose_host", "ouster_hip_interp_pose_pair_host",
           "ouster_hip_interp_pose_columns", "ouster_hip_interp_pose_pair_columns", "ouster_hip_transform", "ouster_hip_transform_host"]
VECTORS = np.load(os.path.join(ROOT, "tests", "golden", "pose_vectors.npz"))
CASES = sorted({k.split("/")[0] for k in VECTORS.files})


def ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def segments(x_known, poses):
    xk = np.ascontiguousarray(x_known, dtype=np.float64)
    po = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 16)
    out = np.full((max(len(xk) - 1, 1), 24), np.nan)
    capi.check(capi.load_hip().ouster_hip_pose_segments(ptr(xk), ptr(po), len(xk), out.ctypes.data))
    return out


def test_symbols_are_declared_and_exported():
    L = capi.load_hip()
    header = open(os.path.join(ROOT, "include", "ouster_hip.h")).read()
    for name in SYMBOLS:
        assert name in capi.ABI_SYMBOLS and hasattr(L, name) and ("int " + name + "(") in header, name


@pytest.mark.parametrize("case", CASES)
def test_pose_segments_match_the_model_table(case):
    xk, poses = VECTORS[case + "/x_known"], VECTORS[case + "/poses_known"]
    got = segments(xk, poses)
    truth = VECTORS[case + "/table_truth"]
    assert got.shape == truth.shape == (len(xk) - 1, 24)
    assert np.array_equal(got[:, 0], xk[:-1]) and np.array_equal(got[:, 1:17], poses[:-1]) and np.all(got[:, 23] == 0.0)
    lim = M.bound(None, VECTORS[case + "/table_err"], VECTORS[case + "/table_scale"])
    err = np.abs(got - truth).max()
    model = M.segments_table(xk, poses)
    print("%s: |table - truth| = %.3g (allowed %.3g), |table - float64 model| = %.3g" % (case, err, lim, np.abs(got - model).max()))
    assert err <= lim


def test_pose_segments_on_the_reference_data():
    import json
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "interp_pose_reference.json")))
    got = segments(g["x_known"], g["poses_known"])
    assert np.abs(got - M.segments_table(g["x_known"], g["poses_known"])).max() <= 1e-15


def test_c_abi_validation_comes_before_the_gpu():
    """ctx is NULL in every call: a validation error must win over it, which shows that nothing touched the GPU"""
    L = capi.load_hip()
    eye = np.tile(np.eye(4).reshape(16), (4, 1))
    out = np.zeros((4, 24))
    x = np.array([0.0, 2.0, 1.0])

    def known(xk, k=None):
        xk = np.array(xk, dtype=np.float64)
        return ptr(xk), ptr(eye), len(xk) if k is None else k, xk

    for message, xk in ((M.MSG_FEW, [1.0]), (M.MSG_FEW, []), (M.MSG_KNOWN, [1.0, 1.0]), (M.MSG_KNOWN, [1.0, 2.0, 3.0, 2.5]),
                        (M.MSG_KNOWN, [2.0, 1.0])):
        a, b, k, keep = known(xk)
        for call in (lambda: L.ouster_hip_pose_segments(a, b, k, out.ctypes.data),
                     lambda: L.ouster_hip_pose_validate(a, b, k, None, 0),
                     lambda: L.ouster_hip_interp_pose(None, None, 3, a, b, k, capi.F64, None),
                     lambda: L.ouster_hip_interp_pose_host(None, ptr(x), 3, a, b, k, capi.F64, out.ctypes.data),
                     lambda: L.ouster_hip_interp_pose_columns(None, None, None, 1, 3, a, b, k, None, None)):
            with pytest.raises(ValueError, match=message):
                capi.check(call())
        del keep
    for call in (lambda: L.ouster_hip_interp_pose_pair_host(None, ptr(x), 3, 1.0, ptr(eye), 1.0, ptr(eye), capi.F64, out.ctypes.data),
                 lambda: L.ouster_hip_interp_pose_pair_columns(None, None, None, 1, 3, 5.0, ptr(eye), 5.0 + 1e-17, ptr(eye), None, None)):
        with pytest.raises(ValueError, match=M.MSG_DURATION):
            capi.check(call())
    assert np.all(out == 0.0)
    xk = np.array([0.0, 5.0])
    with pytest.raises(ValueError, match="x_interp values must be monotonically increasing: 1.000000 < 2.000000"):
        capi.check(L.ouster_hip_pose_validate(ptr(xk), ptr(eye), 2, ptr(x), 3))
    capi.check(L.ouster_hip_pose_validate(ptr(xk), ptr(eye), 2, ptr(np.sort(x)), 3))


def test_python_face_shapes_and_errors():
    import ouster.sdk.core as core
    from ouster_sdk_amd import core as amd
    assert core.interp_pose is amd.interp_pose and core.interp_pose_float is amd.interp_pose_float and core.transform is amd.transform
    eye = np.tile(np.eye(4), (3, 1, 1))
    cases = [
        (ValueError, M.MSG_FEW, lambda: core.interp_pose(np.zeros(2), np.array([1.0]), eye[:1])),
        (ValueError, M.MSG_KNOWN, lambda: core.interp_pose(np.zeros(2), np.array([1.0, 1.0]), eye[:2])),
        (ValueError, M.MSG_KNOWN, lambda: core.interp_pose_float(np.zeros(0), np.array([1.0, 2.0, 1.5]), eye.astype(np.float32))),
        (ValueError, "x_interp values must be monotonically increasing: 1.000000 < 2.000000",
         lambda: core.interp_pose(np.array([[0.0], [2.0], [1.0]]), np.array([0.0, 5.0]), eye[:2])),
        (RuntimeError, r"x_interp must have shape \(N,\) or \(N,1\)", lambda: core.interp_pose(np.zeros((2, 2)), np.array([0.0, 1.0]), eye[:2])),
        (RuntimeError, r"x_known must have shape \(N,\) or \(N,1\)", lambda: core.interp_pose(np.zeros(2), np.zeros((2, 2)), eye[:2])),
        (RuntimeError, "The number of poses in poses_known must match the number of values in x_known",
         lambda: core.interp_pose(np.zeros(2), np.array([0.0, 1.0]), eye)),
        (TypeError, "poses_known must have shape", lambda: core.interp_pose(np.zeros(2), np.array([0.0, 1.0]), np.zeros((2, 16)))),
        (ValueError, r"points array must have shape \(n, 3\) or \(h, w, 3\)", lambda: core.transform(np.zeros((4, 2)), np.eye(4))),
        (ValueError, r"points array must have shape \(n, 3\) or \(h, w, 3\)", lambda: core.transform(np.zeros((4, 3, 2, 3)), np.eye(4))),
        (TypeError, "points and pose must be floating-point arrays", lambda: core.transform(np.zeros((4, 3), np.int32), np.eye(4))),
        (TypeError, "pose must have shape", lambda: core.transform(np.zeros((4, 3)), np.eye(3))),
    ]
    for exc, message, call in cases:
        with pytest.raises(exc, match=message):
            call()


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_per_x_work_without_a_gpu_raises():
    import ouster.sdk.core as core
    eye = np.tile(np.eye(4), (2, 1, 1))
    for call in (lambda: core.interp_pose(np.array([0.0, 0.5]), np.array([0.0, 1.0]), eye),
                 lambda: core.interp_pose_float(np.array([0.5]), np.array([0.0, 1.0]), eye.astype(np.float32)),
                 lambda: core.transform(np.zeros((4, 3)), np.eye(4)),
                 lambda: core.transform(np.zeros((2, 2, 3), np.float32), np.eye(4, dtype=np.float32))):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(RuntimeError):
        capi.Context(0)


def test_cpp_caller_compiles_links_and_runs():
    """tests/cpp/pose_snippet.cpp, built by tests/cpp/Makefile with the flags of the other C++ tests and -Werror"""
    p = cpp_tools.run("pose_snippet", [], timeout=300)
    assert "validation ok" in p.stdout, p.stdout
    assert p.stdout.splitlines()[-1].startswith("ok" if has_gpu() else "no-gpu"), p.stdout
