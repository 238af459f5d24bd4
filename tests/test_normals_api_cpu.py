"""The public surface of algorithm::normals, checked without a GPU: C ABI symbols, the host half (ouster_hip_normals_constants)
bit for bit against tests/normals_model.py -- the same libm on the same machine -- every validation error with the reference's
message through the C ABI, through Python and through C++ (tests/cpp/normals_snippet.cpp, compiled and linked against
include/ouster/algorithm/normals.h), and the loud failure of the pixel work without a GPU."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import cpp_tools
import normals_model as M
from conftest import ROOT, has_gpu
from ouster_sdk_amd import _capi as capi

sys.path.insert(0, os.path.join(ROOT, "ouster_sdk_amd", "compat"))

SYMBOLS = ["ouster_hip_normals_constants", "ouster_hip_normals", "ouster_hip_normals_host"]
X22 = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0], [1.0, 1.0, 0.0]]])
R22 = np.array([[0.0, 1.0], [1.0, 1.0]], np.uint32)


def constants(w, h, angle, target, pair):
    out = capi.NormalsConsts()
    capi.check(capi.load_hip().ouster_hip_normals_constants(w, h, angle, target, 0 if pair is None else 1,
                                                            0.0 if pair is None else pair[0], 0 if pair is None else pair[1],
                                                            C.byref(out)))
    return {k: getattr(out, k) for k, _ in capi.NormalsConsts._fields_}


def bits(d):
    return {k: np.float64(v).view(np.uint64) for k, v in d.items()}


def test_symbols_are_declared_and_exported():
    L = capi.load_hip()
    header = open(os.path.join(ROOT, "include", "ouster_hip.h")).read()
    for name in SYMBOLS:
        assert name in capi.ABI_SYMBOLS and hasattr(L, name) and ("int " + name + "(") in header, name
    assert C.sizeof(capi.NormalsConsts) == 40 and C.sizeof(capi.NormalsDesc) == 10 * 8 + 2 * 8 + 9 * 4 + 4 + 2 * 8


@pytest.mark.parametrize("w,h,angle,target,pair", [
    (1024, 128, M.DEFAULT_MIN_ANGLE_INCIDENCE_RAD, M.DEFAULT_TARGET_DISTANCE_METER, (0.8390715290764524, 127)),
    (2048, 128, 0.1, 100.0, (0.9999999, 3)),
    (7, 5, 1e-9, 0.3, (-0.25, 4)),                        # min_angle below the 1e-6 floor
    (256, 64, 0.5, 0.025, None),                          # no pair: 90 degrees over h - 1 intervals
    (8, 1, 0.1, 1.0, None),                               # h = 1: one interval
    (1, 1, 0.1, 1.0, None),
    (16, 4, 0.1, 1.0, (1.0 + 2.0 ** -52, 2)),             # a dot just above 1: the clamp, not a NaN from acos
    (16, 4, 0.1, 1.0, (-1.0 - 2.0 ** -52, 1)),
    (16, 4, 0.1, 1.0, (float("nan"), 1)),                 # std::min(1.0, NaN) is 1.0
    (16, 4, 0.1, 1.0, (1.0, 3)),                          # subtent 0: px_res_v is +inf
])
def test_constants_equal_the_model_bit_for_bit(w, h, angle, target, pair):
    got, want = constants(w, h, angle, target, pair), M.constants(w, h, angle, target, pair)
    assert set(got) == set(want)
    assert bits(got) == bits(want), (got, want)
    assert not math.isnan(got["subtent"])


def desc(xyz, rng, xyz2=None, rng2=None, origins=None, n_origins=None, angle=0.1, target=100.0, keep=None):
    h, w = rng.shape
    d = capi.NormalsDesc()
    arrays = [np.ascontiguousarray(xyz, np.float64), np.ascontiguousarray(rng, np.uint32), np.zeros((h * w, 3)), np.zeros((h * w, 3))]
    d.xyz, d.range, d.normals = arrays[0].ctypes.data, arrays[1].ctypes.data, arrays[2].ctypes.data
    d.xyz_rows = arrays[0].size // 3
    if xyz2 is not None:
        arrays += [np.ascontiguousarray(xyz2, np.float64), np.ascontiguousarray(rng2, np.uint32)]
        d.xyz2, d.range2, d.normals2 = arrays[4].ctypes.data, arrays[5].ctypes.data, arrays[3].ctypes.data
        d.xyz2_rows = arrays[4].size // 3
        d.range2_h, d.range2_w = arrays[5].shape
    if origins is not None:
        arrays.append(np.ascontiguousarray(origins, np.float64))
        d.sensor_origins = arrays[-1].ctypes.data if arrays[-1].size else arrays[2].ctypes.data
        d.n_origins = len(origins) if n_origins is None else n_origins
    d.n_frames, d.h, d.w = 1, h, w
    d.pixel_search_range, d.xyz_dtype = 1, capi.F64
    d.min_angle_of_incidence_rad, d.target_distance_m = angle, target
    keep.append(arrays)
    return d


def test_c_abi_validation_comes_before_the_gpu():
    """ctx is NULL in every call: a validation error must win over it, which shows that nothing touched the GPU"""
    L = capi.load_hip()
    keep = []
    org = np.zeros((2, 3))
    cases = [
        (M.MSG_XYZ, desc(X22.reshape(-1, 3)[:3], R22, origins=org, keep=keep)),
        (M.MSG_XYZ, desc(X22, R22, X22.reshape(-1, 3)[:3], R22, origins=org, keep=keep)),
        (M.MSG_RANGE2, desc(X22, R22, X22, R22.reshape(1, 4), origins=org, keep=keep)),
        (M.MSG_ORIGINS, desc(X22, R22, origins=np.zeros((0, 3)), keep=keep)),
        (M.MSG_ORIGINS, desc(X22, R22, X22, R22, origins=np.zeros((3, 3)), keep=keep)),
        (M.MSG_TARGET, desc(X22, R22, origins=org, target=-100.0, keep=keep)),
        (M.MSG_TARGET, desc(X22, R22, X22, R22, origins=org, target=0.0, angle=-1.0, keep=keep)),   # target is checked first
        (M.MSG_ANGLE, desc(X22, R22, origins=org, angle=-0.1, keep=keep)),
        (M.MSG_ANGLE, desc(X22, R22, X22, R22, origins=org, angle=0.0, keep=keep)),
        (M.MSG_XYZ, desc(X22, R22[:1], origins=org, target=-1.0, keep=keep)),                        # shapes before parameters
    ]
    for message, d in cases:
        for fn in (L.ouster_hip_normals, L.ouster_hip_normals_host):
            with pytest.raises(ValueError, match=message):
                capi.check(fn(None, C.byref(d)))
    out = capi.NormalsConsts()
    with pytest.raises(ValueError, match=M.MSG_TARGET):
        capi.check(L.ouster_hip_normals_constants(8, 8, 0.1, 0.0, 0, 0.0, 0, C.byref(out)))
    with pytest.raises(ValueError, match=M.MSG_ANGLE):
        capi.check(L.ouster_hip_normals_constants(8, 8, 0.0, 1.0, 0, 0.0, 0, C.byref(out)))
    for arrays in keep:
        assert not arrays[2].any() and not arrays[3].any()


def test_python_face_shapes_and_errors():
    import ouster.sdk.algorithm as algorithm
    from ouster_sdk_amd import core as amd
    assert algorithm.normals is amd.normals
    org = np.zeros((2, 3))
    angle = 0.017453292519943295
    for extra in ((), (X22, R22)):
        cases = [
            (RuntimeError, "target_distance_m must be positive", lambda: amd.normals(X22, R22, *extra, org, 1, angle, -100)),
            (TypeError, "incompatible function arguments", lambda: amd.normals(X22, R22, *extra, np.zeros((0, 0)), 1, angle, 100)),
            (RuntimeError, "normals: sensor_origins size must match image width",
             lambda: amd.normals(X22, R22, *extra, np.zeros((0, 3)), 1, angle, 100)),
            (RuntimeError, "normals: xyz dimensions mismatch",
             lambda: amd.normals(X22, np.array([[0.0, 1.0]], np.uint32), *extra, org, 1, angle, 100)),
            (RuntimeError, "normals: min_angle_of_incidence_rad must be positive", lambda: amd.normals(X22, R22, *extra, org, 1, -0.1, 100)),
            (RuntimeError, "normals: xyz dimensions mismatch",
             lambda: amd.normals(X22.reshape(-1, 3)[:3], R22, *extra, sensor_origins_xyz=org)),
        ]
        for exc, message, call in cases:
            with pytest.raises(exc, match=message):
                call()
    with pytest.raises(RuntimeError, match="normals: range2 dimensions mismatch"):
        amd.normals(X22, R22, X22, R22.reshape(1, 4), sensor_origins_xyz=org)


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_pixel_work_without_a_gpu_raises():
    from ouster_sdk_amd import core as amd
    org = np.zeros((2, 3))
    for call in (lambda: amd.normals(X22, R22, org, 1, 0.1, 100), lambda: amd.normals(X22, R22, X22, R22, org, 1, 0.1, 100),
                 lambda: amd.normals(X22.reshape(4, 3), R22, sensor_origins_xyz=org)):
        with pytest.raises(RuntimeError):
            call()


def test_cpp_caller_compiles_links_and_runs():
    """tests/cpp/normals_snippet.cpp, built by tests/cpp/Makefile with the flags of the other C++ tests and -Werror"""
    p = cpp_tools.run("normals_snippet", [], timeout=300)
    assert "validation ok" in p.stdout, p.stdout
    assert p.stdout.splitlines()[-1].startswith("ok" if has_gpu() else "no-gpu"), p.stdout
