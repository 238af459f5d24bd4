"""The public surface of frame_ops, checked without a GPU: C ABI symbols and struct sizes, the ouster.sdk.core.frame_ops module,
every validation error with the reference's message through Python (tests/cpp/frame_ops_snippet.cpp does the same through
C++, compiled and linked against include/ouster/core/frame_ops.h), the metadata functions on a real metadata file, and the
loud failure of pixel work without a GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import cpp_tools
import frame_ops_model as M
from conftest import ROOT, has_gpu
from ouster_sdk_amd import _capi as capi

sys.path.insert(0, os.path.join(ROOT, "ouster_sdk_amd", "compat"))

META = os.path.join(ROOT, "tests", "golden", "pcaps", "OS-0-128-U1_v2.3.0_1024x10.json")
SYMBOLS = ["ouster_hip_frame_ops_invalid_bits", "ouster_hip_frame_ops_clip", "ouster_hip_frame_ops_invalidate",
           "ouster_hip_frame_ops_select_rows", "ouster_hip_frame_ops_clip_host", "ouster_hip_frame_ops_invalidate_host",
           "ouster_hip_frame_ops_select_rows_host"]


def test_symbols_are_declared_and_exported():
    L = capi.load_hip()
    header = open(os.path.join(ROOT, "include", "ouster_hip.h")).read()
    for name in SYMBOLS:
        assert name in capi.ABI_SYMBOLS and hasattr(L, name) and ("int " + name + "(") in header, name
    assert C.sizeof(capi.FopsPlane) == 40 and C.sizeof(capi.FopsPred) == 72   # LP64 layout of the C structs


def test_invalid_bits_truncate_toward_zero_and_refuse_what_does_not_fit():
    L = capi.load_hip()
    out = C.c_uint64()
    for dt, tag in capi.FOPS_TYPES.items():
        for v in (0.0, 1.9, 100.5, -0.9):
            capi.check(L.ouster_hip_frame_ops_invalid_bits(tag, v, C.byref(out)))
            want = M.cast_invalid(v, dt)
            assert out.value == int(np.array([want]).view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[want.itemsize])[0]), (dt, v)
    for dt, v in [("uint8", 256.0), ("uint8", -1.0), ("int8", -129.0), ("uint16", 65536.0), ("int32", 2.0 ** 31), ("uint32", 2.0 ** 32),
                  ("uint64", 2.0 ** 64), ("int64", 2.0 ** 63), ("uint32", float("nan")), ("int16", float("inf")), ("float32", 1e39)]:
        with pytest.raises(ValueError, match="does not fit a field of type"):
            capi.check(L.ouster_hip_frame_ops_invalid_bits(capi.FOPS_TYPES[dt], v, C.byref(out)))
        with pytest.raises(ValueError):
            M.cast_invalid(v, dt)
    capi.check(L.ouster_hip_frame_ops_invalid_bits(capi.F32, float("inf"), C.byref(out)))
    assert out.value == 0x7F800000
    capi.check(L.ouster_hip_frame_ops_invalid_bits(capi.I8, -128.9, C.byref(out)))
    assert out.value == 0x80


def _frame(h=8, w=32):
    from ouster_sdk_amd import core
    info = core.SensorInfo()
    f = info.format
    f.pixels_per_column, f.columns_per_frame, f.columns_per_packet = h, w, 16
    f.pixel_shift_by_row = [0] * h
    info.format = f
    info.beam_azimuth_angles = [0.0] * h
    info.beam_altitude_angles = [float(i) for i in range(h)]
    info.prod_line = "OS-1-%d" % h
    types = [core.FieldType("RANGE", np.uint32), core.FieldType("REFLECTIVITY", np.uint8),
             core.FieldType("PER_COL", np.uint32, (), core.FieldClass.COLUMN_FIELD)]
    fr = core.LidarFrame(info, types)
    fr.field("RANGE")[:] = np.arange(h * w, dtype=np.uint32).reshape(h, w)
    fr.field("REFLECTIVITY")[:] = (np.arange(h * w) % 200).astype(np.uint8).reshape(h, w)
    return info, fr


def test_module_imports_with_the_reference_names():
    import ouster.sdk.core.frame_ops as fo
    for name in ("clip", "filter_field", "filter_uv", "filter_xyz", "mask", "select_by_index", "select_by_index_metadata",
                 "reduce_by_factor", "reduce_by_factor_metadata"):
        assert callable(getattr(fo, name)), name
    from ouster_sdk_amd import core
    assert core.reduce_factor_to_indices(128, 128) == [64]
    assert core.reduce_factor_to_indices(2, 8) == [0, 2, 4, 6]


def test_validation_errors_carry_the_reference_messages():
    import ouster.sdk.core.frame_ops as fo
    from ouster_sdk_amd import core
    info, fr = _frame()
    before = {n: np.array(fr.field(n)) for n in ("RANGE", "REFLECTIVITY", "PER_COL")}
    cases = [
        ("beam indices can't be empty", lambda: fo.select_by_index(fr, [])),
        ("beam indices can't contain duplicates", lambda: fo.select_by_index(fr, [1, 1])),
        (r"beam indices \[8, -1\] must be in the range \[0, 8\)", lambda: fo.select_by_index(fr, [0, 8, -1])),
        ("beam indices can't be empty", lambda: fo.select_by_index_metadata(info, [])),
        (r"beam indices \[9\] must be in the range \[0, 8\)", lambda: core.select_by_index_metadata(info, [9])),
        ("beam indices can't contain duplicates", lambda: core.select_by_index(fr, [2, 2])),
        ("factor == 0 can't be negative", lambda: fo.reduce_by_factor(fr, 0)),
        ("factor == 3 must be a divisor of 8", lambda: fo.reduce_by_factor_metadata(info, 3)),
        ("factor == 0 can't be negative", lambda: core.reduce_factor_to_indices(0, 8)),
        ("factor == 5 must be a divisor of 8", lambda: core.reduce_by_factor(fr, 5)),
        ("coord_2d == x must be either 'u' or 'v'", lambda: fo.filter_uv(fr, "x", 0, 1)),
        ("coord_2d == w must be either 'u' or 'v'", lambda: core._frame_ops_filter_uv(fr, "w", 0, 1, 0, [], False)),
        (r"lower == 0 and upper == 9 must be in the range \[0, 8\]", lambda: fo.filter_uv(fr, "u", 0, 9)),
        (r"lower == -1 and upper == 4 must be in the range \[0, 32\]", lambda: fo.filter_uv(fr, "v", -1, 4)),
        (r"lower == 0 and upper == 33 must be in the range \[0, 32\]", lambda: core._frame_ops_filter_uv(fr, "v", 0, 33, 0, [], False)),
        ("lower == 5 must be less than upper == 2", lambda: fo.filter_uv(fr, "u", 5, 2)),
        ("lower == 24 must be less than upper == 8", lambda: fo.filter_uv(fr, "v", 0.75, 0.25)),
        ("lower == 5 must be less than upper == 2", lambda: core._frame_ops_filter_uv(fr, "u", 5, 2, 0, [], False)),
        ("doesn't match frame size", lambda: fo.mask(fr, [], np.ones((8, 33), np.uint8))),
        ("Used mask size doesn't match frame size", lambda: core._frame_ops_mask(fr, [], np.ones((9, 32), np.uint8))),
        (r"Only PIXEL_FIELD frame fields are supported here; requested non-pixel fields: \[PER_COL\]",
         lambda: fo.clip(fr, ["RANGE", "PER_COL"], 0, 1)),
        (r"Only PIXEL_FIELD frame fields are supported here; requested non-pixel fields: \[PER_COL\]",
         lambda: fo.filter_field(fr, "RANGE", 0, 1, 0, ["PER_COL", "MISSING"])),
        (r"Only PIXEL_FIELD frame fields are supported here; requested non-pixel fields: \['PER_COL'\]",
         lambda: fo.filter_xyz(fr, lambda r: np.zeros((8, 32, 3)), 0, 0, 1, 0, ["PER_COL"])),
        (r"axis_idx == 3 must be in the range \[0, 2\]", lambda: fo.filter_xyz(fr, lambda r: None, 3)),
        ("filter_field requires a pixel field with shape", lambda: fo.filter_field(fr, "PER_COL", 0, 1)),
        ("invalid == 256 does not fit a field of type UINT8", lambda: fo.clip(fr, [], 0, 1, 256)),
        ("invalid == -1 does not fit a field of type UINT32", lambda: fo.filter_field(fr, "RANGE", 0, 1, -1, ["RANGE"])),
        ("invalid == 300 does not fit a field of type UINT8", lambda: fo.filter_uv(fr, "u", 0, 1, 300)),
    ]
    for message, call in cases:
        with pytest.raises(ValueError, match=message):
            call()
    for n, a in before.items():
        assert np.array_equal(np.array(fr.field(n)), a), n


def test_metadata_functions_on_a_real_metadata_file():
    import ouster.sdk.core.frame_ops as fo
    from ouster_sdk_amd import core
    info = core.SensorInfo(open(META).read())
    h = info.format.pixels_per_column
    assert h == 128 and info.prod_line == "OS-0-128"
    indices = [127, 3, 64]
    sel = fo.select_by_index_metadata(info, indices)
    assert sel.format.pixels_per_column == 3 and sel.format.columns_per_frame == info.format.columns_per_frame
    assert list(sel.format.pixel_shift_by_row) == [info.format.pixel_shift_by_row[i] for i in indices]
    assert list(sel.beam_azimuth_angles) == [info.beam_azimuth_angles[i] for i in indices]
    assert list(sel.beam_altitude_angles) == [info.beam_altitude_angles[i] for i in indices]
    assert sel.prod_line == "OS-0-3"
    assert info.format.pixels_per_column == 128 and len(info.beam_altitude_angles) == 128   # the source is left alone
    for factor in (1, 2, 4, 128):
        red = fo.reduce_by_factor_metadata(info, factor)
        idx = M.reduce_factor_to_indices(factor, h)
        assert core.reduce_factor_to_indices(factor, h) == idx
        assert red.format.pixels_per_column == len(idx)
        assert list(red.beam_altitude_angles) == [info.beam_altitude_angles[i] for i in idx]
        assert list(red.format.pixel_shift_by_row) == [info.format.pixel_shift_by_row[i] for i in idx]
        assert red.prod_line == "OS-0-%d" % len(idx)


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_pixel_work_without_a_gpu_raises_and_leaves_the_frame():
    import ouster.sdk.core.frame_ops as fo
    info, fr = _frame()
    before = {n: np.array(fr.field(n)) for n in ("RANGE", "REFLECTIVITY")}
    calls = [lambda: fo.clip(fr, [], 10, 20), lambda: fo.filter_field(fr, "RANGE", 10, 20), lambda: fo.filter_uv(fr, "u", 0, 4),
             lambda: fo.filter_uv(fr, "v", 0, 4), lambda: fo.mask(fr, [], np.zeros((8, 32), np.uint8)),
             lambda: fo.filter_xyz(fr, lambda r: np.zeros((8, 32, 3)), 0), lambda: fo.select_by_index(fr, [0, 1]),
             lambda: fo.reduce_by_factor(fr, 2)]
    for call in calls:
        with pytest.raises(RuntimeError):
            call()
    for n, a in before.items():
        assert np.array_equal(np.array(fr.field(n)), a), n


def test_cpp_caller_compiles_links_and_runs():
    """tests/cpp/frame_ops_snippet.cpp, built by tests/cpp/Makefile with the flags of the other C++ tests and -Werror: every
    validation error through C++, the metadata functions, and the pixel work (or its refusal without a GPU)."""
    p = cpp_tools.run("frame_ops_snippet", [META], timeout=300)
    assert "meta 128 OS-0-128 -> 32 OS-0-32" in p.stdout, p.stdout
    assert p.stdout.splitlines()[-1].startswith("ok" if has_gpu() else "no-gpu"), p.stdout
