"""The public surface of the RGB display images, checked without a GPU: C ABI symbols and the record's layout, the ouster.sdk.core
names and constructor shapes, every argument error (through the C ABI, C++ and Python, with nothing written), the loud failure
without a GPU (no CPU fallback), a C++ caller that compiles with -Werror, and the host half -- LocalToneMapper::step and
AutoExposure::step fed the model's luminance statistics -- against tests/tonemap_model.py bit for bit."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

import cpp_tools
import tonemap_cases as K
import tonemap_model as M
from conftest import ROOT, has_gpu
from ouster_sdk_amd import _capi as capi

sys.path.insert(0, os.path.join(ROOT, "ouster_sdk_amd", "compat"))

SYMBOLS = ["ouster_hip_image_lum_percentiles", "ouster_hip_image_tonemap", "ouster_hip_image_lum_percentiles_host",
           "ouster_hip_image_tonemap_host", "ouster_hip_image_apply_rgb_host"]


def test_symbols_and_record_layout():
    L = capi.load_hip()
    for name in SYMBOLS:
        assert name in capi.ABI_SYMBOLS and hasattr(L, name), name
    assert C.sizeof(capi.TonemapParams) == 48 and capi.TonemapParams.color_ramp.offset == 40 and capi.F16 == 12
    p = M.Params(M.MAP_AFFINE, 0.25, 3.0, 0.1, True, 0.5, False)
    rec = capi.TonemapParams.from_buffer_copy(K.pack_params(p))
    assert (rec.map.mode, rec.map.sub, rec.map.mul, rec.map.add, rec.compress, rec.color_correct, rec.color_ramp) == (2, 0.25, 3.0, 0.1, 1, 0, 0.5)


def last_error():
    return capi.load_hip().ouster_hip_last_error().decode()


def test_c_abi_refuses_bad_arguments_before_it_looks_for_a_gpu():
    """ctx NULL throughout (no context can exist without a GPU): the message tells which check spoke, and nothing is written"""
    L = capi.load_hip()
    img = np.full(64 * 64 * 3, 0.5, np.float32)
    out = np.full(64 * 64 * 3, -7.25, np.float32)
    rec = capi.TonemapParams()
    n, lo_hi = (C.c_uint32 * 1)(7), (C.c_float * 2)(-7.25, -7.25)
    pi, po = img.ctypes.data, out.ctypes.data

    def tm(in_type=capi.F32, out_type=capi.F32, h=64, w=64, src=pi, dst=po, params=C.addressof(rec), in_stride=0, out_stride=0):
        return L.ouster_hip_image_tonemap(None, src, in_type, dst, out_type, 1, h, w, in_stride, out_stride, params)

    for call, what in ((lambda: tm(in_type=capi.U16), "in_type"), (lambda: tm(out_type=capi.U8), "out_type"),
                       (lambda: tm(in_type=capi.F16, out_type=capi.F64), "in_type"), (lambda: tm(in_type=capi.F64), "in_type"),
                       (lambda: tm(h=7), "at least 8 x 8"), (lambda: tm(w=7), "at least 8 x 8"), (lambda: tm(h=0), "at least 8 x 8"),
                       (lambda: tm(src=None), "NULL image"), (lambda: tm(dst=None), "out is NULL"), (lambda: tm(params=None), "params is NULL"),
                       (lambda: tm(in_stride=100), "image_stride"), (lambda: tm(out_stride=100), "out_stride"),
                       (lambda: tm(dst=pi, out_stride=64 * 64 * 3 + 4), "in place"), (lambda: tm(), "ctx is NULL")):
        assert call() == capi.ERR_INVALID_ARGUMENT and what in last_error(), (what, last_error())
    assert L.ouster_hip_image_tonemap(None, pi, capi.F32, po, capi.F32, 0, 64, 64, 0, 0, None) == 0     # no images: nothing to do
    # h * w = 2^31 is allowed, a tile of 2^25 pixels is not: the reference's float counts stop at 2^24
    assert L.ouster_hip_image_tonemap(None, pi, capi.F32, po, capi.F32, 1, 1 << 15, 1 << 16, 0, 0, C.addressof(rec)) == -4
    assert "2^24" in last_error()
    assert L.ouster_hip_image_tonemap_host(None, pi, capi.F32, po, capi.F32, 1 << 15, 1 << 16, C.addressof(rec)) == -4 and "2^24" in last_error()

    def pc(in_type=capi.F32, out_type=capi.F32, src=pi, lo=0.1, hi=0.2, cnt=n, res=lo_hi):
        return L.ouster_hip_image_lum_percentiles(None, src, in_type, out_type, 1, 64, 64, 0, lo, hi, cnt, res)

    for call, what in ((lambda: pc(in_type=capi.U32), "in_type"), (lambda: pc(src=None), "NULL image"), (lambda: pc(cnt=None), "NULL output"),
                       (lambda: pc(res=None), "NULL output"), (lambda: pc(lo=0.6, hi=0.4), "percentiles"), (lambda: pc(lo=-0.1), "percentiles"),
                       (lambda: pc(), "ctx is NULL")):
        assert call() == capi.ERR_INVALID_ARGUMENT and what in last_error(), (what, last_error())
    for call, what in ((lambda: L.ouster_hip_image_tonemap_host(None, pi, capi.F32, po, capi.F32, 7, 64, C.addressof(rec)), "at least 8 x 8"),
                       (lambda: L.ouster_hip_image_tonemap_host(None, pi, capi.F16, pi, capi.F32, 64, 64, C.addressof(rec)), "in place"),
                       (lambda: L.ouster_hip_image_tonemap_host(None, pi, capi.F32, po, capi.F32, 64, 64, None), "params is NULL"),
                       (lambda: L.ouster_hip_image_tonemap_host(None, None, capi.F32, po, capi.F32, 64, 64, C.addressof(rec)), "NULL image"),
                       (lambda: L.ouster_hip_image_apply_rgb_host(None, pi, capi.U8, po, capi.F32, 64, 64, None), "in_type"),
                       (lambda: L.ouster_hip_image_apply_rgb_host(None, pi, capi.F32, None, capi.F32, 64, 64, None), "NULL image"),
                       (lambda: L.ouster_hip_image_lum_percentiles_host(None, pi, capi.F32, capi.U16, 64, 64, 0.1, 0.2, n, lo_hi), "F32 or F64"),
                       (lambda: L.ouster_hip_image_lum_percentiles_host(None, pi, capi.F16, capi.F64, 64, 64, 0.1, 0.2, n, lo_hi), "in_type"),
                       (lambda: L.ouster_hip_image_lum_percentiles_host(None, pi, capi.F64, capi.F32, 64, 64, 0.1, 0.2, n, lo_hi), "in_type"),
                       (lambda: L.ouster_hip_image_lum_percentiles_host(None, pi, capi.F32, capi.F32, 64, 64, 0.7, 0.4, n, lo_hi), "percentiles"),
                       (lambda: L.ouster_hip_image_lum_percentiles_host(None, pi, capi.F32, capi.F32, 64, 64, 0.1, 0.2, None, lo_hi), "bad image"),
                       (lambda: L.ouster_hip_image_tonemap_host(None, pi, capi.F32, po, capi.F32, 64, 64, C.addressof(rec)), "ctx is NULL")):
        assert call() == capi.ERR_INVALID_ARGUMENT and what in last_error(), (what, last_error())
    assert (out == -7.25).all() and (img == 0.5).all() and n[0] == 7 and lo_hi[0] == -7.25


def test_compat_names_constructors_and_shape_errors():
    from ouster.sdk.core import AutoExposure, LocalToneMapper
    import ouster_sdk_amd.core as core
    assert LocalToneMapper is core.LocalToneMapper
    LocalToneMapper()
    LocalToneMapper(3)
    LocalToneMapper(update_every=3)
    LocalToneMapper(0.0, 0.2, 1, 0.3, True, False)
    LocalToneMapper(0.0, 0.2, 1, 0.3, 0.25, True)
    LocalToneMapper(lo_percentile=0.0, hi_percentile=0.2, update_every=1, damping=0.3, compress_dr=True, color_correct=True)
    LocalToneMapper(lo_percentile=0.0, hi_percentile=0.2, update_every=1, damping=0.3, compress_dr_max_lum=0.3, color_correct=True)
    with pytest.raises(TypeError):
        LocalToneMapper(0.0, 0.2, 1, 0.3, compress_dr=True, compress_dr_max_lum=0.2, color_correct=True)
    for dtype in (np.float16, np.float32, np.float64):
        for obj in (LocalToneMapper(), AutoExposure()):
            for shape in ((16, 16, 4), (16, 16, 1)):
                keep = np.ones(shape, dtype)
                with pytest.raises(ValueError, match="Expected an H x W x 3 array"):
                    obj.update(keep)
                assert (keep == 1).all()
        for shape in ((7, 64, 3), (64, 7, 3)):
            with pytest.raises(ValueError, match="at least 8"):
                LocalToneMapper().update(np.ones(shape, dtype))
        with pytest.raises(ValueError, match="Expected an H x W x 3 array"):
            LocalToneMapper().update(np.ones((16, 16), dtype))
    with pytest.raises(TypeError):
        LocalToneMapper().update(np.ones((16, 16, 3), np.uint16))
    with pytest.raises(TypeError):
        LocalToneMapper().update(np.ones((16, 3, 16), np.float32).transpose(0, 2, 1))      # not C-contiguous: nothing is converted
    with pytest.raises(TypeError):
        AutoExposure().update(np.ones(8, np.float32))                                      # the single-channel rule stands


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
@pytest.mark.parametrize("dtype", [np.float16, np.float32, np.float64])
def test_update_without_a_gpu_raises_and_leaves_the_image(dtype):
    from ouster.sdk.core import AutoExposure, LocalToneMapper
    img = (np.arange(1, 32 * 64 * 3 + 1) % 251 / 100).astype(dtype).reshape(32, 64, 3)
    keep = img.copy()
    for obj in (LocalToneMapper(), AutoExposure()):
        with pytest.raises(capi.OusterHipError):
            obj.update(img)
        assert np.array_equal(img, keep)
        assert not obj.initialized


def test_cpp_caller_compiles_links_and_runs():
    """tests/cpp/tonemap_snippet.cpp, built by tests/cpp/Makefile with the flags of the other snippets, -Werror among them"""
    p = cpp_tools.run("tonemap_snippet", [], timeout=300)
    assert p.stdout.startswith("ok" if has_gpu() else "no-gpu"), p.stdout


def test_eigen_tensor_maps_bind_where_the_mirror_takes_rgb_img_ref():
    """tests/cpp/tonemap_eigen_snippet.cpp with -DOUSTER_HIP_USE_EIGEN over the mocked Tensor module: temporaries of
    Eigen::TensorMap<rgb_img_t<T>>, const and not, in the reference's own call spelling"""
    assert cpp_tools.run("tonemap_eigen_snippet", [], timeout=300).stdout.strip() == "ok"


def steps(tmp_path, kind, model, calls):
    """the C++ host half over the model's recorded statistics -> [(record bytes, lo_state, hi_state)]"""
    src, dst = tmp_path / "steps.in", tmp_path / "steps.out"
    with open(src, "wb") as f:
        f.write(struct.pack("<4I4d", kind, model.update_every, int(getattr(model, "color_correct", True)), len(calls),
                            model.lo_percentile, model.hi_percentile, model.damping, getattr(model, "compress_dr_max_lum", 0.0)))
        for (n, lo, hi), flag in calls:
            f.write(struct.pack("<2I2d", n, int(flag), lo, hi))
    cpp_tools.run("tonemap_snippet", ["steps", src, dst])
    raw = open(dst, "rb").read()
    size = (48 if kind == 0 else 32) + 16
    assert len(raw) == size * len(calls)
    return [(raw[i * size:(i + 1) * size - 16], struct.unpack("<2d", raw[(i + 1) * size - 16:(i + 1) * size])) for i in range(len(calls))]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_half_equals_the_model_over_twelve_calls(tmp_path, dtype):
    for name, kw, const_first in K.LTM_CONFIGS:
        model, twin = M.LocalToneMapperModel(**kw), M.LocalToneMapperModel(**kw)
        calls, states = [], []
        for img, flag in K.frames(32, 64, dtype, seed=11, const_first=const_first):
            model.update(img, flag)
            calls.append((model.stats[-1] or (0, 0.0, 0.0), flag))
            states.append((model.lo_state, model.hi_state))
        assert len(calls) == 12
        got = steps(tmp_path, 0, twin, calls)
        for i, (rec, st) in enumerate(got):
            assert rec == K.pack_params(model.params[i]), (name, i, model.branches[i])
            assert st == states[i], (name, i)
    for kw, const_first in K.AE_CONFIGS:
        model = M.RgbAutoExposureModel(**kw)
        calls, states = [], []
        for img, flag in K.frames(32, 64, dtype, seed=12, const_first=const_first):
            model.update(img, flag)
            calls.append((model.stats[-1] or (0, 0.0, 0.0), flag))
            states.append((model.lo_state, model.hi_state))
        got = steps(tmp_path, 1, model, calls)
        for i, (rec, st) in enumerate(got):
            assert rec == K.pack_map(model.params[i]), (kw, i, model.branches[i])
            assert st == states[i], (kw, i)
