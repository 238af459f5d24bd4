"""RGB display images on the GPU -- the luminance percentiles, LocalToneMapper and the RGB overloads of AutoExposure -- against the
plain-numpy model of tests/tonemap_model.py (never against the product itself), bit for bit: an order statistic of exactly rounded
values has one correct answer, the integer histograms are exact, and every float step is one IEEE operation in a fixed order on
both sides.  tests/test_tonemap_model.py asserts that the sequences used here reach every branch of the model."""
import ctypes as C

import numpy as np
import pytest

import tonemap_cases as K
import tonemap_model as M
from conftest import has_gpu

pytestmark = pytest.mark.gpu

GUARD = -7.25


@pytest.fixture(scope="module")
def gpu():
    import torch
    from ouster_sdk_amd import _capi as capi
    assert has_gpu()
    ctx = capi.Context(0)
    yield capi, ctx, torch
    ctx.close()


def to_dev(torch, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()


def from_dev(t, dtype, shape):
    return t.cpu().numpy().view(dtype).reshape(shape)


def as_T(img):
    """what the kernels compute on: FLOAT16 patterns through the front end, anything else as it is"""
    return M.f16_bits_to_f32(img) if img.dtype == np.uint16 else img


def typed(kind, img):
    """a float64 scene as the input of one of the three forms -> (array, T)"""
    if kind == "f16":
        return K.to_f16_bits(img), np.float32
    return img.astype(np.float32 if kind == "f32" else np.float64), (np.float32 if kind == "f32" else np.float64)


def tags(capi, kind):
    return {"f16": (capi.F16, capi.F32), "f32": (capi.F32, capi.F32), "f64": (capi.F64, capi.F64)}[kind]


# ---- 1. luminance percentiles -------------------------------------------------------------------------------------------------
def percentile_images(rng, kind, h, w):
    imgs = {}
    imgs["normal"] = np.abs(K.scene(rng, h, w, 1.0, np.float64)) + 1e-3                      # every sample positive
    imgs["ties"] = rng.integers(1, 4, (h, w, 1)).astype(np.float64) * np.ones((1, 1, 3))      # three luminances in all
    drop = imgs["normal"].copy()
    drop[rng.random((h, w)) < 0.3] = 0                                                        # dropped pixels: 0 ...
    imgs["dropped"] = drop
    few = np.zeros((h, w, 3))
    idx = rng.choice(h * w // 4, size=min(60, h * w // 8), replace=False) * 4
    few.reshape(-1, 3)[idx] = rng.uniform(0.1, 2.0, (idx.size, 3))
    imgs["few_positive"] = few
    neg = imgs["normal"].copy()
    sel = rng.random((h, w)) < 0.3
    neg[sel, 2] = -20 * neg[sel, 2]                                                           # a channel that drives lum <= 0
    imgs["negative_channel"] = neg
    names = list(imgs)
    stack = []
    for name in names:
        a, _ = typed(kind, imgs[name])
        if kind == "f16" and name == "dropped":
            a.reshape(-1, 3)[::3][a.reshape(-1, 3)[::3, 0] == 0] = 0x7e00                     # ... and as the quiet NaN pattern
        if kind == "f16" and name in ("normal", "few_positive"):
            a = np.ascontiguousarray(imgs[name].astype(np.float16)).view(np.uint16)           # no odd patterns: the counts are the point
        stack.append(a)
    return names, np.stack(stack)


@pytest.mark.parametrize("h,w", [(8, 50), (8, 49), (37, 130), (128, 2048)])
@pytest.mark.parametrize("kind", ["f16", "f32", "f64"])
def test_luminance_percentiles_bit_exact(gpu, kind, h, w):
    capi, ctx, torch = gpu
    rng = np.random.default_rng(h * 13 + w)
    names, batch = percentile_images(rng, kind, h, w)
    in_tag, out_tag = tags(capi, kind)
    T = np.float64 if kind == "f64" else np.float32
    n = len(names)
    d_in = to_dev(torch, batch)
    es = np.dtype(T).itemsize
    d_n = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
    d_lh = torch.zeros(n * 2 * es, dtype=torch.uint8, device="cuda")
    capi.check(ctx.L.ouster_hip_image_lum_percentiles(ctx.h, d_in.data_ptr(), in_tag, out_tag, n, h, w, 0, 0.1, 0.25, d_n.data_ptr(),
                                                      d_lh.data_ptr()))
    ctx.sync()
    got_n, got = from_dev(d_n, np.uint32, (n,)), from_dev(d_lh, T, (n, 2))
    seen = {}
    for i, name in enumerate(names):
        want_n, lo, hi = M.lum_stats(as_T(batch[i]), 0.1, 0.25)
        seen[name] = want_n
        print(kind, h, w, name, "n", got_n[i], want_n, "lo/hi", got[i], lo, hi)
        assert got_n[i] == want_n, (name, got_n[i], want_n)
        assert K.same_bits(got[i], np.array([lo, hi], T)), (name, got[i], lo, hi)
    assert 0 < seen["few_positive"] < 100 and seen["dropped"] < seen["normal"]
    if kind == "f16":
        assert seen["negative_channel"] == seen["normal"]     # the front end knows no sign: the sign bit lands in the exponent
    else:
        assert seen["negative_channel"] < seen["normal"]
    if (h, w) == (8, 50):
        assert seen["normal"] == 100            # exactly the threshold: not the early return
    if (h, w) == (8, 49):
        assert seen["normal"] == 98             # the early return


# ---- 2. single images through ouster_hip_image_tonemap ---------------------------------------------------------------------
def run_tonemap(gpu, kind, images, records, in_place, pad_in=0, pad_out=0):
    """images: equally shaped (h, w, 3) inputs of one form -> ([outputs], the guard elements behind each output)"""
    capi, ctx, torch = gpu
    in_tag, out_tag = tags(capi, kind)
    T = np.float64 if kind == "f64" else np.float32
    n, (h, w, _) = len(images), images[0].shape
    dense = 3 * h * w
    in_stride = dense + pad_in
    out_stride = in_stride if in_place else dense + pad_out
    src = np.full((n, in_stride), 77 if kind == "f16" else GUARD, images[0].dtype)
    for i, img in enumerate(images):
        src[i, :dense] = img.reshape(-1)
    d_in = to_dev(torch, src)
    d_out = d_in if in_place else to_dev(torch, np.full((n, out_stride), GUARD, T))
    d_par = to_dev(torch, np.frombuffer(b"".join(K.pack_params(p) for p in records), np.uint8))
    capi.check(ctx.L.ouster_hip_image_tonemap(ctx.h, d_in.data_ptr(), in_tag, d_out.data_ptr(), out_tag, n, h, w,
                                              in_stride if (pad_in or n > 1) else 0, out_stride if (pad_in or pad_out or n > 1) else 0,
                                              d_par.data_ptr()))
    ctx.sync()
    out = from_dev(d_out, T, (n, out_stride))
    if not in_place:
        assert np.array_equal(from_dev(d_in, src.dtype, src.shape), src)          # the input is left alone
    return [out[i, :dense].reshape(h, w, 3) for i in range(n)], out[:, dense:]


def form_case(path, kind, h, w, seed):
    """K.model_case for one of the three forms -> (input array, record, expected output, branch)"""
    if kind != "f16":
        return K.model_case(path, h, w, np.float32 if kind == "f32" else np.float64, seed)
    level, const, kw = K.PIXEL_PATHS[path]
    rng = np.random.default_rng(seed)
    m = M.LocalToneMapperModel(**kw)
    m.update_f16(np.full((32, 64, 3), 0x35EC, np.uint16) if const else K.to_f16_bits(K.scene(rng, 32, 64, level)))
    bits = K.to_f16_bits(K.scene(rng, h, w, level))
    want = m.update_f16(bits, False)
    return bits, m.params[-1], want, m.branches[-1]


@pytest.mark.parametrize("h,w", [(8, 8), (9, 13), (16, 64), (37, 130), (64, 1024), (128, 2048)])
@pytest.mark.parametrize("kind", ["f16", "f32", "f64"])
def test_single_images_equal_the_model(gpu, kind, h, w):
    """every way through the per-pixel code at every size class: one-pixel tiles, uneven tiles, rows that change inside a lane's
    four pixels, histograms split into bands (64 x 1024: 2 per tile, 128 x 2048: 8)"""
    paths = list(K.PIXEL_PATHS) if h * w <= 64 * 1024 else ["dark", "full"]
    for k, path in enumerate(paths):
        img, p, want, branch = form_case(path, kind, h, w, seed=1000 * k + h)
        outs, guard = run_tonemap(gpu, kind, [img], [p], in_place=kind != "f16", pad_in=0 if k % 2 else 8)
        diff = np.abs(outs[0].astype(np.float64) - want.astype(np.float64)).max()
        print(kind, h, w, path, branch, "max |diff|", diff, "differing elements", int((K.bits(outs[0]) != K.bits(want)).sum()))
        assert K.same_bits(outs[0], want), (path, branch, diff)
        assert (guard == GUARD).all()
        assert want.min() >= 0 and want.max() <= 1


@pytest.mark.parametrize("kind,pad", [("f16", 4), ("f16", 3), ("f32", 4), ("f32", 1), ("f64", 2), ("f64", 3)])
def test_batch_of_five_with_strides_and_guards(gpu, kind, pad):
    """five different images with their own records, one of them the early return (NONE), strides that keep the vector path (a
    multiple of 16 bytes) and strides that do not; the guard elements between the images stay as they were"""
    cases = [form_case(path, kind, 37, 130, seed=7 + k) for k, path in enumerate(["dark", "ramp", "full", "no_color"])]
    images, records, wants = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    extra, _ = typed(kind, K.scene(np.random.default_rng(99), 37, 130, 1.0, np.float64))
    images.insert(2, extra)
    records.insert(2, M.Params())
    wants.insert(2, as_T(extra))
    for in_place in ([False] if kind == "f16" else [True, False]):
        outs, guard = run_tonemap(gpu, kind, images, records, in_place, pad_in=pad, pad_out=pad + 4)
        for i in range(5):
            assert K.same_bits(outs[i], wants[i]), (in_place, i)
        assert (guard == GUARD).all()


def test_histogram_bands_give_the_same_bits(gpu):
    """knob "tonemap_bands": a tile's histogram counted by 1, 3, 16 or 64 workgroups (more bands than a tile has rows among them)
    instead of the launch's own choice -- integer counts, so the same image bit for bit"""
    capi, ctx, torch = gpu
    try:
        for h, w in ((37, 130), (64, 1024)):
            img, p, want, _ = form_case("dark", "f16", h, w, seed=h)
            for bands in (1, 3, 16, 64):
                ctx.set_knob("tonemap_bands", bands)
                outs, _ = run_tonemap(gpu, "f16", [img, img], [p, p], in_place=False)
                assert K.same_bits(outs[0], want) and K.same_bits(outs[1], want), (h, w, bands)
    finally:
        ctx.set_knob("tonemap_bands", 0)


# ---- 3. state sequences through the Python classes (thin bindings of the C++ mirror) ---------------------------------------
def update_form(obj, kind, img, flag):
    """obj.update on one of the three forms -> the result (the in-place forms return their argument)"""
    if kind == "f16":
        return obj.update(img.view(np.float16), flag)      # the classes take float16 arrays; the bits are what counts
    obj.update(img, flag)
    return img


def model_form(m, kind, img, flag):
    if kind == "f16":
        return m.update_f16(img, flag)
    m.update(img, flag)
    return img


@pytest.mark.parametrize("config", range(len(K.LTM_CONFIGS)), ids=[c[0] for c in K.LTM_CONFIGS])
def test_tone_mapper_sequences_match_the_model(gpu, config):
    from ouster_sdk_amd import core
    name, kw, const_first = K.LTM_CONFIGS[config]
    for kind, h, w in (("f32", 32, 64), ("f64", 32, 64), ("f16", 32, 64), ("f32", 64, 1024), ("f16", 64, 1024)):
        args = dict(kw)
        if "compress_dr_max_lum" in args and isinstance(args["compress_dr_max_lum"], bool):
            args["compress_dr"] = args.pop("compress_dr_max_lum")
        obj, m = core.LocalToneMapper(**args), M.LocalToneMapperModel(**kw)
        for i, (img64, flag) in enumerate(K.frames(h, w, np.float64, seed=h + config, const_first=const_first)):
            a, _ = typed(kind, img64)
            if kind == "f16" and i == 7:
                a = np.ascontiguousarray(img64.astype(np.float16)).view(np.uint16)           # keep the nearly black frame black
            b = a.copy()
            got, want = update_form(obj, kind, a, flag), model_form(m, kind, b, flag)
            assert K.same_bits(got, want), (name, kind, h, w, i, m.branches[-1], np.abs(got - want).max())
            assert (obj.lo_state, obj.hi_state) == (m.lo_state, m.hi_state), (name, kind, i)
        assert "early" in m.branches


@pytest.mark.parametrize("config", range(len(K.AE_CONFIGS)))
def test_rgb_auto_exposure_sequences_match_the_model(gpu, config):
    from ouster_sdk_amd import core
    kw, const_first = K.AE_CONFIGS[config]
    for kind in ("f32", "f64", "f16"):
        obj = core.AutoExposure(**kw) if kw else core.AutoExposure()
        m = M.RgbAutoExposureModel(**kw)
        for i, (img64, flag) in enumerate(K.ae_frames(32, 64, np.float64, seed=40 + config, const_first=const_first)):
            a, _ = typed(kind, img64)
            if kind == "f16" and i == 3:
                a = np.ascontiguousarray(img64.astype(np.float16)).view(np.uint16)
            b = a.copy()
            got, want = update_form(obj, kind, a, flag), model_form(m, kind, b, flag)
            assert K.same_bits(got, want), (kind, i, m.branches[-1])
            assert (obj.lo_state, obj.hi_state) == (m.lo_state, m.hi_state), (kind, i)


# ---- 4. update_batch against single updates ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f16", "f32", "f64"])
def test_update_batch_equals_single_updates(gpu, kind):
    from ouster_sdk_amd import core
    fr = K.frames(32, 64, np.float64, seed=5)
    stack = []
    for i, (img64, _) in enumerate(fr):
        a, _ = typed(kind, img64)
        if kind == "f16" and i == 7:
            a = np.ascontiguousarray(img64.astype(np.float16)).view(np.uint16)
        stack.append(a)
    stack = np.stack(stack)
    f64 = kind == "f64"
    for cls, model, kws in ((core.LocalToneMapper, M.LocalToneMapperModel, (dict(), dict(update_every=3))),
                            (core.AutoExposure, M.RgbAutoExposureModel, (dict(update_every=1), dict(update_every=2)))):
        early = False
        for kw in kws:
            batch, single, m = cls(**kw), cls(**kw), model(**kw)
            for flag in (True, False, True):
                got = batch.update_batch(stack.view(np.float16) if kind == "f16" else stack, float64=f64, update_state=flag)
                for i in range(len(stack)):
                    a, b = stack[i].copy(), stack[i].copy()
                    one, want = update_form(single, kind, a, flag), model_form(m, kind, b, flag)
                    assert K.same_bits(one, want) and K.same_bits(np.ascontiguousarray(got[i]), want), (cls.__name__, kw, flag, i, m.branches[-1])
                assert (batch.lo_state, batch.hi_state) == (single.lo_state, single.hi_state) == (m.lo_state, m.hi_state)
            early |= "early" in m.branches
        assert early                                            # an early return in the middle of a batch


# ---- 5. the _host forms: pool memory in place, foreign memory through scratch ------------------------------------------------
def pool_image(capi, shape, dtype):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = capi.load_hip().ouster_hip_host_alloc(n, 1)
    assert p and capi.load_hip().ouster_hip_host_is_pinned(p, n) == 1
    return p, np.ctypeslib.as_array((C.c_uint8 * n).from_address(p)).view(dtype).reshape(shape)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_forms_in_place_and_no_steady_state_allocations(gpu, dtype):
    capi, _, _ = gpu
    from ouster_sdk_amd import core
    src = K.scene(np.random.default_rng(3), 64, 256, 0.7, dtype)
    half = K.to_f16_bits(src)
    p, pooled = pool_image(capi, src.shape, dtype)
    ph, pooled_half = pool_image(capi, src.shape, np.float16)
    try:
        foreign = np.empty_like(src)
        objs = [(core.LocalToneMapper(), core.AutoExposure()) for _ in range(2)]
        halves = [core.LocalToneMapper() for _ in range(2)]
        m_ltm, m_ae, m_half = M.LocalToneMapperModel(), M.RgbAutoExposureModel(), M.LocalToneMapperModel()
        pooled_half[:] = half.view(np.float16)
        for k in range(3):
            pooled[:] = src * dtype(k + 1)
            foreign[:] = src * dtype(k + 1)
            want = (src * dtype(k + 1)).copy()
            for (ltm, ae), img in zip(objs, (pooled, foreign)):
                ae.update(img)
                ltm.update(img)
            m_ae.update(want)
            m_ltm.update(want)
            assert K.same_bits(np.array(pooled), want) and K.same_bits(foreign, want), k
            want_half = m_half.update_f16(half)
            assert K.same_bits(halves[0].update(pooled_half), want_half) and K.same_bits(halves[1].update(half.view(np.float16)), want_half)
        before = capi.alloc_stats()
        for k in range(50):
            pooled[:] = src
            foreign[:] = src
            for (ltm, ae), img in zip(objs, (pooled, foreign)):
                ae.update(img)
                ltm.update(img)
            halves[0].update(pooled_half)
        after = capi.alloc_stats()
        assert after["device_allocs"] == before["device_allocs"] and after["pinned_allocs"] == before["pinned_allocs"]
        assert K.same_bits(np.array(pooled), foreign)
    finally:
        capi.load_hip().ouster_hip_host_free(p)
        capi.load_hip().ouster_hip_host_free(ph)


# ---- 6. the Python face ----------------------------------------------------------------------------------------------------------
def test_python_face(gpu):
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "ouster_sdk_amd", "compat"))
    from ouster.sdk.core import AutoExposure, LocalToneMapper
    half = K.to_f16_bits(K.scene(np.random.default_rng(8), 128, 1024, 0.3)).view(np.float16)
    out = LocalToneMapper().update(half)
    assert out.dtype == np.float32 and out.shape == half.shape
    assert K.same_bits(out, M.LocalToneMapperModel().update_f16(half.view(np.uint16)))
    assert out.min() >= 0 and out.max() <= 1
    ae = AutoExposure().update(half)
    assert ae.dtype == np.float32 and K.same_bits(ae, M.RgbAutoExposureModel().update_f16(half.view(np.uint16)))
    with pytest.raises(ValueError, match="Expected an H x W x 3 array"):
        LocalToneMapper().update(np.ones((64, 64, 4), np.float16))
    with pytest.raises(ValueError):
        LocalToneMapper().update(np.ones((7, 64, 3), np.float16))
