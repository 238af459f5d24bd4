"""The display-image kernels (k_img_colmask, k_img_dark_rows, k_img_percentiles, k_img_apply) through the C ABI at ragged shapes,
with strides, offset pointers and every input type, bit for bit against the plain-numpy models of tests/image_cases.py and
tests/image_model.py; the refusals of capi_image.hip; the classes on small images and at the 4096-column limit of the dark-row
median.  tests/test_image_cases_cpu.py holds the precondition of every case used here."""
import ctypes as C

import numpy as np
import pytest

import image_cases as ic
from conftest import has_gpu
from image_cases import MAP_AFFINE, MAP_NONE, MAP_SCALE, NP, Map, same_bits, same_bits_or_nan
from image_model import AutoExposureModel, BeamUniformityModel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    from ouster_sdk_amd import _capi as capi
    assert has_gpu()
    ctx = capi.Context(0)
    yield capi, ctx, torch
    ctx.close()


def check_apply(gpu, imgs, in_name, out_name, dark, maps, in_stride=0, out_stride=0, in_off=0, out_off=0, in_place=False):
    """one ouster_hip_image_apply against apply_model per image; gaps, lead and guard keep the sentinel; the input survives a
    call that is not in place.  -> the output images"""
    n, h, w = imgs.shape
    T = NP[out_name]
    out, src = ic.call_apply(gpu, imgs, in_name, out_name, dark, maps, in_stride, out_stride, in_off, out_off, in_place)
    if in_place:
        out_stride, out_off = in_stride, in_off
    got, clean = ic.unpack(out, T, n, h, w, out_stride, out_off)
    assert clean, "a store outside the images"
    for i in range(n):
        want = ic.apply_model(imgs[i], in_name, T, dark[i] if dark is not None else None, maps[i] if maps is not None else None)
        assert same_bits_or_nan(got[i], want), (i, np.flatnonzero(ic.bits(got[i]).reshape(-1) != ic.bits(want).reshape(-1))[:8])
    if not in_place:
        assert np.array_equal(src, ic.pack(imgs.astype(NP[in_name], copy=False), in_stride, in_off))
    return got


# ---- apply --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_name", ["f32", "f64"])
@pytest.mark.parametrize("h,w", ic.APPLY_RAGGED)
def test_apply_ragged_shapes(gpu, h, w, out_name):
    """1 and 3 images; NONE / SCALE / AFFINE with use_dark 1 / 0 / 1 in one call, and maps == NULL; into a second buffer and in
    place.  Three dense images with hw % 4 != 0 take the scalar path, one image the vector path with a scalar tail."""
    T = NP[out_name]
    rng = np.random.default_rng(31 * h + w)
    imgs = ic.apply_images(rng, 3, h, w, T)
    dark = ic.apply_dark(rng, 3, h, T)
    runs = [(imgs[i:i + 1], dark[i:i + 1], [m]) for i, m in enumerate(ic.THREE_MAPS)] + [(imgs, dark, ic.THREE_MAPS)]
    for im, dk, maps in runs:
        for mp in (maps, None):
            for in_place in (False, True):
                check_apply(gpu, im, out_name, out_name, dk, mp, in_place=in_place)
    check_apply(gpu, imgs, out_name, out_name, None, ic.THREE_MAPS)            # use_dark set, no dark counts given
    same = check_apply(gpu, imgs, out_name, out_name, None, None, in_place=True)   # nothing to do: the early return
    assert same_bits_or_nan(same, imgs)


@pytest.mark.parametrize("h,w", ic.APPLY_TYPE_SHAPES)
@pytest.mark.parametrize("in_name,out_name", ic.APPLY_INT_TYPES + [("f16", "f32")])
def test_apply_input_types(gpu, h, w, in_name, out_name):
    """u8 / u16 / u32 converted like astype(T) (u32 -> f32 rounds to nearest even), FLOAT16 patterns by the integer formula; NONE
    into another buffer is a converting copy"""
    T = NP[out_name]
    rng = np.random.default_rng(h + w)
    n = 3
    if in_name == "f16":
        pats = ic.f16_patterns()
        imgs = rng.choice(pats, (n, h, w))
        if n * h * w >= pats.size:
            imgs.reshape(-1)[:pats.size] = pats
        top = 131072.0
    else:
        top = float(np.iinfo(NP[in_name]).max)
        imgs = rng.integers(0, int(top) + 1, (n, h, w)).astype(NP[in_name])
        imgs.reshape(n, -1)[:, :3] = [0, int(top), min(int(top), 2 ** 24 + 1)]
    dark = (rng.uniform(0, 0.5, (n, h)) * top).astype(T)
    maps = [Map(MAP_NONE, 0, 0.0, 1.0, 0.0), Map(MAP_SCALE, 1, 0.0, 1.5 / top, 0.0), Map(MAP_AFFINE, 1, 0.1 * top, 2.0 / top, 0.05)]
    got = check_apply(gpu, imgs, in_name, out_name, dark, maps)
    assert same_bits(got[0], ic.to_T(imgs[0], in_name, T))
    copy = check_apply(gpu, imgs, in_name, out_name, None, None)
    assert same_bits(copy, ic.to_T(imgs, in_name, T))
    check_apply(gpu, imgs, in_name, out_name, dark, None)
    check_apply(gpu, imgs[:1], in_name, out_name, dark[:1], maps[2:])


@pytest.mark.parametrize("in_name", ["f32", "u8", "u16"])
def test_apply_strides_and_alignment(gpu, in_name):
    """4 images of 6 x 64 with in / out strides of hw, hw + 1, hw + 4, and plane / output pointers off by one element: every
    case takes the path it names, leaves gaps and guards alone, and the vector and the scalar runs give the same bytes"""
    n, h, w = ic.STRIDE_SHAPE
    hw = h * w
    rng = np.random.default_rng(5)
    top = {"u8": 255, "u16": 65535}.get(in_name)
    imgs = ic.apply_images(rng, n, h, w, np.float32) if top is None else rng.integers(0, top + 1, (n, h, w)).astype(NP[in_name])
    scale = 1.0 / 60.0 if top is None else 1.5 / top
    dark = ic.apply_dark(rng, n, h, np.float32) if top is None else (rng.uniform(0, 0.5, (n, h)) * top).astype(np.float32)
    maps = [Map(MAP_SCALE, 1, 0.0, scale, 0.0), Map(MAP_AFFINE, 0, 3.0, scale, 0.1), Map(MAP_NONE, 1, 0.0, 1.0, 0.0),
            Map(MAP_AFFINE, 1, 3.0, scale, 0.1)]
    es = np.dtype(NP[in_name]).itemsize
    results, paths = [], set()
    for case_type, si, so, ioff, ooff, path in ic.STRIDE_CASES:
        if case_type != in_name:
            continue
        assert ic.expect_vec(in_name, n, h, w, hw + si, hw + so, ioff * es, ooff * 4) == (path == "vector")
        paths.add(path)
        results.append(check_apply(gpu, imgs, in_name, "f32", dark, maps, hw + si, hw + so, ioff * es, ooff * 4))
        if in_name == "f32" and si == so and ooff == 0:
            results.append(check_apply(gpu, imgs, in_name, "f32", dark, maps, hw + si, hw + so, ioff * es, in_place=True))
    assert paths == {"vector", "scalar"}
    for r in results[1:]:
        assert same_bits_or_nan(r, results[0])


@pytest.mark.parametrize("case", ic.GRID_CASES, ids=lambda c: c["path"])
def test_apply_grid_stride(gpu, case):
    """1024 images get 8 blocks each and want 9: the grid-stride loop runs again.  Every image has its own content, dark counts
    and multiplier, so a lane that picks up another image's chunk changes bits."""
    n, h, w = case["n"], case["h"], case["w"]
    nchunk, want, cap = ic.launch_shape(n, h, w)
    assert want > cap and ic.expect_vec("f32", n, h, w) == (case["path"] == "vector")
    rng = np.random.default_rng(h)
    base = rng.normal(50, 40, (h, w)).astype(np.float32)
    imgs = base[None] + np.arange(n, dtype=np.float32)[:, None, None]
    dark = rng.uniform(0, 60, (n, h)).astype(np.float32)
    dark[:, 1] = np.float32(1e9)
    maps = [Map(MAP_SCALE, 1, 0.0, 1.0 / (200.0 + 1.5 * i), 0.0) for i in range(n)]
    got = check_apply(gpu, imgs, "f32", "f32", dark, maps)
    assert len({got[i].tobytes() for i in range(n)}) == n and ((got > 0) & (got < 1)).mean() > 0.5


def pool_image(capi, shape, dtype):
    """an image at the start of a pool block (requests below OUSTER_HIP_HOST_POOL_MIN would be plain malloc memory)"""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = capi.load_hip().ouster_hip_host_alloc(max(nbytes, 4096), 1)
    assert p and capi.load_hip().ouster_hip_host_is_pinned(p, nbytes) == 1
    return p, np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(p)).view(dtype).reshape(shape)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("h,w", ic.HOST_SHAPES)
def test_apply_host_on_foreign_and_pool_memory(gpu, h, w, dtype):
    """ouster_hip_image_apply_host in place on a numpy array and on pool memory, map NULL (dark counts only) and AFFINE; no
    allocation after the first call"""
    capi, ctx, _ = gpu
    T = NP[dtype]
    rng = np.random.default_rng(h * w)
    src = ic.apply_images(rng, 1, h, w, T)[0]
    dark = ic.apply_dark(rng, 1, h, T)[0]
    affine = ic.THREE_MAPS[2]
    rec = capi.ImageMap(affine.mode, affine.use_dark, affine.sub, affine.mul, affine.add)
    p, pooled = pool_image(capi, (h, w), T)
    try:
        foreign = np.empty_like(src)
        before = None
        for k in range(21):
            for m, m_arg in ((None, None), (affine, C.addressof(rec))):
                want = ic.apply_model(src, dtype, T, dark, m)
                for img in (foreign, pooled):
                    img[:] = src
                    capi.check(ctx.L.ouster_hip_image_apply_host(ctx.h, img.ctypes.data, ic.tag(capi, dtype), h, w, dark.ctypes.data, m_arg))
                    if k in (0, 20):
                        assert same_bits_or_nan(np.array(img), want), (k, m)
            if k == 0:
                before = capi.alloc_stats()
        after = capi.alloc_stats()
        assert after["device_allocs"] == before["device_allocs"] and after["pinned_allocs"] == before["pinned_allocs"]
    finally:
        capi.load_hip().ouster_hip_host_free(p)


# ---- dark rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_name,out_name", ic.DARK_TYPES)
@pytest.mark.parametrize("h,w", ic.DARK_SHAPES)
def test_dark_rows_edges(gpu, h, w, in_name, out_name):
    """w below, at and above one wave and one block, h == 2, word-edge masks, both parities of n_cols, -0.0 differences; the
    whole batch dense, one image, three images with strides hw + 1 / hw + 4 and with the plane pointer off by one element"""
    T = NP[out_name]
    names, imgs, n_cols = ic.dark_images(h, w, in_name)
    want = [ic.medians_model(img.astype(T)) for img in imgs]
    assert [nc for _, nc in want] == n_cols
    hw, es = h * w, np.dtype(NP[in_name]).itemsize
    last3 = slice(len(names) - 3, len(names))
    runs = [(slice(0, len(names)), 0, 0, True), (slice(0, 1), 0, 0, False), (slice(0, 3), hw + 1, 0, True),
            (slice(0, 3), hw + 4, 0, True), (last3, 0, es, True), (last3, hw + 4, es, False)]
    for sel, stride, off, with_nc in runs:
        idx = list(range(len(names)))[sel]
        med, nc = ic.call_dark_rows(gpu, imgs[sel], in_name, out_name, stride, off, with_nc)
        k = len(idx)
        for j, i in enumerate(idx):
            got = med[j * (h - 1):(j + 1) * (h - 1)]
            assert same_bits(got, want[i][0]), (names[i], stride, off, got[:4], want[i][0][:4])
        assert np.array_equal(nc[:k], n_cols[idx[0]:idx[-1] + 1]) if with_nc else same_bits(nc[:k], ic.sentinel_of(np.uint32, k))
        assert same_bits(med[k * (h - 1):], ic.sentinel_of(T, ic.GUARD)) and same_bits(nc[k:], ic.sentinel_of(np.uint32, ic.GUARD))


# ---- percentiles --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_name,out_name", ic.PCT_TYPES)
@pytest.mark.parametrize("h,w", ic.PCT_SHAPES)
def test_percentiles_shapes_fills_and_pairs(gpu, h, w, in_name, out_name):
    """every fill (all positive, mixed signs, one key, adjacent floats, subnormal next to inf, one positive sample) as one batch,
    once per percentile pair"""
    T = NP[out_name]
    fills = [f for f in ic.PCT_FILLS if ic.pct_image(f, h, w, in_name) is not None]
    imgs = np.stack([ic.pct_image(f, h, w, in_name) for f in fills])
    k = len(fills)
    for lo, hi in ic.PCT_PAIRS:
        n, lo_hi = ic.call_percentiles(gpu, imgs, in_name, out_name, lo, hi)
        for i, f in enumerate(fills):
            want_n, want = ic.percentiles_model(imgs[i].astype(T), lo, hi)
            assert n[i] == want_n, (f, lo, hi, n[i], want_n)
            assert same_bits(lo_hi[2 * i:2 * i + 2], want), (f, lo, hi, lo_hi[2 * i:2 * i + 2], want)
        assert same_bits(n[k:], ic.sentinel_of(np.uint32, ic.GUARD)) and same_bits(lo_hi[2 * k:], ic.sentinel_of(T, ic.GUARD))


@pytest.mark.parametrize("case", ic.PCT_NAMED, ids=lambda c: c.name)
def test_percentiles_named_cases(gpu, case):
    h, w = case.shape
    for in_name, out_name in ic.PCT_TYPES:
        img = ic.pct_image(case.fill, h, w, in_name)
        if img is None:
            continue
        T = NP[out_name]
        n, lo_hi = ic.call_percentiles(gpu, img[None], in_name, out_name, *case.pair)
        want_n, k_lo, k_hi, kept = ic.pct_named_ranks(case, in_name, out_name)
        srt = np.sort(kept)
        assert n[0] == want_n and same_bits(lo_hi[:2], np.array([srt[k_lo], srt[k_hi]], T)), (in_name, n[0], lo_hi[:2], k_lo, k_hi)


@pytest.mark.parametrize("out_name", ["f32", "f64"])
@pytest.mark.parametrize("h,w", ic.PCT_DARK_SHAPES)
def test_percentiles_dark_counts_and_strides(gpu, h, w, out_name):
    """the sample is corrected by the dark count of ITS row, (4 j) // w, at widths that are no multiple of 4; three images
    hw + 3 elements apart"""
    T = NP[out_name]
    rng = np.random.default_rng(h * 7 + w)
    imgs = rng.normal(100, 10, (3, h, w)).astype(T)
    dark = rng.uniform(80, 105, (3, h)).astype(T)
    dark[:, ::3] = T(1e9)
    zeroed = False
    for stride in (0, h * w + 3):
        for lo, hi in ((0.1, 0.1), (0.0, 0.0), (0.5, 0.49)):
            n, lo_hi = ic.call_percentiles(gpu, imgs, out_name, out_name, lo, hi, dark, stride)
            for i in range(3):
                want_n, want = ic.percentiles_model(imgs[i], lo, hi, dark[i])
                assert n[i] == want_n and same_bits(lo_hi[2 * i:2 * i + 2], want), (i, stride, lo, hi, n[i], want_n)
                zeroed |= want_n < ic.percentiles_model(imgs[i], lo, hi)[0]
    assert zeroed


# ---- the classes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("h,w", ic.CLASS_SHAPES)
def test_classes_on_small_and_ragged_images(gpu, h, w, dtype):
    """buc.update(img); ae.update(img), six calls, against the models: image, dark counts, lo_state, hi_state"""
    from ouster_sdk_amd import core
    buc, m_buc = core.BeamUniformityCorrector(), BeamUniformityModel()
    ae, m_ae = core.AutoExposure(0.1, 0.1, 1, 0.5), AutoExposureModel(0.1, 0.1, 1, 0.5)
    for i, img in enumerate(ic.class_sequence(h, w, dtype)):
        a, b = img.copy(), img.copy()
        buc.update(a)
        m_buc.update(b)
        assert same_bits(a, b), i
        assert np.array_equal(buc.dark_count, m_buc.dark_count), i
        ae.update(a)
        m_ae.update(b)
        assert same_bits(a, b), (i, m_ae.branches[-1])
        assert (ae.lo_state, ae.hi_state, ae.initialized) == (m_ae.lo_state, m_ae.hi_state, m_ae.initialized), i
    if (h, w) == (1, 400):
        assert m_ae.branches[0] == "early" and m_ae.branches[1] != "early"      # 99 positive samples, then exactly 100
    if h * w < 400:
        assert set(m_ae.branches) == {"early"}


def narrow_sequence(dtype):
    rng = np.random.default_rng(23)
    flags = [1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 0, 1]
    return [((rng.normal(100, 10, (32, 256)) + rng.normal(0, 3, (32, 1)) + i).astype(dtype), bool(f)) for i, f in enumerate(flags)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_width_limit_refuses_before_any_state_changes(gpu, dtype):
    """A 2 x 4100 image is wider than the dark-row median takes: update() and update_batch() raise, the image keeps its bytes,
    and the object goes on as if the call had not happened -- a fresh object, and one three calls into a sequence."""
    capi, _, _ = gpu
    from ouster_sdk_amd import core
    rng = np.random.default_rng(1)
    wide = rng.normal(100, 10, (2, 4100)).astype(dtype)
    keep = wide.copy()

    def refused(buc):
        with pytest.raises(capi.OusterHipError, match="wider than 4096"):
            buc.update(wide)
        assert same_bits(wide, keep)
        ae = core.AutoExposure()
        with pytest.raises(capi.OusterHipError, match="wider than 4096"):
            buc.update_batch(np.stack([wide, wide]), float64=dtype == np.float64, then=ae)
        assert same_bits(wide, keep) and not ae.initialized and (ae.lo_state, ae.hi_state) == (-1.0, -1.0)

    buc, m = core.BeamUniformityCorrector(), BeamUniformityModel()
    refused(buc)
    assert buc.dark_count.size == 0
    for i, (img, flag) in enumerate(narrow_sequence(dtype)):
        if i == 3:
            state = buc.dark_count.copy()
            refused(buc)
            assert np.array_equal(buc.dark_count, state)
        a, b = img.copy(), img.copy()
        buc.update(a, flag)
        m.update(b, flag)
        assert same_bits(a, b), i
        assert np.array_equal(buc.dark_count, m.dark_count), i       # the counter too: call 8 of the model updates them
    # a call that needs no new dark counts (known height, not the 8th update) never reaches the median: any width passes
    buc2, m2 = core.BeamUniformityCorrector(), BeamUniformityModel()
    for img in (wide[:, :256].copy(), wide.copy()):
        b = img.copy()
        buc2.update(img)
        m2.update(b)
        assert same_bits(img, b) and np.array_equal(buc2.dark_count, m2.dark_count)
    # AutoExposure has no such limit
    ae, m_ae = core.AutoExposure(), AutoExposureModel()
    a, b = wide.copy(), wide.copy()
    ae.update(a)
    m_ae.update(b)
    assert same_bits(a, b) and (ae.lo_state, ae.hi_state) == (m_ae.lo_state, m_ae.hi_state)
    assert m_ae.branches[0] in ("affine", "hi") and not same_bits(a, wide)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_calls_leave_the_outputs_alone(gpu):
    """every fail(...) branch of capi_image.hip by return code and message, and the calls with nothing to do"""
    capi, ctx, torch = gpu
    L = ctx.L
    U8, U16, U64, F16, F32, F64 = capi.U8, capi.U16, capi.U64, capi.F16, capi.F32, capi.F64
    INV, UNS = capi.ERR_INVALID_ARGUMENT, capi.ERR_UNSUPPORTED
    h = w = 8
    d_in = ic.to_dev(torch, np.ones((2, h, w + 1), np.float32))
    outs = {k: ic.to_dev(torch, np.full(4096, ic.SENTINEL, np.uint8)) for k in ("out", "med", "nc", "n", "lh")}
    pin, out, med, nc, pn, lh = (d_in.data_ptr(),) + tuple(outs[k].data_ptr() for k in ("out", "med", "nc", "n", "lh"))
    d_dark = ic.to_dev(torch, np.zeros((2, h), np.float32))
    d_maps = ic.device_maps(capi, torch, [Map(MAP_SCALE, 1, 0.0, 0.5, 0.0)] * 2)
    dk, mp = d_dark.data_ptr(), d_maps.data_ptr()
    nan = float("nan")

    def refused(rc, want_rc, fragment):
        assert rc == want_rc, (rc, want_rc, fragment)
        msg = L.ouster_hip_last_error().decode()
        assert fragment in msg, (fragment, msg)

    A, D, P = L.ouster_hip_image_apply, L.ouster_hip_image_dark_rows, L.ouster_hip_image_percentiles
    # ouster_hip_image_apply(ctx, planes, in_type, out, out_type, n, h, w, in_stride, out_stride, dark, maps)
    refused(A(None, pin, F32, out, F32, 1, h, w, 0, 0, dk, mp), INV, "ctx is NULL")
    refused(A(ctx.h, pin, F32, out, U8, 1, h, w, 0, 0, dk, mp), INV, "out_type must be F32 or F64")
    refused(A(ctx.h, pin, F32, out, F16, 1, h, w, 0, 0, dk, mp), INV, "out_type must be F32 or F64")
    refused(A(ctx.h, pin, F64, out, F32, 1, h, w, 0, 0, dk, mp), INV, "in_type must be")
    refused(A(ctx.h, pin, F32, out, F64, 1, h, w, 0, 0, dk, mp), INV, "in_type must be")
    refused(A(ctx.h, pin, U64, out, F32, 1, h, w, 0, 0, dk, mp), INV, "in_type must be")
    refused(A(ctx.h, pin, F16, out, F64, 1, h, w, 0, 0, dk, mp), INV, "in_type must be")
    refused(A(ctx.h, pin, F32, out, F32, 65536, 1, 1, 0, 0, dk, mp), INV, "at most 65535 images")
    refused(A(ctx.h, pin, F32, out, F32, 1, 65536, 32769, 0, 0, dk, mp), INV, "larger than 2^31")
    refused(A(ctx.h, None, F32, out, F32, 1, h, w, 0, 0, dk, mp), INV, "NULL image pointer")
    refused(A(ctx.h, pin, F32, out, F32, 2, h, w, h * w - 1, 0, dk, mp), INV, "image_stride smaller than an image")
    refused(A(ctx.h, pin, F32, None, F32, 1, h, w, 0, 0, dk, mp), INV, "out is NULL")
    refused(A(ctx.h, pin, F32, out, F32, 2, h, w, 0, h * w - 1, dk, mp), INV, "out_stride smaller than an image")
    refused(A(ctx.h, pin, U16, pin, F32, 1, h, w, 0, 0, dk, mp), INV, "in place needs equal types and strides")
    refused(A(ctx.h, pin, F32, pin, F32, 2, h, w, h * w, h * w + 4, dk, mp), INV, "in place needs equal types and strides")
    # ouster_hip_image_dark_rows(ctx, planes, in_type, out_type, n, h, w, stride, medians, n_cols)
    refused(D(None, pin, F32, F32, 1, h, w, 0, med, nc), INV, "ctx is NULL")
    refused(D(ctx.h, pin, F32, U16, 1, h, w, 0, med, nc), INV, "out_type must be F32 or F64")
    refused(D(ctx.h, pin, F16, F32, 1, h, w, 0, med, nc), INV, "in_type must be")
    refused(D(ctx.h, pin, F64, F32, 1, h, w, 0, med, nc), INV, "in_type must be")
    refused(D(ctx.h, pin, F32, F32, 65536, 2, 1, 0, med, nc), INV, "at most 65535 images")
    refused(D(ctx.h, None, F32, F32, 1, h, w, 0, med, nc), INV, "NULL image pointer")
    refused(D(ctx.h, pin, F32, F32, 2, h, w, h * w - 1, med, nc), INV, "image_stride smaller than an image")
    refused(D(ctx.h, pin, F32, F32, 1, 1, w, 0, med, nc), INV, "at least two rows")
    refused(D(ctx.h, pin, F32, F32, 1, 2, 4097, 0, med, nc), UNS, "wider than 4096 columns")
    refused(D(ctx.h, pin, F32, F32, 1, h, w, 0, None, nc), INV, "medians is NULL")
    # ouster_hip_image_percentiles(ctx, planes, in_type, out_type, n, h, w, stride, dark, lo, hi, n, lo_hi)
    refused(P(None, pin, F32, F32, 1, h, w, 0, dk, 0.1, 0.1, pn, lh), INV, "ctx is NULL")
    refused(P(ctx.h, pin, F16, F32, 1, h, w, 0, dk, 0.1, 0.1, pn, lh), INV, "in_type must be")
    refused(P(ctx.h, None, F32, F32, 1, h, w, 0, dk, 0.1, 0.1, pn, lh), INV, "NULL image pointer")
    refused(P(ctx.h, pin, F32, F32, 1, h, w, 0, dk, 0.1, 0.1, None, lh), INV, "NULL output pointer")
    refused(P(ctx.h, pin, F32, F32, 1, h, w, 0, dk, 0.1, 0.1, pn, None), INV, "NULL output pointer")
    for lo, hi in ((-0.1, 0.1), (0.1, -0.1), (nan, 0.1), (0.1, nan), (0.5, 0.5), (1.0, 0.0), (0.0, 1.5)):
        refused(P(ctx.h, pin, F32, F32, 1, h, w, 0, dk, lo, hi, pn, lh), INV, "percentiles must be >= 0 and sum to less than 1")
    # nothing to do: OK, and nothing is written
    for n_, h_, w_ in ((0, h, w), (1, 0, w), (1, h, 0)):
        assert A(ctx.h, pin, F32, out, F32, n_, h_, w_, 0, 0, dk, mp) == capi.OK
        assert D(ctx.h, pin, F32, F32, n_, h_, w_, 0, med, nc) == capi.OK
        assert P(ctx.h, pin, F32, F32, n_, h_, w_, 0, dk, 0.1, 0.1, pn, lh) == capi.OK
    # the _host forms: host outputs
    img = np.ones((h, w), np.float32)
    keep = img.copy()
    wide = np.ones((2, 4097), np.float32)
    h_med, h_nc = ic.sentinel_of(np.float32, 16), ic.sentinel_of(np.uint32, 2)
    h_n, h_lh = ic.sentinel_of(np.uint32, 2), ic.sentinel_of(np.float32, 4)
    ip, mdp, ncp, np_, lhp = (a.ctypes.data for a in (img, h_med, h_nc, h_n, h_lh))
    DH, PH, AH = L.ouster_hip_image_dark_rows_host, L.ouster_hip_image_percentiles_host, L.ouster_hip_image_apply_host
    refused(DH(None, ip, F32, h, w, mdp, ncp), INV, "ctx is NULL")
    refused(DH(ctx.h, ip, U16, h, w, mdp, ncp), INV, "dtype must be F32 or F64")
    refused(DH(ctx.h, ip, F32, 1, w, mdp, ncp), INV, "at least two rows")
    refused(DH(ctx.h, ip, F32, h, 0, mdp, ncp), INV, "at least two rows")
    refused(DH(ctx.h, None, F32, h, w, mdp, ncp), INV, "NULL pointer")
    refused(DH(ctx.h, ip, F32, h, w, None, ncp), INV, "NULL pointer")
    refused(DH(ctx.h, ip, F32, h, w, mdp, None), INV, "NULL pointer")
    refused(DH(ctx.h, wide.ctypes.data, F32, 2, 4097, mdp, ncp), UNS, "wider than 4096 columns")
    refused(PH(None, ip, F32, h, w, None, 0.1, 0.1, np_, lhp), INV, "ctx is NULL")
    refused(PH(ctx.h, ip, U8, h, w, None, 0.1, 0.1, np_, lhp), INV, "dtype must be F32 or F64")
    refused(PH(ctx.h, None, F32, h, w, None, 0.1, 0.1, np_, lhp), INV, "bad image arguments")
    refused(PH(ctx.h, ip, F32, h, w, None, 0.1, 0.1, None, lhp), INV, "bad image arguments")
    refused(PH(ctx.h, ip, F32, h, w, None, 0.1, 0.1, np_, None), INV, "bad image arguments")
    refused(PH(ctx.h, ip, F32, 0, w, None, 0.1, 0.1, np_, lhp), INV, "bad image arguments")
    refused(PH(ctx.h, ip, F32, h, w, None, 0.6, 0.4, np_, lhp), INV, "percentiles must be")
    refused(AH(None, ip, F32, h, w, None, None), INV, "ctx is NULL")
    refused(AH(ctx.h, ip, F16, h, w, None, None), INV, "dtype must be F32 or F64")
    refused(AH(ctx.h, None, F32, h, w, None, None), INV, "NULL image pointer")
    assert AH(ctx.h, ip, F32, 0, w, None, None) == capi.OK and AH(ctx.h, ip, F32, h, 0, None, None) == capi.OK
    ctx.sync()
    for k, t in outs.items():
        assert (t.cpu().numpy() == ic.SENTINEL).all(), k
    assert np.array_equal(d_in.cpu().numpy().view(np.float32), np.ones(2 * h * (w + 1), np.float32))
    assert same_bits(img, keep)
    for a in (h_med, h_nc, h_n, h_lh):
        assert (a.view(np.uint8) == ic.SENTINEL).all()
