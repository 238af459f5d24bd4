"""Display images on the GPU against the plain-numpy model of tests/image_model.py (never against the product itself).
Order statistics are compared bit for bit: an order statistic of exactly rounded values has one correct answer; the images
and the carried state likewise, because every step is one IEEE operation in a fixed order on both sides."""
import ctypes as C

import numpy as np
import pytest

from conftest import has_gpu
from image_model import AutoExposureModel, BeamUniformityModel, dark_row_medians, kth

pytestmark = pytest.mark.gpu

NP = {"u8": np.uint8, "u16": np.uint16, "u32": np.uint32, "f32": np.float32, "f64": np.float64}


def _tag(capi, name):
    return {"u8": capi.U8, "u16": capi.U16, "u32": capi.U32, "f32": capi.F32, "f64": capi.F64}[name]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


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


def make_images(rng, in_name, h, w):
    """One batch with every kind of image the order statistics have to get right."""
    dt = NP[in_name]
    integer = np.issubdtype(dt, np.integer)
    top = {"u8": 255, "u16": 65535, "u32": 2 ** 32 - 1}.get(in_name, 0)
    imgs = {}
    x = rng.normal(100, 10, (h, w))
    imgs["normal"] = np.clip(np.rint(x), 0, top) if integer else x
    imgs["ties"] = rng.integers(0, 4, (h, w)).astype(np.float64)                       # heavy ties (8-bit-like data)
    ramp = np.linspace(5000 if in_name != "u8" else 240, 10, h)[:, None] + rng.integers(0, 7, (h, w))
    imgs["negative_diffs"] = ramp                                                        # rows get darker downwards
    if in_name == "u32":
        imgs["wide"] = rng.integers(0, 2 ** 32 - 1, (h, w)).astype(np.float64)          # needs rounding on the way to f32
    elif not integer:
        imgs["wide"] = rng.normal(0, 1, (h, w)) * 10.0 ** rng.integers(-6, 6, (h, w))   # negative pixels, many exponents
    imgs["no_columns"] = np.zeros((h, w))                                                # n_cols = 0
    one = np.zeros((h, w))
    one[:, w // 3] = rng.integers(1, 200, h)
    imgs["one_column"] = one                                                             # n_cols = 1
    win = imgs["normal"].copy()
    win[:, : w // 2 + 1] = 0
    imgs["window"] = win                                                                 # an azimuth window
    few = np.zeros((h, w))
    idx = rng.choice(h * w // 4, size=min(60, h * w // 8), replace=False) * 4
    few.reshape(-1)[idx] = rng.integers(1, 200, idx.size)
    imgs["few_positive"] = few                                                           # fewer than 100 positive samples
    names = list(imgs)
    return names, np.stack([imgs[n] for n in names]).astype(dt)


@pytest.mark.parametrize("h,w", [(128, 2048), (32, 1024), (7, 130), (3, 4096)])
@pytest.mark.parametrize("in_name,out_name", [("f32", "f32"), ("f64", "f64"), ("u8", "f32"), ("u16", "f32"), ("u32", "f32"),
                                              ("u8", "f64"), ("u16", "f64"), ("u32", "f64")])
def test_order_statistics_bit_exact(gpu, h, w, in_name, out_name):
    capi, ctx, torch = gpu
    L = ctx.L
    rng = np.random.default_rng(h * 7 + w)
    names, batch = make_images(rng, in_name, h, w)
    T = NP[out_name]
    n = len(names)
    d_in = to_dev(torch, batch)
    es = np.dtype(T).itemsize
    d_med = torch.zeros(n * (h - 1) * es, dtype=torch.uint8, device="cuda")
    d_nc = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
    capi.check(L.ouster_hip_image_dark_rows(ctx.h, d_in.data_ptr(), _tag(capi, in_name), _tag(capi, out_name), n, h, w, 0,
                                            d_med.data_ptr(), d_nc.data_ptr()))
    # dark counts for the percentile kernel: none for the first pass, then rows dark enough to zero part of the sample
    dark = np.zeros((n, h), T)
    dark[:, ::2] = T(95)
    dark[:, 1::4] = T(1e9)
    d_dark = to_dev(torch, dark)
    res = []
    for dk in (None, d_dark):
        d_n = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
        d_lh = torch.zeros(n * 2 * es, dtype=torch.uint8, device="cuda")
        capi.check(L.ouster_hip_image_percentiles(ctx.h, d_in.data_ptr(), _tag(capi, in_name), _tag(capi, out_name), n, h, w, 0,
                                                  dk.data_ptr() if dk is not None else None, 0.1, 0.25, d_n.data_ptr(),
                                                  d_lh.data_ptr()))
        res.append((d_n, d_lh))
    ctx.sync()
    med = from_dev(d_med, T, (n, h - 1))
    n_cols = from_dev(d_nc, np.uint32, (n,))
    seen_small = seen_zeroed = False
    for i, name in enumerate(names):
        img = batch[i].astype(T)
        want_med, want_nc = dark_row_medians(img)
        assert n_cols[i] == want_nc, (name, n_cols[i], want_nc)
        assert same_bits(med[i], want_med), (name, med[i][:8], want_med[:8])
        for (d_n, d_lh), dk in zip(res, (None, dark[i])):
            x = img
            if dk is not None:
                x = img - dk[:, None]
                x = np.where(x < 0, T(0), x)
                seen_zeroed |= bool((x.reshape(-1)[::4] == 0).any() and (img.reshape(-1)[::4] > 0).any())
            s = x.reshape(-1)[::4]
            kept = s[s > 0]
            got_n = from_dev(d_n, np.uint32, (n,))[i]
            got = from_dev(d_lh, T, (n, 2))[i]
            assert got_n == kept.size, (name, got_n, kept.size)
            seen_small |= 0 < kept.size < 100
            if kept.size:
                want = np.array([kth(kept, int(kept.size * 0.1)), kth(kept, kept.size - int(kept.size * 0.25) - 1)], T)
            else:
                want = np.zeros(2, T)
            assert same_bits(got, want), (name, dk is not None, got, want)
    assert 0 in n_cols and 1 in n_cols and seen_small and seen_zeroed


def sequence(dtype, h=32, w=256, seed=7):
    """20 images with a fixed seed and the update_state flag of every call."""
    rng = np.random.default_rng(seed)
    flags = [1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 0, 1, 1, 0, 1, 1]
    out = []
    for i in range(20):
        if i == 0:
            img = np.full((h, w), 100.0)                                   # constant: the inf branch
        elif i == 6:
            img = np.zeros((h, w))                                         # fewer than 100 positive samples
            img[3, 8:200:4] = rng.uniform(1, 50, 48)
        elif 7 <= i <= 13 or i in (17, 18):
            img = rng.normal(400, 5, (h, w))                               # 30 % of the positive values below 1
            low = rng.random((h, w)) < 0.3
            img[low] = rng.uniform(0.01, 0.9, int(low.sum()))
        elif i == 14:
            img = rng.normal(100, 10, (h + 16, w)) + np.arange(h + 16)[:, None] * 0.5   # a change of h
        else:
            img = rng.normal(100, 10, (h, w)) + rng.normal(0, 3, (h, 1))   # per-row offsets for the corrector
        out.append((img.astype(dtype), bool(flags[i])))
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_twenty_updates_match_the_model_bit_for_bit(gpu, dtype):
    """The Python classes (thin bindings of the C++ mirror): buc.update(img); ae.update(img) on one image, and two more
    AutoExposure objects on copies, after every call compared with the model: image, lo_state, hi_state, dark_count."""
    from ouster_sdk_amd import core
    buc, m_buc = core.BeamUniformityCorrector(), BeamUniformityModel()
    aes = [(core.AutoExposure(), AutoExposureModel()),
           (core.AutoExposure(0.1, 0.1, 1, 0.5), AutoExposureModel(0.1, 0.1, 1, 0.5)),
           (core.AutoExposure(4), AutoExposureModel(update_every=4))]
    chained, m_chained = core.AutoExposure(0.1, 0.1, 1, 0.5), AutoExposureModel(0.1, 0.1, 1, 0.5)
    early_on_initialised = False
    for i, (img, flag) in enumerate(sequence(dtype)):
        for ae, m in aes:
            a, b = img.copy(), img.copy()
            was_init = m.initialized
            ae.update(a, flag)
            m.update(b, flag)
            assert same_bits(a, b), (i, m.branches[-1], np.abs(a - b).max())
            assert (ae.lo_state, ae.hi_state) == (m.lo_state, m.hi_state), i
            early_on_initialised |= m.branches[-1] == "early" and was_init
        a, b = img.copy(), img.copy()
        buc.update(a, flag)
        m_buc.update(b, flag)
        assert same_bits(a, b), (i, np.abs(a - b).max())
        assert np.array_equal(buc.dark_count, m_buc.dark_count), i
        chained.update(a, flag)
        m_chained.update(b, flag)
        assert same_bits(a, b), (i, m_chained.branches[-1])
        assert (chained.lo_state, chained.hi_state) == (m_chained.lo_state, m_chained.hi_state), i
        assert a.min() >= 0 and (a.max() <= 1 or m_chained.branches[-1] in ("early", "uninit"))
    fast = aes[1][1]
    assert {"inf", "affine", "hi", "early"} <= set(fast.branches), fast.branches
    assert early_on_initialised
    assert m_buc.dark_count.size == 32 and any(img.shape[0] == 48 for img, _ in sequence(dtype))


def pool_image(capi, shape, dtype):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = capi.load_hip().ouster_hip_host_alloc(n, 1)
    assert p and capi.load_hip().ouster_hip_host_is_pinned(p, n) == 1
    return p, np.ctypeslib.as_array((C.c_uint8 * n).from_address(p)).view(dtype).reshape(shape)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_containers_in_place_and_no_steady_state_allocations(gpu, dtype):
    capi, _, _ = gpu
    from ouster_sdk_amd import core
    rng = np.random.default_rng(3)
    src = (rng.normal(100, 10, (64, 1024)) + rng.normal(0, 3, (64, 1))).astype(dtype)
    p, pooled = pool_image(capi, src.shape, dtype)
    try:
        foreign = np.empty_like(src)
        objs = [(core.BeamUniformityCorrector(), core.AutoExposure()) for _ in range(2)]
        m_buc, m_ae = BeamUniformityModel(), AutoExposureModel()
        for k in range(3):
            pooled[:] = src + k
            foreign[:] = src + k
            want = (src + dtype(k)).copy()
            for (buc, ae), img in zip(objs, (pooled, foreign)):
                buc.update(img)
                ae.update(img)
            m_buc.update(want)
            m_ae.update(want)
            assert same_bits(np.array(pooled), want) and same_bits(foreign, want), k
        before = capi.alloc_stats()
        for k in range(100):
            pooled[:] = src
            foreign[:] = src
            for (buc, ae), img in zip(objs, (pooled, foreign)):
                buc.update(img)
                ae.update(img)
        after = capi.alloc_stats()
        assert after["device_allocs"] == before["device_allocs"] and after["pinned_allocs"] == before["pinned_allocs"]
        assert same_bits(np.array(pooled), foreign)
    finally:
        capi.load_hip().ouster_hip_host_free(p)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_update_batch_equals_single_updates(gpu, dtype):
    """update_batch over 24 images (one launch per kernel) == 24 update() calls on a second object, and == the model; the
    corrector handing its dark counts to an AutoExposure == buc.update(img); ae.update(img) per image; uint16 planes are
    converted on load like astype()."""
    from ouster_sdk_amd import core
    rng = np.random.default_rng(11)
    stack = (rng.normal(100, 10, (24, 32, 256)) + rng.normal(0, 3, (24, 32, 1))).astype(dtype)
    stack[6] = 0
    stack[6, 2, 0:160:4] = 7                            # call 6 samples again (update_every = 3): an early return mid-batch
    f64 = dtype == np.float64
    ae_b, ae_s, m_ae = core.AutoExposure(), core.AutoExposure(), AutoExposureModel()
    got = ae_b.update_batch(stack, float64=f64)
    assert got.dtype == dtype
    for i in range(24):
        a, b = stack[i].copy(), stack[i].copy()
        ae_s.update(a)
        m_ae.update(b)
        assert same_bits(a, b) and same_bits(np.ascontiguousarray(got[i]), b), (i, m_ae.branches[-1])
    assert "early" in m_ae.branches and (ae_b.lo_state, ae_b.hi_state) == (ae_s.lo_state, ae_s.hi_state) == (m_ae.lo_state, m_ae.hi_state)
    # the pair in one pass over the pixels, from uint16 planes
    planes = np.clip(np.rint(stack * 20), 0, 65535).astype(np.uint16)
    buc, ae, m_buc, m_ae = core.BeamUniformityCorrector(), core.AutoExposure(), BeamUniformityModel(), AutoExposureModel()
    for flag in (True, False, True):
        got = buc.update_batch(planes, float64=f64, update_state=flag, then=ae)
        for i in range(24):
            b = planes[i].astype(dtype)
            m_buc.update(b, flag)
            m_ae.update(b, flag)
            assert same_bits(np.ascontiguousarray(got[i]), b), (flag, i, m_ae.branches[-1])
        assert np.array_equal(buc.dark_count, m_buc.dark_count)
        assert (ae.lo_state, ae.hi_state) == (m_ae.lo_state, m_ae.hi_state)
    alone = core.BeamUniformityCorrector().update_batch(planes[:3], float64=f64)
    m = BeamUniformityModel()
    for i in range(3):
        b = planes[i].astype(dtype)
        m.update(b)
        assert same_bits(np.ascontiguousarray(alone[i]), b), i


def _run(args):
    """tests/cpp/image_batch_tool.cpp, built by tests/cpp/Makefile -> what it printed"""
    import cpp_tools
    return cpp_tools.run("image_batch_tool", args).stdout


def test_render_images_two_sensors_equals_model_per_sensor(gpu, oracle, tmp_path):
    """DeviceFrameBatch::render_images("NEAR_IR") on 16 decoded synthetic frames of two interleaved sensors == the model run per
    sensor (frame f -> sensor f % 2, a sensor's frames in index order) on the ORACLE's destaggered planes, bit for bit; a second
    call with update_state = false likewise; the per-sensor state too."""
    O = oracle
    h, w, n, S = 128, 1024, 16, 2
    cal = O.synthetic_calib(h=h, w=w, profile="RNG15_RFL8_NIR8_DUAL")
    pf = cal.packet_format()
    packets, _ = O.synth_packets(cal, n)
    src = tmp_path / "packets.bin"
    np.ascontiguousarray(packets).tofile(src)
    out = _run(["render", src, h, w, n, S, tmp_path / "r"])
    elem = int(out.split("elem")[1].split()[0])
    planes = np.fromfile(tmp_path / "r.planes", {1: np.uint8, 2: np.uint16, 4: np.uint32}[elem]).reshape(n, h, w)
    want_planes = []
    for f in range(n):
        fr = O.Frame.for_profile(cal.profile, cal.h, cal.w, cal.cpp, with_window=True)
        O.batch_frame(pf, packets[f], fr, init_id=cal.init_id & 0xFFFFFF)
        want_planes.append(O.destagger(fr.plane("NEAR_IR"), cal.pixel_shift_by_row))
        assert np.array_equal(planes[f], want_planes[f]), f
    bucs = [BeamUniformityModel() for _ in range(S)]
    aes = [AutoExposureModel() for _ in range(S)]
    for k, flag in enumerate((True, False)):
        got = np.fromfile(tmp_path / ("r.images%d" % k), np.float32).reshape(n, h, w)
        for f in range(n):
            img = want_planes[f].astype(np.float32)
            bucs[f % S].update(img, flag)
            aes[f % S].update(img, flag)
            assert same_bits(np.ascontiguousarray(got[f]), img), (k, f, aes[f % S].branches[-1])
            assert img.min() >= 0 and img.max() <= 1
    st = np.fromfile(tmp_path / "r.state", np.float64).reshape(S, 2 + h)
    for s in range(S):
        assert (st[s, 0], st[s, 1]) == (aes[s].lo_state, aes[s].hi_state) and np.array_equal(st[s, 2:], bucs[s].dark_count), s
    assert aes[0].lo_state != aes[1].lo_state          # the two sensors really kept their own state


def test_render_images_on_a_plane_that_was_not_requested_throws(gpu):
    assert _run(["refuse", "32", "512"]).startswith("invalid_argument")


def test_cpp_update_on_a_std_vector_equals_pool_memory(gpu):
    """The C++ classes themselves, ten calls: a std::vector-backed ImgRef (foreign memory, staged) gives the bits and the state
    of the same calls on an img_t (pool memory, in place)."""
    assert _run(["cpp_update"]).strip() == "same"
