"""tests/tonemap_model.py pinned by hand: the yardstick of the RGB display-image tests has to be right on its own.  Bit patterns
of the float16 front end and of fast_log10, a table computed by hand, the extrapolating blend, uneven tiles, the properties a
tone mapper must have, and the branches the sequences of the GPU tests reach."""
import numpy as np
import pytest

import tonemap_cases as K
import tonemap_model as M

f32 = np.float32


def u32(x):
    return int(np.array(x, np.float32).view(np.uint32))


def test_f16_front_end_bit_patterns():
    got = M.f16_bits_to_f32(np.array([0x3C00, 0x0000, 0x7e00, 0x0001, 0x7C00, 0xBC00, 0x3800, 0x4200], np.uint16)).view(np.uint32)
    assert got[0] == 0x3F800000 and got[1] == 0 and got[2] == 0          # 1.0, and both ways a pixel is dropped
    assert got[3] == (0x0001 + 0x1C000) << 13 == 0x38002000              # a subnormal: not 2^-24, what the formula gives
    assert got[4] == (0x7C00 + 0x1C000) << 13 == 0x47800000              # infinity: 65536.0
    assert got[5] == (0xBC00 + 0x1C000) << 13 == 0x4F800000              # -1.0: the sign bit lands in the exponent
    assert M.f16_bits_to_f32(np.array([0x3800, 0x4200], np.uint16)).tolist() == [0.5, 3.0]
    every = M.f16_bits_to_f32(np.arange(65536, dtype=np.uint16))
    assert np.isfinite(every).all() and (every >= 0).all()
    normal = np.arange(0x0400, 0x7C00, dtype=np.uint16)                  # on normal halves the formula IS the conversion
    assert np.array_equal(M.f16_bits_to_f32(normal), normal.view(np.float16).astype(np.float32))


def test_fast_log10_bit_patterns():
    got = M.fast_log10(np.array([1.0, 2.0, 10.0], np.float32))
    assert u32(got[0]) == 0                                               # bits(1.0) - 0x3F800000 = 0
    two = f32(f32(1 << 23) * f32(1.1920929e-7)) * f32(0.30103)            # one exponent step = 2^23 counts
    assert u32(got[1]) == u32(two) and abs(float(got[1]) - 0.30103) < 1e-7
    ten = f32(f32(0x41200000 - 0x3F800000) * f32(1.1920929e-7)) * f32(0.30103)
    assert u32(got[2]) == u32(ten) and abs(float(got[2]) - 0.97835) < 1e-5   # the linear mantissa: 3.25 * 0.30103, not 1.0


def test_luminance_order_and_constants():
    px = np.array([[0.3, 0.6, 0.9]], np.float32)
    want = f32(f32(px[0, 0] * f32(0.299)) + f32(px[0, 1] * f32(0.587))) + f32(px[0, 2] * f32(0.114))
    assert u32(M.luminance(px)[0]) == u32(want)
    px = np.array([[0.3, 0.6, 0.9]], np.float64)
    assert M.luminance(px)[0] == (0.3 * 0.299 + 0.6 * 0.587) + 0.9 * 0.114


def test_sample_is_every_fourth_pixel_and_the_indices():
    img = np.zeros((8, 50, 3), np.float32)
    img.reshape(-1, 3)[::4] = np.arange(1, 101, dtype=np.float32)[:, None]      # exactly 100 samples, luminance ~ 1 .. 100
    img.reshape(-1, 3)[1::4] = 1e6                                               # pixels 1, 5, ...: never looked at
    n, lo, hi = M.lum_stats(img, 0.1, 0.2)
    lum = M.luminance(img.reshape(-1, 3)[::4])
    assert n == 100 and lo == np.sort(lum)[10] and hi == np.sort(lum)[100 - 20 - 1]
    img.reshape(-1, 3)[0] = [1.0, 1.0, -10.0]                                    # a channel below zero: lum <= 0, dropped
    assert M.lum_stats(img, 0.1, 0.2)[0] == 99


def test_one_pixel_tiles_table_by_hand():
    """8 x 8: a tile holds one pixel.  clip = 1/1024, the occupied bin loses 1 - 1/1024, every bin gains that / 1024."""
    lum = np.full((8, 8), 0.5, np.float32)
    lum[3, 5] = 0.25
    luts = M.clahe_luts(lum)
    clip = f32(1) / f32(1024)
    excess = f32(1) - clip
    red = excess / f32(1024)
    for tile, b in ((0, 512), (3 * 8 + 5, 256)):
        lut = luts[tile]
        cdf = f32(0)
        for i in range(1024):
            cdf = f32(cdf + (f32(clip + red) if i == b else f32(f32(0) + red)))
            assert u32(lut[i]) == u32(min(f32(cdf * f32(1)), f32(1))), (tile, i)
        assert float(lut[b - 1]) == pytest.approx(b * float(red), rel=1e-5)            # before the occupied bin: a slow ramp
        assert float(lut[b]) - float(lut[b - 1]) == pytest.approx(float(clip + red), rel=1e-4)
        assert 0.999 < float(lut[1023]) <= 1.0


def test_extrapolation_in_the_first_half_tile():
    tx0, tx1, fx = M.tile_coords(2048)
    assert tx0[0] == 0 and tx1[0] == 1 and -0.4981 < fx[0] < -0.4980
    assert fx[127] < 0 <= fx[128]
    assert tx0[2047] == 7 and tx1[2047] == 7                          # the last half tile: both tables are tile 7's
    rng = np.random.default_rng(0)
    lum = rng.random((16, 64)).astype(np.float32)
    luts = M.clahe_luts(lum)
    out = M.clahe_apply(lum, luts)
    ty0, ty1, fy = M.tile_coords(16)
    tx0, tx1, fx = M.tile_coords(64)
    assert fx[0] < 0 and fy[0] < 0
    b = min(int(f32(lum[0, 0]) * f32(1024)), 1023)
    L = luts.reshape(8, 8, 1024)
    top = f32(f32(f32(1) - fx[0]) * L[0, 0, b]) + f32(fx[0] * L[0, 1, b])
    bot = f32(f32(f32(1) - fx[0]) * L[1, 0, b]) + f32(fx[0] * L[1, 1, b])
    hand = f32(f32(f32(1) - fy[0]) * top) + f32(fy[0] * bot)
    assert u32(out[0, 0]) == u32(hand)


def test_uneven_tiles_9_by_13():
    rows = M.tile_bounds(9)
    assert rows[0] == (0, 1) and rows[7] == (7, 9) and sum(b - a for a, b in rows) == 9
    cols = M.tile_bounds(13)
    assert [b - a for a, b in cols] == [1, 2, 1, 2, 2, 1, 2, 2]
    rng = np.random.default_rng(1)
    lum = rng.random((9, 13)).astype(np.float64)
    luts = M.clahe_luts(lum)
    assert luts.shape == (64, 1024) and (np.diff(luts, axis=1) >= 0).all() and (luts <= 1).all() and (luts[:, -1] > 0.999).all()
    # a one-row tile of two pixels: two steps of clip + redistribute each
    tile = luts[0 * 8 + 1]
    b = np.sort(M.bins_of(lum[0:1, 1:3]).reshape(-1))
    if b[0] != b[1]:
        assert float(tile[b[0]]) - float(tile[b[0] - 1]) == pytest.approx(float(tile[b[1]]) - float(tile[b[1] - 1]), rel=1e-4)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_properties(dtype):
    rng = np.random.default_rng(2)
    m = M.LocalToneMapperModel()
    img = K.scene(rng, 32, 64, 0.7, dtype)
    img[5, 7] = 0                                                       # a black pixel
    out = img.copy()
    m.update(out)
    assert out.dtype == dtype and out.min() >= 0 and out.max() <= 1 and not np.isnan(out).any()
    assert (out[5, 7] == 0).all()
    state = (m.lo_state, m.hi_state, m.counter)
    again = img.copy()
    m.update(again, update_state=False)
    assert (m.lo_state, m.hi_state, m.counter) == state and m.stats[-1] is None
    # fewer than 100 positive samples: nothing changes, not even the counter
    few = np.zeros((32, 64, 3), dtype)
    few.reshape(-1, 3)[:4 * 99:4] = 0.5
    keep = few.copy()
    m.update(few)
    assert K.same_bits(few, keep) and (m.lo_state, m.hi_state, m.counter) == state and m.branches[-1] == "early"
    # a mapper that has seen a bright scene maps the same image differently
    other = M.LocalToneMapperModel()
    other.update(K.scene(rng, 32, 64, 5.0, dtype))
    b = img.copy()
    other.update(b, update_state=False)
    assert not np.array_equal(b, again)
    # an uninitialised mapper asked not to update does nothing
    fresh, c = M.LocalToneMapperModel(), img.copy()
    fresh.update(c, update_state=False)
    assert K.same_bits(c, img) and fresh.branches == ["uninit"]


def test_rgb_auto_exposure_clamps_and_converts():
    rng = np.random.default_rng(3)
    m = M.RgbAutoExposureModel()
    img = K.scene(rng, 32, 64, 0.7)
    out = img.copy()
    m.update(out)
    assert out.min() == 0 and out.max() == 1 and m.branches[0] in ("affine", "hi")
    few = np.zeros((8, 49, 3), np.uint16)
    few[...] = 0x3C00                                                   # 98 samples: the early return, the plain converted image
    got = M.RgbAutoExposureModel().update_f16(few)
    assert got.dtype == np.float32 and (got == 1.0).all()
    assert M.RgbAutoExposureModel().update_f16(np.full((8, 50, 3), 0x3C00, np.uint16)).max() <= 1.0


def test_the_gpu_sequences_reach_every_branch():
    """What tests/test_gpu_tonemap.py and tests/test_tonemap_lanes_cpu.py feed the product passes through every map, compression
    on and off, every kind of colour factor and colour correction off -- asserted on the model's own log, so that no GPU test
    can silently cover one path only."""
    seen, early = set(), False
    for name, kw, const_first in K.LTM_CONFIGS:
        for h, w in ((32, 64), (64, 1024)):
            m = M.LocalToneMapperModel(**kw)
            for img, flag in K.frames(h, w, np.float32, seed=h, const_first=const_first):
                m.update(img, flag)
            early |= "early" in m.branches
            seen |= {b for b in m.branches if isinstance(b, tuple)}
    assert early
    assert {b[0] for b in seen} == {"inf", "affine", "hi"}
    assert {b[1] for b in seen} == {True, False}
    assert {b[2] for b in seen} == {"zero", "ramp", "full", "off"}
    paths = {K.model_case(p, 9, 13, np.float32, 0)[3] for p in K.PIXEL_PATHS}
    assert {b[0] for b in paths} == {"inf", "affine", "hi"} and {b[1] for b in paths} == {True, False}
    assert {b[2] for b in paths} == {"zero", "ramp", "full", "off"}
    ae_seen = set()
    for kw, const_first in K.AE_CONFIGS:
        ae = M.RgbAutoExposureModel(**kw)
        for img, flag in K.ae_frames(32, 64, np.float32, seed=1, const_first=const_first):
            ae.update(img, flag)
        ae_seen |= set(ae.branches)
    assert {"inf", "affine", "hi", "early"} <= ae_seen


def test_params_pack_to_the_abi_layout():
    p = M.Params(M.MAP_AFFINE, 0.25, 3.0, 0.1, True, 0.5, False)
    raw = K.pack_params(p)
    assert len(raw) == 48 and len(K.pack_map(p)) == 32 and raw[:32] == K.pack_map(p)
