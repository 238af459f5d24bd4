"""tests/image_cases.py without a GPU: apply_model pinned by hand, and the precondition of every case of
test_gpu_image_kernels.py, so that no case there passes for a trivial reason."""
import numpy as np
import pytest

import image_cases as ic
from image_cases import MAP_AFFINE, MAP_NONE, MAP_SCALE, Map, same_bits

f32 = np.float32


def test_apply_model_pinned_by_hand():
    img = np.array([[4.0, 10.0, -0.0], [1.0, 30.0, 9.0]], f32)
    dark = np.array([2.0, 5.0], f32)
    # dark counts only (maps == NULL): 4-2, 10-2, -0-2 -> 0 ; 1-5 -> 0, 30-5, 9-5
    assert ic.same_bits(ic.apply_model(img, "f32", f32, dark), np.array([[2, 8, 0], [0, 25, 4]], f32))
    # NONE without dark counts: the image itself, -0.0 included
    none = ic.apply_model(img, "f32", f32, dark, Map(MAP_NONE, 0, 0.0, 1.0, 0.0))
    assert ic.same_bits(none, img) and np.signbit(none[0, 2])
    # SCALE by 1/8 after the dark counts: 25 / 8 ends above 1
    got = ic.apply_model(img, "f32", f32, dark, Map(MAP_SCALE, 1, 0.0, 0.125, 0.0))
    assert ic.same_bits(got, np.array([[0.25, 1.0, 0.0], [0.0, 1.0, 0.5]], f32))
    # SCALE without them: -0.0 * 0.125 = -0.0, and neither clamp touches it (x < 0 is false for both zeros)
    got = ic.apply_model(img, "f32", f32, dark, Map(MAP_SCALE, 0, 0.0, 0.125, 0.0))
    assert ic.same_bits(got, np.array([[0.5, 1.0, -0.0], [0.125, 1.0, 1.0]], f32)) and np.signbit(got[0, 2])
    # AFFINE (x - 3) * 0.25 + 0.5 on the raw pixels: 1 -> 0 and -0 -> -0.25 -> 0 go negative before the clamp
    got = ic.apply_model(img, "f32", f32, None, Map(MAP_AFFINE, 1, 3.0, 0.25, 0.5))
    assert ic.same_bits(got, np.array([[0.75, 1.0, 0.0], [0.0, 1.0, 1.0]], f32)) and not np.signbit(got[0, 2])
    # AFFINE with a pixel that goes negative BEFORE the map: 1 - 5 -> 0, then (0 - 3) * 0.25 + 1 = 0.25
    got = ic.apply_model(img, "f32", f32, dark, Map(MAP_AFFINE, 1, 3.0, 0.25, 1.0))
    assert got[1, 0] == f32(0.25) and got[0, 0] == f32(0.75)
    # every step is rounded in T: the float32 product differs from the double one
    a = ic.apply_model(np.array([[0.1]], f32), "f32", f32, None, Map(MAP_SCALE, 0, 0.0, 0.3, 0.0))
    assert a[0, 0] == f32(0.1) * f32(0.3) and float(a[0, 0]) != float(f32(0.1)) * 0.3


def test_apply_model_conversions():
    u = np.array([[2 ** 24 + 1, 2 ** 24 + 3, 2 ** 32 - 1]], np.uint32)
    got = ic.apply_model(u, "u32", f32)
    assert got.tolist() == [[2.0 ** 24, 2.0 ** 24 + 4, 2.0 ** 32]]       # round to nearest even
    assert ic.apply_model(u, "u32", np.float64).tolist() == [[2.0 ** 24 + 1, 2.0 ** 24 + 3, 2.0 ** 32 - 1]]
    h = ic.apply_model(np.array([[0x0001, 0x3C00, 0x7BFF, 0x8000]], np.uint16), "f16", f32)
    # the reference's integer formula, not an IEEE conversion: the sign bit is carried into the exponent (0x8000 -> 2^17)
    assert ic.bits(h).tolist() == [[0x38002000, 0x3F800000, 0x477FE000, 0x48000000]]
    assert h[0, 1] == 1.0 and h[0, 2] == 65504.0 and h[0, 3] == 131072.0
    assert ic.apply_model(np.array([[0x0000, 0x7E00]], np.uint16), "f16", f32).tolist() == [[0.0, 0.0]]
    pats = ic.f16_patterns()
    assert {int(p) >> 10 & 31 for p in pats} == set(range(32)) and {0x0000, 0x8000, 0x0001, 0x03FF, 0x7BFF} <= set(pats.tolist())


def test_medians_model_stores_plus_zero():
    img = np.array([[5.0, 5.0, 5.0], [0.0, 0.0, 0.0], [-0.0, -0.0, 7.0]], f32)
    med, n_cols = ic.medians_model(img)
    assert n_cols == 3 and med.tolist() == [-5.0, 0.0] and not np.signbit(med[1])
    assert np.signbit((img[2] - img[1])[0])          # the difference itself is -0.0


def test_launch_shape_and_grid_stride_cases():
    assert ic.launch_shape(1, 32, 256) == (2048, 8, 8192)
    assert ic.launch_shape(1024, 33, 256) == (2112, 9, 8)
    assert ic.launch_shape(65535, 1, 1) == (1, 1, 8)
    for c in ic.GRID_CASES:
        nchunk, want, cap = ic.launch_shape(c["n"], c["h"], c["w"])
        assert want > cap, c                                             # the grid-stride loop runs a second time
        assert ic.expect_vec("f32", c["n"], c["h"], c["w"]) == (c["path"] == "vector"), c
        assert c["n"] * c["h"] * c["w"] * 4 < 36 * 2 ** 20
    scalar = ic.GRID_CASES[1]
    assert scalar["h"] * scalar["w"] == 8193 and scalar["h"] * scalar["w"] % 4 == 1      # a 1-element tail
    assert ic.chunks_spanning_rows(scalar["h"], scalar["w"])[0] == 2


def test_expect_vec_restates_the_three_conditions():
    assert ic.expect_vec("f32", 3, 6, 64)
    assert not ic.expect_vec("f32", 3, 6, 64, in_off=4) and not ic.expect_vec("f32", 3, 6, 64, in_off=8)
    assert ic.expect_vec("u8", 3, 6, 64, in_off=4) and not ic.expect_vec("u8", 3, 6, 64, in_off=1)
    assert ic.expect_vec("u16", 3, 6, 64, in_off=8) and not ic.expect_vec("u16", 3, 6, 64, in_off=4)
    assert not ic.expect_vec("f32", 3, 6, 64, out_off=4) and not ic.expect_vec("f64", 3, 6, 64, out_off=8)
    assert not ic.expect_vec("f32", 3, 6, 64, in_stride=385) and not ic.expect_vec("f32", 3, 6, 64, out_stride=385)
    assert ic.expect_vec("f32", 1, 5, 3) and not ic.expect_vec("f32", 3, 5, 3) and ic.expect_vec("f32", 3, 5, 3, 16, 16)


def test_stride_cases_take_the_path_they_name():
    n, h, w = ic.STRIDE_SHAPE
    hw = h * w
    seen = set()
    for in_name, si, so, ioff, ooff, path in ic.STRIDE_CASES:
        es = np.dtype(ic.NP[in_name]).itemsize
        vec = ic.expect_vec(in_name, n, h, w, hw + si, hw + so, ioff * es, ooff * 4)
        assert vec == (path == "vector"), (in_name, si, so, ioff, ooff)
        seen.add((si, so))
    assert {(a, b) for a in (0, 1, 4) for b in (0, 1, 4)} <= seen
    assert {("f32", 1), ("u8", 1), ("u16", 1)} <= {(c[0], c[3]) for c in ic.STRIDE_CASES}
    assert any(c[4] == 1 for c in ic.STRIDE_CASES)


def test_ragged_apply_shapes_walk_rows():
    for h, w in ic.APPLY_RAGGED:
        count, most = ic.chunks_spanning_rows(h, w)
        if w % 4:
            assert count >= 1, (h, w)
        if w == 1:
            assert most == 4
        if w in (2, 3):
            assert most >= 2
        assert ic.expect_vec("f32", 1, h, w)                                  # one aligned image: the vector path
        assert ic.expect_vec("f32", 3, h, w) == (h * w % 4 == 0)              # three dense ones: only where hw % 4 == 0
    assert any(h * w % 4 in (1, 2, 3) for h, w in ic.APPLY_RAGGED)            # a tail chunk
    assert {w for _, w in ic.APPLY_RAGGED} >= {1, 2, 3}
    assert ic.chunks_spanning_rows(5, 3)[1] == 2 and ic.chunks_spanning_rows(9, 1) == (2, 4)
    # the special values survive the ragged shapes
    img = ic.apply_images(np.random.default_rng(0), 3, 33, 131, f32)
    assert np.isnan(img).sum() == 3 and np.isinf(img).sum() == 6 and (img < 0).any()
    assert (np.signbit(img) & (img == 0)).sum() >= 3
    d = ic.apply_dark(np.random.default_rng(0), 3, 33, f32)
    x = ic.apply_model(img[0], "f32", f32, d[0])
    assert (x[1] == 0).all() and (x[0] > 0).any()                           # a zeroed row and a live one
    got = ic.apply_model(img[0], "f32", f32, d[0], ic.THREE_MAPS[2])
    assert (got == 1).any() and (got == 0).any() and ((got > 0) & (got < 1)).any()
    assert [m.mode for m in ic.THREE_MAPS] == [MAP_NONE, MAP_SCALE, MAP_AFFINE] and [m.use_dark for m in ic.THREE_MAPS] == [1, 0, 1]


@pytest.mark.parametrize("h,w", ic.DARK_SHAPES)
def test_dark_cases_state_their_masks_and_parities(h, w):
    for in_name, out_name in ic.DARK_TYPES:
        names, imgs, n_cols = ic.dark_images(h, w, in_name)
        T = ic.NP[out_name]
        assert np.isfinite(imgs.astype(np.float64)).all()
        for name, img, nc in zip(names, imgs, n_cols):
            mask = (img != 0).any(axis=0)
            med, got_nc = ic.medians_model(img.astype(T))
            assert got_nc == nc == int(mask.sum()), (name, nc)
            if name in ic.WORD_EDGE_MASKS:
                assert np.flatnonzero(mask).tolist() == ic.edge_columns(name, w)
            if name == "distinct_even":
                d = np.sort(img[1:, mask].astype(T) - img[:-1, mask].astype(T), axis=1)
                assert nc % 2 == 0 and nc >= 2 and (d[:, nc // 2] != d[:, (nc - 1) // 2]).all()
                assert same_bits(med, d[:, nc // 2])
            if name == "neg_zero":
                d = img[2].astype(T) - img[1].astype(T)
                assert np.signbit(d[mask]).sum() * 2 > nc and med[1] == 0 and not np.signbit(med[1])
        assert ("distinct_even" in names) == (w > 1)
        if w > 1:
            assert {n_cols[names.index("all_columns")] % 2, n_cols[names.index("all_but_first")] % 2} == {0, 1}
        diffs = imgs[0, 1:].astype(np.float64) - imgs[0, :-1].astype(np.float64)
        if w >= 63:
            assert (diffs == 0).mean() > 0.2 and (diffs > 0).any() and (diffs < 0).any()      # ties at zero, both signs
        assert ("neg_zero" in names) == (in_name != "u16" and h >= 3)
        if w > 64:
            assert set(ic.WORD_EDGE_MASKS) <= set(names)
    if w % 4:
        assert ic.chunks_spanning_rows(h, w)[0] >= 1


def test_dark_shapes_cover_the_edges():
    ws = {w for _, w in ic.DARK_SHAPES}
    assert {1, 63, 64, 65, 255, 256, 257, 4095, 4096} <= ws and any(h == 2 for h, _ in ic.DARK_SHAPES)
    parities = set()
    for h, w in ic.DARK_SHAPES:
        parities |= {n % 2 for n in ic.dark_images(h, w, "f32")[2] if n}
    assert parities == {0, 1}


@pytest.mark.parametrize("case", ic.PCT_NAMED, ids=lambda c: c.name)
def test_percentile_cases_are_what_they_say(case):
    types = [t for t in ic.PCT_TYPES if ic.pct_image(case.fill, *case.shape, t[0]) is not None]
    assert ("f32", "f32") in types and ("f64", "f64") in types
    for in_name, out_name in types:
        n, k_lo, k_hi, kept = ic.pct_named_ranks(case, in_name, out_name)
        assert n >= 1 and 0 <= k_lo < n and 0 <= k_hi < n, (n, k_lo, k_hi)
        srt = np.sort(kept)
        K = np.uint32 if out_name == "f32" else np.uint64
        keys = np.unique(srt.view(K))
        top = 8 * np.dtype(K).itemsize - 8
        if case.fact == "same":
            assert k_lo == k_hi
        elif case.fact == "last_digit":
            assert keys.size == 2 and keys[0] >> K(8) == keys[1] >> K(8) and keys[0] != keys[1]
            assert srt[k_lo] != srt[k_hi]
        elif case.fact == "first_digit":
            assert keys.size == 2 and keys[0] >> K(top) != keys[1] >> K(top) and srt[k_lo] != srt[k_hi]
            if in_name == "f32":
                assert srt[0] == f32(2.0 ** -127) and 0 < srt[0] < np.finfo(f32).tiny and np.isinf(srt[-1])
        elif case.fact == "one_key":
            assert keys.size == 1 and k_lo != k_hi
        elif case.fact == "lo_is_min":
            assert k_lo == 0 and 0 < k_hi < n - 1
        elif case.fact == "hi_is_max":
            assert k_hi == n - 1 and 0 < k_lo < n - 1
        else:
            h, w = case.shape
            assert n == case.fact == -(-(h * w) // 4)


def test_percentile_lists():
    assert {c.fact for c in ic.PCT_NAMED if isinstance(c.fact, int)} == {1023, 1024, 1025, 4095, 4096, 4097}
    assert {h * w for h, w in ic.PCT_SHAPES} >= {1, 2, 3, 4, 5}
    for lo, hi in ic.PCT_PAIRS:
        assert lo >= 0 and hi >= 0 and lo + hi < 1
    assert (0.0, 0.0) in ic.PCT_PAIRS and (0.1, 0.1) in ic.PCT_PAIRS
    # the pairs never leave the sample, whatever its size
    for n in list(range(1, 50)) + [99, 100, 1023, 1024, 1025, 4095, 4096, 4097]:
        for lo, hi in ic.PCT_PAIRS:
            k_lo, k_hi = ic.ranks(n, lo, hi)
            assert 0 <= k_lo < n and 0 <= k_hi < n
    single = ic.pct_image("single", 1, 4100, "f32")
    assert ic.percentiles_model(single, 0.1, 0.1)[0] == 1
    for h, w in ic.PCT_DARK_SHAPES:
        assert w % 4 != 0


def test_percentiles_model_uses_the_row_of_the_sample():
    img = np.arange(1, 16, dtype=f32).reshape(5, 3)                  # samples: flat 0, 4, 8, 12 -> rows 0, 1, 2, 4
    dark = np.array([0, 100, 0, 100, 0], f32)                         # row 1 is zeroed, row 3 holds no sample
    n, lo_hi = ic.percentiles_model(img, 0.0, 0.0, dark)
    assert n == 3 and lo_hi.tolist() == [1.0, 13.0]


def test_pack_and_unpack_keep_the_sentinel():
    imgs = np.arange(24, dtype=f32).reshape(2, 3, 4)
    buf = ic.pack(imgs, 13, 4)
    got, clean = ic.unpack(buf, f32, 2, 3, 4, 13, 4)
    assert clean and np.array_equal(got, imgs) and buf.size == 4 + (13 + 12 + ic.GUARD) * 4
    buf[4 + 12 * 4] ^= 1                                             # the first gap byte
    assert not ic.unpack(buf, f32, 2, 3, 4, 13, 4)[1]


def test_class_sequence_sample_sizes():
    seq = ic.class_sequence(1, 400, f32)
    counts = [int((s.reshape(-1)[::4] > 0).sum()) for s in seq]
    assert counts[0] == 99 and counts[1] == 100 and len(seq) == 6
