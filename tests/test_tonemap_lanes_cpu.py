"""CPU-only: k_tm_hist, k_tm_luts and k_tm_finish of csrc/k_tonemap.hip compiled for the host, one thread per lane and 64 lanes per
workgroup (tests/cpp/tonemap_lanes.cpp over tests/cpp/host_lanes/hip/hip_runtime.h, whose integer atomics are real ones), against tests/tonemap_model.py bit for bit: the counts, the tables and the images.  It checks
what can go wrong without a GPU in sight -- tile bounds, the order of the float sums, the extrapolating blend, rows that change
inside a lane's four pixels, strides, in place and out of place; the device's own arithmetic and the C ABI around the kernels are
tests/test_gpu_tonemap.py's business."""
import struct
import subprocess

import numpy as np
import pytest

import cpp_tools
import tonemap_cases as K
import tonemap_model as M

F16, F32, F64 = 12, 9, 10
GUARD = -7.25


@pytest.fixture(scope="module")
def lanes():
    return cpp_tools.build("tonemap_lanes")[0]


def run(exe, tmp_path, images, records, out_dtype, in_place, pad_in=0, pad_out=0, pieces=0):
    """images: list of equally shaped (h, w, 3) arrays (uint16 patterns / float32 / float64) -> (outputs [n] of (h, w, 3), the
    guard elements behind each output, luts (n, 64, 1024), hist (n, 64, 1024))"""
    n, (h, w, _) = len(images), images[0].shape
    in_dtype = images[0].dtype
    tag = {np.dtype(np.uint16): F16, np.dtype(np.float32): F32, np.dtype(np.float64): F64}[in_dtype]
    dense = 3 * h * w
    in_stride, out_stride = dense + pad_in, dense + (pad_in if in_place else pad_out)
    src = np.full((n, in_stride), 77 if tag == F16 else GUARD, in_dtype)
    for i, img in enumerate(images):
        src[i, :dense] = img.reshape(-1)
    dst = np.full((n, out_stride), GUARD, out_dtype)
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("<8I", tag, n, h, w, in_stride, out_stride, int(in_place), pieces))
        for p in records:
            f.write(K.pack_params(p))
        f.write(src.tobytes())
        if not in_place:
            f.write(dst.tobytes())
    subprocess.check_call([exe, case, res], timeout=600)
    raw = open(res, "rb").read()
    nb = n * out_stride * np.dtype(out_dtype).itemsize
    out = np.frombuffer(raw[:nb], out_dtype).reshape(n, out_stride)
    tables = n * 64 * 1024
    luts = np.frombuffer(raw[nb:nb + 4 * tables], np.float32).reshape(n, 64, 1024)
    hist = np.frombuffer(raw[nb + 4 * tables:], np.uint32).reshape(n, 64, 1024)
    return [out[i, :dense].reshape(h, w, 3) for i in range(n)], out[:, dense:], luts, hist


def model_tables(img, p):
    """the model's counts and tables for one original image"""
    x = img.copy()
    T = x.dtype.type
    M.apply_map(x.reshape(-1), p)
    if p.compress:
        px = x.reshape(-1, 3)
        lum = M.luminance(px)
        sel = lum > T(0.8)
        ls = lum[sel]
        scale = (T(0.8) + M.fast_log10(((ls - T(0.8)).astype(np.float64) + 1.0).astype(np.float32)).astype(x.dtype)) / ls
        px[sel] = px[sel] * scale[:, None]
    flat = x.reshape(-1)
    flat[:] = np.where(flat < 0, T(0), flat)
    flat[:] = flat / (T(1) + flat)
    lum_ae = M.luminance(x)
    bins = M.bins_of(lum_ae)
    h, w = bins.shape
    hist = np.zeros((64, 1024), np.uint32)
    for ty, (y0, y1) in enumerate(M.tile_bounds(h)):
        for tx, (x0, x1) in enumerate(M.tile_bounds(w)):
            hist[ty * 8 + tx] = np.bincount(bins[y0:y1, x0:x1].reshape(-1), minlength=1024)
    return hist, M.clahe_luts(lum_ae)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("h,w", [(8, 8), (9, 13), (37, 130)])
def test_every_pixel_path_in_place(lanes, tmp_path, h, w, dtype):
    seen = set()
    for k, path in enumerate(K.PIXEL_PATHS):
        img, p, want, branch = K.model_case(path, h, w, dtype, seed=100 * h + k)
        seen.add(branch)
        outs, guard, luts, hist = run(lanes, tmp_path, [img], [p], dtype, in_place=True, pad_in=5)
        want_hist, want_luts = model_tables(img, p)
        assert np.array_equal(hist[0], want_hist), path
        assert K.same_bits(luts[0], want_luts), path
        assert K.same_bits(outs[0], want), (path, np.abs(outs[0] - want).max())
        assert (guard == GUARD).all(), path
    assert {b[0] for b in seen} == {"affine", "inf", "hi"} and {b[1] for b in seen} == {True, False}
    assert {b[2] for b in seen} == {"zero", "ramp", "full", "off"}


@pytest.mark.parametrize("h,w", [(8, 8), (9, 13), (37, 130)])
def test_f16_input_out_of_place(lanes, tmp_path, h, w):
    for k, path in enumerate(("dark", "full", "no_color")):
        level, _, kw = K.PIXEL_PATHS[path]
        rng = np.random.default_rng(7 * h + k)
        m = M.LocalToneMapperModel(**kw)
        m.update_f16(K.to_f16_bits(K.scene(rng, 32, 64, level)))
        bits = K.to_f16_bits(K.scene(rng, h, w, level))
        want = m.update_f16(bits, False)
        outs, guard, _, _ = run(lanes, tmp_path, [bits], [m.params[-1]], np.float32, in_place=False, pad_in=3, pad_out=7)
        assert K.same_bits(outs[0], want), path
        assert (guard == GUARD).all()


@pytest.mark.parametrize("dtype,pad", [(np.float32, 0), (np.float32, 4), (np.float32, 3), (np.float64, 2), (np.float64, 1)])
def test_two_images_one_launch_strides_and_an_early_return(lanes, tmp_path, dtype, pad):
    """Two different images with their own records and a third whose record says NONE (the early return), dense, padded to an
    aligned stride (the vector path) and to an odd one (the scalar path); bands of a tile's rows forced to 3 per tile."""
    a, pa, wa, _ = K.model_case("dark", 37, 130, dtype, seed=1)
    b, pb, wb, _ = K.model_case("full", 37, 130, dtype, seed=2)
    c = K.scene(np.random.default_rng(3), 37, 130, 1.0, dtype)
    for in_place in (True, False):
        outs, guard, luts, _ = run(lanes, tmp_path, [a, b, c], [pa, pb, M.Params()], dtype, in_place, pad_in=pad, pad_out=pad + 4, pieces=3)
        assert K.same_bits(outs[0], wa) and K.same_bits(outs[1], wb) and K.same_bits(outs[2], c), in_place
        assert (guard == GUARD).all()
        assert (luts[2] == np.float32(GUARD)).all()          # nothing was computed for the skipped image


def test_one_pixel_tiles_and_the_negative_weights(lanes, tmp_path):
    """8 x 8: every tile is one pixel, every table a step; the outer half tile of a 16 x 64 image blends with a negative weight"""
    img, p, want, _ = K.model_case("full", 8, 8, np.float32, seed=9)
    outs, _, luts, hist = run(lanes, tmp_path, [img], [p], np.float32, in_place=False)
    assert (hist[0].sum(axis=1) == 1).all()
    assert K.same_bits(outs[0], want)
    _, _, fx = M.tile_coords(64)
    assert fx[0] < 0 and fx[3] < 0 and fx[4] >= 0
    img, p, want, _ = K.model_case("ramp", 16, 64, np.float64, seed=10)
    outs, _, _, _ = run(lanes, tmp_path, [img], [p], np.float64, in_place=True)
    assert K.same_bits(outs[0], want)
