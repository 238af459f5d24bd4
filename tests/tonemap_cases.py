"""The images, sequences and parameter records the tone-map tests share (tests/test_tonemap_*.py, tests/test_gpu_tonemap.py):
HDR-like RGB scenes with dropped pixels, hot spots and a channel below zero, brightness sweeps that carry hi_state across 0.2, 0.5
and 1.0 in both directions, and the packing of a model record into ouster_hip_tonemap_params.  No product import."""
import struct

import numpy as np

import tonemap_model as M

# scene brightness per frame: with sigma 1.3 the 80th percentile of the luminance is about 3 x the level
LEVELS = [0.03, 0.08, 0.25, 0.7, 2.0, 5.0, 2.0, 0.7, 0.25, 0.08, 0.03, 0.02]
FLAGS = [1, 1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1]

# every way LocalToneMapper is constructed in the sequence tests: (name, model kwargs, first frame constant?)
LTM_CONFIGS = [
    ("default", dict(), False),
    ("every3", dict(update_every=3), False),
    ("const_first", dict(), True),
    ("hi_map", dict(lo_percentile=0.1, hi_percentile=0.2, update_every=1, damping=0.3, compress_dr_max_lum=0.2, color_correct=True), False),
    ("no_color", dict(lo_percentile=0.0, hi_percentile=0.2, update_every=1, damping=0.3, compress_dr_max_lum=0.2, color_correct=False), False),
    ("no_compress", dict(lo_percentile=0.0, hi_percentile=0.1, update_every=2, damping=0.5, compress_dr_max_lum=False, color_correct=True), False),
]

# the RGB AutoExposure objects of the sequence tests: (model kwargs, first frame constant?)
AE_CONFIGS = [
    (dict(), False),
    (dict(lo_percentile=0.0, hi_percentile=0.1, update_every=1, damping=0.5), True),
    (dict(lo_percentile=0.1, hi_percentile=0.1, update_every=2, damping=0.5), False),
]


def scene(rng, h, w, level, dtype=np.float32, sigma=1.3):
    """An (h, w, 3) image: log-normal luminance around `level`, 3 % dropped pixels, 1 % hot spots (x 40: they reach the
    compression), 1 % pixels whose blue channel is far below zero (lum <= 0)."""
    img = rng.lognormal(0.0, sigma, (h, w, 1)) * level * rng.uniform(0.4, 1.6, (h, w, 3))
    img[rng.random((h, w)) < 0.03] = 0
    img[rng.random((h, w)) < 0.01] *= 40
    neg = rng.random((h, w)) < 0.01
    img[neg, 2] = -8 * img[neg, 2]
    return img.astype(dtype)


def to_f16_bits(img):
    """float image -> FLOAT16 patterns (uint16), with the patterns a sensor drops pixels as and the formula's odd ones mixed in"""
    with np.errstate(over="ignore"):
        bits = np.ascontiguousarray(img.astype(np.float16)).view(np.uint16).copy()
    flat = bits.reshape(-1)
    for k, pat in enumerate((0x7e00, 0x0001, 0x7C00, 0xBC00, 0x0000)):
        flat[7 + 13 * k::97] = pat
    return bits


def frames(h, w, dtype, seed, const_first=False):
    """12 (image, update_state) pairs: the brightness sweep; frame 7 nearly black (fewer than 100 positive samples)"""
    rng = np.random.default_rng(seed)
    out = []
    for i, (level, flag) in enumerate(zip(LEVELS, FLAGS)):
        img = scene(rng, h, w, level, dtype)
        if i == 0 and const_first:
            img = np.full((h, w, 3), 0.37, dtype)
        if i == 7:
            img = np.zeros((h, w, 3), dtype)
            img.reshape(-1, 3)[:4 * 60:4] = 0.5
        out.append((img, bool(flag)))
    return out


def ae_frames(h, w, dtype, seed, const_first=False):
    """6 of the 12 frames for the RGB AutoExposure sequences; the nearly black one is the fourth"""
    fr = frames(h, w, dtype, seed, const_first)
    return [fr[i] for i in (0, 1, 2, 7, 4, 5)]


def pack_params(p):
    """tonemap_model.Params -> the 48 bytes of ouster_hip_tonemap_params"""
    return struct.pack("<iidddiid", p.mode, 0, p.sub, p.mul, p.add, int(p.compress), int(p.color_correct), p.color_ramp)


def pack_map(p):
    """tonemap_model.Params -> the 32 bytes of ouster_hip_image_map"""
    return struct.pack("<iiddd", p.mode, 0, p.sub, p.mul, p.add)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# (level, const, model kwargs) -> the ways through the per-pixel code: a dark scene (affine map, compression, colour factor 0),
# the colour ramp, full colour, colour correction off, the inf map, the hi map
PIXEL_PATHS = {
    "dark": (0.03, False, dict()),
    "ramp": (0.25, False, dict()),
    "full": (2.0, False, dict()),
    "no_color": (2.0, False, dict(LTM_CONFIGS[4][1])),
    "inf": (1.0, True, dict()),
    "hi_map": (0.7, False, dict(LTM_CONFIGS[3][1])),
}


def model_case(path, h, w, dtype, seed):
    """One image of any size with state to map it by: a fresh model sees a 32 x 64 scene of the same kind first, then the image
    itself with update_state = False.  -> (original image, the model's record, the model's output, its branch)"""
    level, const, kw = PIXEL_PATHS[path]
    rng = np.random.default_rng(seed)
    m = M.LocalToneMapperModel(**kw)
    m.update(np.full((32, 64, 3), 0.37, dtype) if const else scene(rng, 32, 64, level, dtype))
    img = scene(rng, h, w, level, dtype)
    want = img.copy()
    m.update(want, False)
    return img, m.params[-1], want, m.branches[-1]
