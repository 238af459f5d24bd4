"""What the tests of the display-image kernels share (tests/test_image_cases_cpu.py, test_gpu_image_kernels.py): no test in
here.  A plain-numpy model of ouster_hip_image_apply written from the comments of k_image.hip and from image_model.py (every step
one separately rounded numpy operation in the image type T), the order statistics of image_model.py, ctypes callers that lay the
images out on torch device buffers with strides, pointer offsets, guard elements and a sentinel, the launch rule and the vector
conditions of the C ABI restated, and the case lists as data.  No product import at module level."""
from collections import namedtuple

import numpy as np

from image_model import dark_row_medians, kth
from tonemap_model import f16_bits_to_f32

NP = {"u8": np.uint8, "u16": np.uint16, "u32": np.uint32, "f16": np.uint16, "f32": np.float32, "f64": np.float64}
MAP_NONE, MAP_SCALE, MAP_AFFINE = 0, 1, 2
Map = namedtuple("Map", "mode use_dark sub mul add")
SENTINEL = 0xA5          # every byte of an output buffer before the call
GUARD = 8                # guard elements after the last image


# ---- models -----------------------------------------------------------------------------------------------------------------
def to_T(img, in_name, T):
    """the conversion on load: astype(T); FLOAT16 patterns by the reference's integer formula"""
    if in_name == "f16":
        return f16_bits_to_f32(img).astype(T)
    return np.asarray(img).astype(T)


def apply_model(img, in_name, T, dark_row=None, m=None):
    """ouster_hip_image_apply on one (h, w) image: convert, x = max(x - dark[row], 0) when dark counts are given and the map
    asks for them (no map: always), the map, and for SCALE / AFFINE the clamp to [0, 1].  m: a Map or None (maps == NULL)."""
    T = np.dtype(T).type
    with np.errstate(all="ignore"):
        x = to_T(img, in_name, T)
        if dark_row is not None and (m is None or m.use_dark):
            x = x - np.asarray(dark_row, T)[:, None]
            x = np.where(x < 0, T(0), x)
        if m is not None and m.mode != MAP_NONE:
            if m.mode == MAP_AFFINE:
                x = x - T(m.sub)
                x = x * T(m.mul)
                x = x + T(m.add)
            else:
                x = x * T(m.mul)
            x = np.where(x < 0, T(0), x)
            x = np.where(x > 1, T(1), x)
    assert x.dtype == T
    return x


def medians_model(img_T):
    """image_model.dark_row_medians with a zero median as +0.0 (np.partition cannot tell the zeros apart, the kernel stores +0)"""
    med, n_cols = dark_row_medians(img_T)
    med = med.copy()
    med[med == 0] = 0
    return med, n_cols


def ranks(n, lo, hi):
    """the reference's two indices into the n kept samples"""
    return int(float(n) * lo), n - int(float(n) * hi) - 1


def percentiles_model(img_T, lo, hi, dark_row=None):
    """(n, [lo value, hi value]) of every 4th flat element, corrected by its row's dark count, kept when > 0"""
    T = img_T.dtype.type
    x = img_T
    if dark_row is not None:
        with np.errstate(all="ignore"):
            x = x - np.asarray(dark_row, T)[:, None]
        x = np.where(x < 0, T(0), x)
    s = x.reshape(-1)[::4]
    kept = s[s > 0]
    if kept.size == 0:
        return 0, np.zeros(2, T)
    k_lo, k_hi = ranks(kept.size, lo, hi)
    return kept.size, np.array([kth(kept, k_lo), kth(kept, k_hi)], T)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def same_bits_or_nan(a, b):
    """bit for bit, NaN by position only (the payload is not part of the contract)"""
    return a.shape == b.shape and a.dtype == b.dtype and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


# ---- the launch rule and the vector conditions, restated ---------------------------------------------------------------------
def launch_shape(n_images, h, w):
    """(nchunk, want, cap): 4-element chunks of an image, the blocks of 256 lanes they ask for, the blocks an image gets"""
    nchunk = -(-(h * w) // 4)
    return nchunk, -(-nchunk // 256), max(8, 8192 // n_images)


def expect_vec(in_name, n_images, h, w, in_stride=0, out_stride=0, in_off=0, out_off=0):
    """Does ouster_hip_image_apply take 4-element accesses?  The plane pointer is aligned to four input elements (16 bytes at
    most), the output pointer to 16 bytes, and with more than one image both strides are multiples of four elements.  The
    offsets are in bytes from a 256-byte aligned allocation."""
    vb = min(16, 4 * np.dtype(NP[in_name]).itemsize)
    strides = all((s or h * w) % 4 == 0 for s in (in_stride, out_stride)) or n_images == 1
    return in_off % vb == 0 and out_off % 16 == 0 and strides


def chunks_spanning_rows(h, w):
    """4-element chunks of the flat image whose elements lie in more than one row -> (count, most rows in one chunk)"""
    count = most = 0
    for i0 in range(0, h * w, 4):
        rows = {i // w for i in range(i0, min(i0 + 4, h * w))}
        count += len(rows) > 1
        most = max(most, len(rows))
    return count, most


# ---- device buffers ----------------------------------------------------------------------------------------------------------
def pack(imgs, stride, off, guard=GUARD):
    """n images (n, h, w) at `off` bytes + i * stride elements in a byte buffer full of the sentinel, `guard` elements after the
    last image -> uint8 array"""
    imgs = np.ascontiguousarray(imgs)
    n, hw, es = imgs.shape[0], imgs.shape[1] * imgs.shape[2], imgs.dtype.itemsize
    stride = stride or hw
    buf = np.full(off + ((n - 1) * stride + hw + guard) * es, SENTINEL, np.uint8)
    for i in range(n):
        a = off + i * stride * es
        buf[a:a + hw * es] = imgs[i].reshape(-1).view(np.uint8)
    return buf


def unpack(buf, dtype, n, h, w, stride, off, guard=GUARD):
    """-> (images (n, h, w), True when every byte outside the images still holds the sentinel)"""
    es, hw = np.dtype(dtype).itemsize, h * w
    stride = stride or hw
    assert buf.size == off + ((n - 1) * stride + hw + guard) * es
    rest = np.ones(buf.size, bool)
    out = np.empty((n, h, w), dtype)
    for i in range(n):
        a = off + i * stride * es
        out[i] = buf[a:a + hw * es].copy().view(dtype).reshape(h, w)
        rest[a:a + hw * es] = False
    return out, bool((buf[rest] == SENTINEL).all())


def to_dev(torch, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()


def tag(capi, name):
    return {"u8": capi.U8, "u16": capi.U16, "u32": capi.U32, "f16": capi.F16, "f32": capi.F32, "f64": capi.F64}[name]


def device_maps(capi, torch, maps):
    arr = (capi.ImageMap * len(maps))()
    for i, m in enumerate(maps):
        arr[i].mode, arr[i].use_dark, arr[i].sub, arr[i].mul, arr[i].add = m.mode, m.use_dark, m.sub, m.mul, m.add
    return to_dev(torch, np.frombuffer(bytes(arr), np.uint8))


def _ptr(t, off=0):
    return t.data_ptr() + off


def call_apply(gpu, imgs, in_name, out_name, dark=None, maps=None, in_stride=0, out_stride=0, in_off=0, out_off=0, in_place=False):
    """ouster_hip_image_apply on imgs (n, h, w) of NP[in_name].  dark: (n, h) of T or None; maps: a list of Map or None (NULL);
    strides in elements, offsets in bytes.  -> (the whole output buffer as bytes, the whole input buffer afterwards): unpack()
    gives the images and tells whether gaps, lead and guard kept the sentinel.  in_place: out is the plane pointer itself."""
    capi, ctx, torch = gpu
    n, h, w = imgs.shape
    T = NP[out_name]
    d_in = to_dev(torch, pack(imgs.astype(NP[in_name], copy=False), in_stride, in_off))
    if in_place:
        d_out, out_off = d_in, in_off
    else:
        d_out = to_dev(torch, np.full(out_off + ((n - 1) * (out_stride or h * w) + h * w + GUARD) * np.dtype(T).itemsize, SENTINEL, np.uint8))
    assert _ptr(d_in) % 256 == 0 and _ptr(d_out) % 256 == 0
    d_dark = to_dev(torch, np.ascontiguousarray(dark, T)) if dark is not None else None
    d_maps = device_maps(capi, torch, maps) if maps is not None else None
    capi.check(ctx.L.ouster_hip_image_apply(ctx.h, _ptr(d_in, in_off), tag(capi, in_name), _ptr(d_out, out_off), tag(capi, out_name),
                                            n, h, w, in_stride, out_stride, _ptr(d_dark) if d_dark is not None else None,
                                            _ptr(d_maps) if d_maps is not None else None))
    ctx.sync()
    return d_out.cpu().numpy(), d_in.cpu().numpy()


def call_dark_rows(gpu, imgs, in_name, out_name, stride=0, in_off=0, with_n_cols=True):
    """ouster_hip_image_dark_rows -> (medians buffer of T [n * (h - 1) + GUARD], n_cols buffer u32 [n + GUARD]), both pre-filled
    with the sentinel; with_n_cols False passes NULL and returns the n_cols buffer untouched."""
    capi, ctx, torch = gpu
    n, h, w = imgs.shape
    T = NP[out_name]
    d_in = to_dev(torch, pack(imgs.astype(NP[in_name], copy=False), stride, in_off))
    d_med = to_dev(torch, np.full((n * (h - 1) + GUARD) * np.dtype(T).itemsize, SENTINEL, np.uint8))
    d_nc = to_dev(torch, np.full((n + GUARD) * 4, SENTINEL, np.uint8))
    capi.check(ctx.L.ouster_hip_image_dark_rows(ctx.h, _ptr(d_in, in_off), tag(capi, in_name), tag(capi, out_name), n, h, w, stride,
                                                _ptr(d_med), _ptr(d_nc) if with_n_cols else None))
    ctx.sync()
    return d_med.cpu().numpy().view(T), d_nc.cpu().numpy().view(np.uint32)


def call_percentiles(gpu, imgs, in_name, out_name, lo, hi, dark=None, stride=0, in_off=0):
    """ouster_hip_image_percentiles -> (n buffer u32 [n + GUARD], lo_hi buffer of T [2 n + GUARD]), pre-filled with the sentinel"""
    capi, ctx, torch = gpu
    n, h, w = imgs.shape
    T = NP[out_name]
    d_in = to_dev(torch, pack(imgs.astype(NP[in_name], copy=False), stride, in_off))
    d_n = to_dev(torch, np.full((n + GUARD) * 4, SENTINEL, np.uint8))
    d_lh = to_dev(torch, np.full((2 * n + GUARD) * np.dtype(T).itemsize, SENTINEL, np.uint8))
    d_dark = to_dev(torch, np.ascontiguousarray(dark, T)) if dark is not None else None
    capi.check(ctx.L.ouster_hip_image_percentiles(ctx.h, _ptr(d_in, in_off), tag(capi, in_name), tag(capi, out_name), n, h, w, stride,
                                                  _ptr(d_dark) if d_dark is not None else None, lo, hi, _ptr(d_n), _ptr(d_lh)))
    ctx.sync()
    return d_n.cpu().numpy().view(np.uint32), d_lh.cpu().numpy().view(T)


def sentinel_of(dtype, count=1):
    return np.full(count * np.dtype(dtype).itemsize, SENTINEL, np.uint8).view(dtype)


# ---- apply: the cases ---------------------------------------------------------------------------------------------------------
APPLY_RAGGED = [(9, 1), (5, 2), (5, 3), (4, 5), (3, 7), (7, 130), (33, 131), (2, 4097)]
APPLY_TYPE_SHAPES = [(3, 7), (16, 256)]
APPLY_INT_TYPES = [("u8", "f32"), ("u16", "f32"), ("u32", "f32"), ("u8", "f64"), ("u16", "f64"), ("u32", "f64")]
THREE_MAPS = [Map(MAP_NONE, 1, 0.0, 1.0, 0.0), Map(MAP_SCALE, 0, 0.0, 1.0 / 60.0, 0.0), Map(MAP_AFFINE, 1, 10.0, 0.02, 0.1)]

STRIDE_SHAPE = (4, 6, 64)                         # n, h, w
# (in_name, in_stride - hw, out_stride - hw, in_off elements, out_off elements, path)
STRIDE_CASES = [(t, si, so, 0, 0, "vector" if si % 4 == 0 and so % 4 == 0 else "scalar")
                for t in ("f32",) for si in (0, 1, 4) for so in (0, 1, 4)]
STRIDE_CASES += [(t, 0, 0, 1, 0, "scalar") for t in ("f32", "u8", "u16")]
STRIDE_CASES += [("f32", 0, 0, 0, 1, "scalar"), ("u16", 4, 4, 0, 0, "vector"), ("u8", 4, 0, 0, 0, "vector"),
                 ("u8", 0, 0, 4, 0, "vector"),       # u8 planes need 4 bytes only
                 ("u16", 0, 0, 2, 0, "scalar")]      # 4 bytes off: not the 8 that four u16 take

GRID_CASES = [dict(n=1024, h=33, w=256, path="vector"), dict(n=1024, h=3, w=2731, path="scalar")]

HOST_SHAPES = [(5, 3), (33, 131)]


def apply_images(rng, n, h, w, T):
    """float images with negative pixels, pixels above 1 after the maps, and -0.0, +-inf and NaN at a few positions"""
    img = rng.normal(50, 40, (n, h, w)).astype(T)
    flat = img.reshape(n, -1)
    hw = h * w
    for i in range(n):
        for k, v in enumerate((-0.0, np.inf, -np.inf, np.nan, -0.0)):
            flat[i, (3 * k + i + 1) % hw] = v         # small images keep the last writes only
    return img


def apply_dark(rng, n, h, T):
    """dark counts around the pixels' mean, every third row large enough to zero its pixels"""
    d = rng.uniform(0, 60, (n, h)).astype(T)
    d[:, 1::3] = T(1e9)
    return d


def f16_patterns():
    """every exponent with a few mantissas, subnormals, both zeros, the largest finite value -> uint16"""
    p = [0x0000, 0x8000, 0x0001, 0x0002, 0x03FF, 0x8001, 0x83FF, 0x7BFF, 0xFBFF, 0x3C00]
    for e in range(32):
        for mant in (0x000, 0x001, 0x155, 0x3FF):
            p += [(e << 10) | mant, 0x8000 | (e << 10) | mant]
    return np.array(p, np.uint16)


# ---- dark rows: the cases -----------------------------------------------------------------------------------------------------
DARK_SHAPES = [(2, 1), (2, 63), (2, 64), (2, 65), (5, 255), (5, 256), (5, 257), (3, 4095), (2, 4096)]
DARK_TYPES = [("f32", "f32"), ("f64", "f64"), ("u16", "f32")]
WORD_EDGE_MASKS = ["c63", "c64", "c63_64", "last"]


def edge_columns(name, w):
    """the columns of a word-edge mask, or None where the image is too narrow for it"""
    cols = {"c63": [63], "c64": [64], "c63_64": [63, 64], "last": [w - 1]}[name]
    return cols if max(cols) < w else None


def dark_images(h, w, in_name):
    """-> (names, (n, h, w) images, n_cols per image).  Active columns hold a non-zero pixel in row 0; every other column is zero
    in every row.  Differences have both signs with heavy ties at zero.  Float images with h >= 3 also get 'neg_zero': most
    columns hold +0 above -0 in rows 1 and 2 (with h == 2 such a column would be empty), so the median difference is -0.0.  'distinct_even' has no ties: an
    off-by-one rank changes its medians."""
    rng = np.random.default_rng(1000 * h + w)
    dt = NP[in_name]
    is_float = in_name in ("f32", "f64")

    def body(cols):
        img = np.zeros((h, w))
        v = rng.integers(1, 4, (h, len(cols))).astype(np.float64)             # 1 .. 3: ties, differences -2 .. 2
        v[:, rng.random(len(cols)) < 0.4] = 2                                     # constant columns: differences of +0
        if is_float:
            v[1:, :] = np.where(rng.random((h - 1, len(cols))) < 0.2, -v[1:, :], v[1:, :])   # negative pixels as well
        img[:, cols] = v
        return img

    out = []
    out.append(("all_columns", body(list(range(w))), w))
    if w > 1:
        out.append(("all_but_first", body(list(range(1, w))), w - 1))
    out.append(("no_columns", np.zeros((h, w)), 0))
    if w > 1:      # an even number of columns whose differences are all distinct (column c: c in every row pair), so the ranks
        even = w - w % 2                                        # n_cols / 2 and (n_cols - 1) / 2 hold different values
        img = np.zeros((h, w))
        img[:, :even] = 1 + np.arange(even)[None, :] * (np.arange(h)[:, None] + 1)
        out.append(("distinct_even", img, even))
    for name in WORD_EDGE_MASKS:
        cols = edge_columns(name, w)
        if cols is not None:
            out.append((name, body(cols), len(cols)))
    if is_float and h >= 3:
        img = body(list(range(w)))
        img[1, : (3 * w + 3) // 4] = 0.0
        img[2, : (3 * w + 3) // 4] = -0.0
        out.append(("neg_zero", img, w))
    return [o[0] for o in out], np.stack([o[1] for o in out]).astype(dt), [o[2] for o in out]


# ---- percentiles: the cases ---------------------------------------------------------------------------------------------------
PCT_PAIRS = [(0.0, 0.0), (0.5, 0.49), (0.999, 0.0), (0.0, 0.999), (0.1, 0.1)]
PCT_SHAPES = [(1, 1), (1, 2), (1, 3), (1, 4), (1, 5), (1, 4092), (1, 4096), (1, 4100), (4, 4095), (4, 4096), (4, 4097)]
PCT_TYPES = [("f32", "f32"), ("f64", "f64"), ("u8", "f32")]
PCT_FILLS = ["positive", "mixed", "const", "adjacent", "extremes", "single"]
PCT_DARK_SHAPES = [(9, 1), (5, 3), (5, 7), (7, 130), (33, 131)]     # w % 4 != 0: the row of sample j is (4 j) // w


def pct_image(fill, h, w, in_name):
    """one (h, w) image of NP[in_name], or None where the fill needs a float type"""
    rng = np.random.default_rng(17 * h + w + len(fill))
    dt = NP[in_name]
    is_float = in_name in ("f32", "f64")
    hw = h * w
    nsamp = -(-hw // 4)
    if fill == "positive":          # every sample is kept: n is the sample size
        a = rng.uniform(0.5, 2000.0, hw) if is_float else rng.integers(1, 256, hw)
    elif fill == "mixed":           # zeros, negatives, ties
        a = rng.integers(-3, 4, hw) * 10.0 ** rng.integers(-3, 4, hw) if is_float else rng.integers(0, 4, hw)
    elif fill == "const":           # a sample of one key
        a = np.full(hw, 7)
    elif fill == "adjacent":        # two keys that differ in the lowest byte only
        if not is_float:
            return None
        a = np.where(rng.random(hw) < 0.5, dt(1.0), np.nextafter(dt(1.0), dt(2.0)))
        a[0], a[4 * (nsamp - 1)] = np.nextafter(dt(1.0), dt(2.0)), dt(1.0)          # both present in any sample of two or more
    elif fill == "extremes":        # keys that differ in the top byte: FLT_MIN / 2 (a float32 subnormal) next to +inf
        a = np.where(rng.random(hw) < 0.5, np.float32(2.0 ** -127), np.inf) if is_float else np.where(rng.random(hw) < 0.5, 1, 255)
        a[0], a[4 * (nsamp - 1)] = a.max(), a.min()
    elif fill == "single":          # n == 1
        a = np.full(hw, -1.0 if is_float else 0.0)
        a[4 * (nsamp // 2)] = 3
    else:
        raise KeyError(fill)
    return np.asarray(a).astype(dt).reshape(h, w)


# name, (h, w), fill, (lo, hi), the fact the case stands for
PctNamed = namedtuple("PctNamed", "name shape fill pair fact")
PCT_NAMED = [
    PctNamed("same_n1", (1, 1), "positive", (0.5, 0.49), "same"),
    PctNamed("same_n2", (1, 5), "positive", (0.5, 0.49), "same"),
    PctNamed("same_n100", (1, 400), "positive", (0.5, 0.49), "same"),
    PctNamed("same_n1_of_many", (1, 4100), "single", (0.1, 0.1), "same"),
    PctNamed("last_digit", (1, 4096), "adjacent", (0.0, 0.0), "last_digit"),
    PctNamed("last_digit_small", (1, 5), "adjacent", (0.0, 0.0), "last_digit"),
    PctNamed("first_digit", (4, 4097), "extremes", (0.0, 0.0), "first_digit"),
    PctNamed("one_key", (4, 4095), "const", (0.1, 0.1), "one_key"),
    PctNamed("minimum", (1, 4092), "positive", (0.0, 0.999), "lo_is_min"),
    PctNamed("maximum", (1, 4100), "positive", (0.999, 0.0), "hi_is_max"),
    PctNamed("n_1023", (1, 4092), "positive", (0.1, 0.1), 1023),
    PctNamed("n_1024", (1, 4096), "positive", (0.1, 0.1), 1024),
    PctNamed("n_1025", (1, 4100), "positive", (0.1, 0.1), 1025),
    PctNamed("n_4095", (4, 4095), "positive", (0.5, 0.49), 4095),
    PctNamed("n_4096", (4, 4096), "positive", (0.5, 0.49), 4096),
    PctNamed("n_4097", (4, 4097), "positive", (0.5, 0.49), 4097),
]


def pct_named_ranks(case, in_name, out_name):
    """-> (n, k_lo, k_hi, kept samples in T) of a named case"""
    img = pct_image(case.fill, *case.shape, in_name).astype(NP[out_name])
    s = img.reshape(-1)[::4]
    kept = s[s > 0]
    k_lo, k_hi = ranks(kept.size, *case.pair)
    return kept.size, k_lo, k_hi, kept


# ---- the classes: six calls per shape -----------------------------------------------------------------------------------------
CLASS_SHAPES = [(5, 7), (1, 400), (33, 130)]


def class_sequence(h, w, dtype):
    """six images.  1 x 400 (a sample of exactly 100): call 0 has 99 positive samples (the early return), call 1 exactly 100."""
    rng = np.random.default_rng(h * 100 + w)
    out = []
    for i in range(6):
        img = rng.normal(100, 10, (h, w)) + rng.normal(0, 3, (h, 1)) + 5 * i
        if (h, w) == (1, 400) and i == 0:
            img[0, 0] = 0.0                     # flat element 0 is a sample
        out.append(img.astype(dtype))
    return out
