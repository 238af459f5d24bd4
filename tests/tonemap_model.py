"""Plain-numpy model of the RGB overloads of ouster::sdk::core::image::AutoExposure and of LocalToneMapper, written from the
description of their semantics, not from the product.  No product import.

Every arithmetic step is one separately rounded IEEE operation in the image type T (float32 or float64), nothing is contracted, the
carried state is float64.  What decides the bits:

  f16 front end   works on the integer pattern: 0 and 0x7e00 give 0.0f, everything else uint32(bits + 0x1C000) << 13 read as a
                  float.  Not an IEEE half conversion: subnormals, infinities and patterns with the sign bit give what the formula
                  gives, always a finite positive float.
  luminance       (r * T(0.299) + g * T(0.587)) + b * T(0.114), constants rounded to T first.
  sample          pixels 0, 4, 8, ... of the flat h * w PIXEL index, kept when lum > 0; n of them.  n < 100: nothing happens (the
                  f16 forms return the plain converted image), the counter stays.  lo = kth(trunc(n * lo_percentile)),
                  hi = kth(n - trunc(n * hi_percentile) - 1).
  map             AutoExposureModel's state machine and choice (tests/image_model.py), the constants cast to T before use.  RGB
                  AutoExposure then clamps all 3 * h * w elements to [0, 1]; LocalToneMapper does not, and advances its counter
                  right after the map.
  compression     only when hi_state < compress_dr_max_lum (doubles).  lum > T(0.8): x = float32((lum - T(0.8)) + 1.0), the + 1.0 a
                  double addition; fast_log10(x) = (float32(int32(bits(x)) - 0x3F800000) * 1.1920929e-7f) * 0.30103f;
                  new_lum = T(0.8) + that; every channel *= new_lum / lum.
  Reinhard        x = max(x, 0); x = x / (T(1) + x); lum_ae from the result.
  CLAHE tables    8 x 8 tiles (y0 = ty * h // 8, y1 = (ty + 1) * h // 8, x alike), bin = min(int(float32(lum) * 1024.0f), 1023),
                  counts held as float32, clip = float32(tile_pixels) / 1024, excess = float32 sum IN BIN ORDER of hist - clip
                  over the bins above clip (which become clip), redistribute = excess / 1024, cdf = running float32 sum IN BIN
                  ORDER of hist[bin] + redistribute, lut[bin] = min(cdf * (1.0f / float32(tile_pixels)), 1.0f).
  CLAHE look-up   tx_f = (float32(x) + 0.5f) * 8 / w - 0.5f; tx0 = clamp(floor(tx_f), 0, 7); tx1 = min(7, tx0 + 1);
                  fx = tx_f - float32(tx0) -- NEGATIVE in the first half tile, where the blend extrapolates; rows alike;
                  mapped = (1 - fy) * ((1 - fx) * L00 + fx * L01) + fy * ((1 - fx) * L10 + fx * L11) in float32, then cast to T.
  last pass       color_factor = T(0.75), times T(max(0, (hi_state - 0.5) / 0.5)) (ratio in double, rounded once) when
                  hi_state < 1.  scale = lum_clahe / lum_ae where lum_ae > T(1e-6), else T(1).  Without colour correction or with
                  color_factor == 0: c = min(c * scale, 1).  Otherwise c = c * scale, then
                  c = (-lum_clahe * color_factor) + c * (T(1) + color_factor), clamped to [0, 1].

Preconditions (the reference is undefined outside them): lo_percentile + hi_percentile < 1; every float / double input element is
finite (any f16 pattern is fine); h >= 8 and w >= 8 (the reference has empty tiles below that and blends NaN tables into the image;
the product refuses such images, the model asserts)."""
import numpy as np

AE_STRIDE = 4
AE_MIN_NONZERO_POINTS = 100
TILES = 8
BINS = 1024
MAP_NONE, MAP_SCALE, MAP_AFFINE = 0, 1, 2
f32 = np.float32


def kth(values, k):
    """k-th smallest (0-based) of a 1-D array: what nth_element leaves at position k."""
    return np.partition(values, k)[k]


def f16_bits_to_f32(bits):
    """uint16 patterns -> float32, the reference's integer formula"""
    b = np.asarray(bits).astype(np.uint32)
    out = ((b + np.uint32(0x1C000)) << np.uint32(13)).astype(np.uint32)
    out[(b == 0) | (b == 0x7e00)] = 0
    return out.view(np.float32)


def fast_log10(x):
    """x: float32 array"""
    x = np.ascontiguousarray(x, np.float32)
    d = (x.view(np.int32).astype(np.int64) - 0x3F800000).astype(np.int32)
    return (d.astype(np.float32) * f32(1.1920929e-7)) * f32(0.30103)


def luminance(img):
    """img (..., 3) of T -> (...) of T"""
    T = img.dtype.type
    return (img[..., 0] * T(0.299) + img[..., 1] * T(0.587)) + img[..., 2] * T(0.114)


def lum_stats(img, lo_percentile, hi_percentile):
    """(n, lo, hi) of the luminance sample of an (h, w, 3) image of T; lo = hi = 0 when n == 0"""
    T = img.dtype.type
    lum = luminance(img.reshape(-1, 3)[::AE_STRIDE])
    kept = lum[lum > 0]
    n = kept.size
    if n == 0:
        return 0, T(0), T(0)
    k_lo = min(int(float(n) * lo_percentile), n - 1)
    k_hi = max(n - int(float(n) * hi_percentile) - 1, 0)
    return n, kth(kept, k_lo), kth(kept, k_hi)


def bins_of(lum):
    return np.minimum((lum.astype(np.float32) * f32(BINS)).astype(np.int32), BINS - 1)


def tile_bounds(n):
    return [(t * n // TILES, (t + 1) * n // TILES) for t in range(TILES)]


def clahe_luts(lum):
    """lum (h, w) of T -> (64, 1024) float32"""
    h, w = lum.shape
    assert h >= TILES and w >= TILES
    bins = bins_of(lum)
    luts = np.zeros((TILES * TILES, BINS), np.float32)
    for ty, (y0, y1) in enumerate(tile_bounds(h)):
        for tx, (x0, x1) in enumerate(tile_bounds(w)):
            pixels = (y1 - y0) * (x1 - x0)
            hist = np.bincount(bins[y0:y1, x0:x1].reshape(-1), minlength=BINS).astype(np.float32)   # exact below 2^24
            clip = f32(pixels) / f32(BINS)
            over = hist > clip
            excess = f32(0)
            if over.any():
                excess = np.cumsum(hist[over] - clip, dtype=np.float32)[-1]       # sequential, in bin order
            hist[over] = clip
            redistribute = excess / f32(BINS)
            cdf = np.cumsum(hist + redistribute, dtype=np.float32)
            luts[ty * TILES + tx] = np.minimum(cdf * (f32(1) / f32(pixels)), f32(1))
    return luts


def tile_coords(n):
    """(t0, t1, f) per pixel coordinate 0 .. n - 1"""
    t_f = (np.arange(n).astype(np.float32) + f32(0.5)) * f32(TILES) / f32(n) - f32(0.5)
    t0 = np.clip(np.floor(t_f).astype(np.int32), 0, TILES - 1)
    return t0, np.minimum(TILES - 1, t0 + 1), t_f - t0.astype(np.float32)


def clahe_apply(lum, luts):
    h, w = lum.shape
    bins = bins_of(lum)
    tx0, tx1, fx = tile_coords(w)
    ty0, ty1, fy = tile_coords(h)
    L = luts.reshape(TILES, TILES, BINS)
    fx, fy = fx[None, :], fy[:, None]
    l00, l01 = L[ty0[:, None], tx0[None, :], bins], L[ty0[:, None], tx1[None, :], bins]
    l10, l11 = L[ty1[:, None], tx0[None, :], bins], L[ty1[:, None], tx1[None, :], bins]
    mapped = (f32(1) - fy) * ((f32(1) - fx) * l00 + fx * l01) + fy * ((f32(1) - fx) * l10 + fx * l11)
    assert mapped.dtype == np.float32
    return mapped.astype(lum.dtype)


class Params:
    """What the state machine hands to the per-pixel work: ouster_hip_tonemap_params"""
    def __init__(self, mode=MAP_NONE, sub=0.0, mul=1.0, add=0.0, compress=False, color_ramp=1.0, color_correct=True):
        self.mode, self.sub, self.mul, self.add = mode, float(sub), float(mul), float(add)
        self.compress, self.color_ramp, self.color_correct = bool(compress), float(color_ramp), bool(color_correct)

    def key(self):
        return (self.mode, self.sub, self.mul, self.add, self.compress, self.color_ramp, self.color_correct)


def apply_map(flat, p):
    """the affine map on every element, in place, no clamp"""
    T = flat.dtype.type
    with np.errstate(over="ignore", invalid="ignore"):
        if p.mode == MAP_AFFINE:
            flat[:] = flat - T(p.sub)
            flat[:] = flat * T(p.mul)
            flat[:] = flat + T(p.add)
        elif p.mode == MAP_SCALE:
            flat[:] = flat * T(p.mul)


def tonemap_pixels(img, p):
    """Everything of LocalToneMapper::apply after the state machine, in place on an (h, w, 3) image of T."""
    if p.mode == MAP_NONE:
        return
    T = img.dtype.type
    h, w, _ = img.shape
    px = img.reshape(-1, 3)
    apply_map(img.reshape(-1), p)
    if p.compress:
        lum = luminance(px)
        sel = lum > T(0.8)
        if sel.any():
            ls = lum[sel]
            x = ((ls - T(0.8)).astype(np.float64) + 1.0).astype(np.float32)
            new_lum = T(0.8) + fast_log10(x).astype(img.dtype)
            scale = new_lum / ls
            px[sel] = px[sel] * scale[:, None]
    flat = img.reshape(-1)
    flat[:] = np.where(flat < 0, T(0), flat)
    flat[:] = flat / (T(1) + flat)
    lum_ae = luminance(img)
    lum_clahe = clahe_apply(lum_ae, clahe_luts(lum_ae))
    color_factor = T(0.75) * T(p.color_ramp)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(lum_ae > T(1e-6), lum_clahe / lum_ae, T(1)).astype(img.dtype)
    c = img * scale[..., None]
    if not p.color_correct or color_factor == T(0):
        img[:] = np.where(c > T(1), T(1), c)
    else:
        c = (-lum_clahe * color_factor)[..., None] + c * (T(1) + color_factor)
        c = np.where(c > T(1), T(1), c)
        img[:] = np.where(c > T(0), c, T(0))      # std::max(T(0), c): a -0.0 comes out as +0.0


class _LumExposure:
    """The state machine both classes share: AutoExposureModel's, on the luminance sample."""
    def __init__(self, lo_percentile, hi_percentile, update_every, damping):
        self.lo_percentile, self.hi_percentile = float(lo_percentile), float(hi_percentile)
        self.update_every, self.damping = int(update_every), float(damping)
        self.lo_state = self.hi_state = self.lo = self.hi = -1.0
        self.initialized = False
        self.counter = 0
        self.stats = []      # per call: (n, lo, hi) as the device would report them, None when the call did not sample
        self.branches = []   # per call: see the subclasses
        self.params = []     # per call: the Params record

    def _map(self, img, update_state):
        """-> Params with the map only (mode NONE: early return), advancing the state"""
        self.stats.append(None)
        if self.counter == 0 and update_state:
            n, lo, hi = lum_stats(img, self.lo_percentile, self.hi_percentile)
            self.stats[-1] = (n, float(lo), float(hi))
            if n < AE_MIN_NONZERO_POINTS:
                return Params(), "early"
            self.lo, self.hi = float(lo), float(hi)
            if not self.initialized:
                self.initialized = True
                self.lo_state, self.hi_state = self.lo, self.hi
        if not self.initialized:
            return Params(), "uninit"
        if update_state:
            self.lo_state = self.damping * self.lo_state + (1.0 - self.damping) * self.lo
            self.hi_state = self.damping * self.hi_state + (1.0 - self.damping) * self.hi
        with np.errstate(divide="ignore", invalid="ignore"):
            scale = np.float64(1.0 - (self.lo_percentile + self.hi_percentile)) / np.float64(self.hi_state - self.lo_state)
            if np.isinf(scale) or np.isnan(scale):
                p, name = Params(MAP_SCALE, mul=np.float64(0.5) / np.float64(self.hi_state)), "inf"
            elif scale * (0.0 - self.lo_state) + self.lo_percentile <= 0.0:
                p, name = Params(MAP_AFFINE, self.lo_state, scale, self.lo_percentile), "affine"
            else:
                p, name = Params(MAP_SCALE, mul=np.float64(1.0 - self.hi_percentile) / np.float64(self.hi_state)), "hi"
        if update_state:
            self.counter = (self.counter + 1) % self.update_every
        return p, name


class RgbAutoExposureModel(_LumExposure):
    """AutoExposure::update on (h, w, 3) images.  branches: "early", "uninit", "inf", "affine" or "hi"."""
    def __init__(self, lo_percentile=0.1, hi_percentile=0.1, update_every=3, damping=0.9):
        super().__init__(lo_percentile, hi_percentile, update_every, damping)

    def update(self, img, update_state=True):
        T = img.dtype.type
        p, name = self._map(img, update_state)
        self.branches.append(name)
        self.params.append(p)
        if p.mode == MAP_NONE:
            return
        flat = img.reshape(-1)
        apply_map(flat, p)
        flat[:] = np.where(flat < 0, T(0), flat)
        flat[:] = np.where(flat > 1, T(1), flat)

    def update_f16(self, bits, update_state=True):
        out = f16_bits_to_f32(bits)
        self.update(out, update_state)
        return out


class LocalToneMapperModel(_LumExposure):
    """LocalToneMapper::update.  branches: "early" / "uninit", or (map, compress on?, "off" | "zero" | "ramp" | "full")."""
    def __init__(self, lo_percentile=0.0, hi_percentile=0.2, update_every=1, damping=0.3, compress_dr_max_lum=0.2,
                 color_correct=True):
        super().__init__(lo_percentile, hi_percentile, update_every, damping)
        if isinstance(compress_dr_max_lum, bool):            # the compress_dr constructor
            compress_dr_max_lum = 0.2 if compress_dr_max_lum else 0.0
        self.compress_dr_max_lum, self.color_correct = float(compress_dr_max_lum), bool(color_correct)

    def update(self, img, update_state=True):
        p, name = self._map(img, update_state)
        p.color_correct = self.color_correct
        if p.mode != MAP_NONE:
            p.compress = self.hi_state < self.compress_dr_max_lum
            p.color_ramp = max(0.0, (self.hi_state - 0.5) / 0.5) if self.hi_state < 1.0 else 1.0
            color = "off" if not self.color_correct else "zero" if p.color_ramp == 0.0 else "ramp" if self.hi_state < 1.0 else "full"
            name = (name, p.compress, color)
        self.branches.append(name)
        self.params.append(p)
        tonemap_pixels(img, p)

    def update_f16(self, bits, update_state=True):
        out = f16_bits_to_f32(bits)
        self.update(out, update_state)
        return out
