"""Plain numpy model of ouster::sdk::core::frame_ops, written from the semantics (not from the product): the yardstick of
tests/test_gpu_frame_ops.py, pinned by hand-computed cases in tests/test_frame_ops_model.py.

Every function returns new arrays and leaves its inputs alone.  "Invalidated" masks are boolean (h, w) arrays, True where
a pixel gets the invalid value."""
import math

import numpy as np

SECOND_RETURN_FIELDS = ("RANGE2", "SIGNAL2", "REFLECTIVITY2", "FLAGS2")
DTYPES = ("uint8", "uint16", "uint32", "uint64", "int8", "int16", "int32", "int64", "float32", "float64")


def cast_invalid(invalid, dtype):
    """static_cast<T>(invalid) where it is defined: toward zero for integers; ValueError where the reference is undefined."""
    dtype = np.dtype(dtype)
    invalid = float(invalid)
    if dtype.kind in "ui":
        if math.isnan(invalid) or math.isinf(invalid):
            raise ValueError(f"invalid == {invalid} does not fit {dtype}")
        t = int(invalid)   # Python truncates toward zero, exactly
        info = np.iinfo(dtype)
        if t < info.min or t > info.max:
            raise ValueError(f"invalid == {invalid} does not fit {dtype}")
        return dtype.type(t)
    if dtype == np.float32 and math.isfinite(invalid) and abs(invalid) > float(np.finfo(np.float32).max):
        raise ValueError(f"invalid == {invalid} does not fit {dtype}")
    return dtype.type(invalid)


def inside(values, lower, upper):
    """lower <= double(v) <= upper; u64 / i64 -> double rounds to nearest even (numpy's astype does); NaN is outside."""
    v = np.asarray(values).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (v >= lower) & (v <= upper)


def apply(img, invalidated, invalid=0):
    out = np.array(img, copy=True)
    out[invalidated] = cast_invalid(invalid, out.dtype)
    return out


def clip(img, lower, upper, invalid=0):
    """kept iff inside [lower, upper]; NaN is replaced"""
    return apply(img, ~inside(img, lower, upper), invalid)


def key_invalidated(key, lower, upper):
    """filter_field: pixels whose key lies INSIDE [lower, upper] are invalidated; a NaN key is kept"""
    return inside(key, lower, upper)


def rows_invalidated(h, w, lower, upper):
    m = np.zeros((h, w), dtype=bool)
    m[lower:upper, :] = True
    return m


def destagger(img, shifts, inverse=False):
    """destaggered[r, (c + shift[r]) mod w] = img[r, c]"""
    img = np.asarray(img)
    out = np.empty_like(img)
    for r in range(img.shape[0]):
        out[r] = np.roll(img[r], -int(shifts[r]) if inverse else int(shifts[r]), axis=0)
    return out


def cols_invalidated(h, w, shifts, lower, upper):
    """filter_uv "v" evaluated on the staggered image: (r, c) goes iff ((c + shift[r]) mod w) in [lower, upper)"""
    c = np.arange(w, dtype=np.int64)[None, :]
    s = np.asarray(shifts, dtype=np.int64)[:, None]
    d = np.mod(c + s, w)   # numpy's mod is the mathematical one for a positive modulus
    return (d >= lower) & (d < upper)


def cols_invalidated_via_destagger(h, w, shifts, lower, upper):
    """the reference's route: destagger, blank the columns, stagger back -- on a mask image"""
    keep = np.ones((h, w), dtype=np.uint8)
    d = destagger(keep, shifts)
    d[:, lower:upper] = 0
    return destagger(d, shifts, inverse=True) == 0


def mask_invalidated(mask):
    return np.asarray(mask) == 0


def xyz_invalidated(xyz, axis, lower, upper, h, w):
    """xyz: (h * w, 3) or (h, w, 3) points of the staggered image"""
    return inside(np.asarray(xyz).reshape(h, w, 3)[:, :, axis], lower, upper)


def xyz_source(field, has_range, has_range2):
    """which range field's cloud decides for `field` in filter_xyz (None: neither exists, nothing happens)"""
    if not has_range and not has_range2:
        return None
    if field in SECOND_RETURN_FIELDS:
        return "RANGE2" if has_range2 else "RANGE"
    return "RANGE" if has_range else "RANGE2"


def uv_bound(val, coord_size):
    """the Python face's reading of a filter_uv bound: floats in [0, 1] are fractions, +-inf the ends"""
    if isinstance(val, float):
        if val == float("-inf"):
            return 0
        if val == float("inf"):
            return coord_size
        if 0 <= val <= 1:
            return int(coord_size * val)
        return int(val)
    return val


def reduce_factor_to_indices(factor, height):
    if factor <= 0:
        raise ValueError(f"factor == {factor} can't be negative")
    if height % factor != 0:
        raise ValueError(f"factor == {factor} must be a divisor of {height}")
    if factor == height:
        return [height // 2]
    return list(range(0, height, factor))


def validate_beam_indices(indices, height):
    if len(indices) == 0:
        raise ValueError("beam indices can't be empty")
    if len(set(indices)) != len(indices):
        raise ValueError("beam indices can't contain duplicates")
    bad = [i for i in indices if i < 0 or i >= height]
    if bad:
        raise ValueError(f"beam indices {bad} must be in the range [0, {height})")


def select_rows(img, indices):
    validate_beam_indices(list(indices), np.asarray(img).shape[-2] if np.asarray(img).ndim >= 2 else 0)
    return np.ascontiguousarray(np.asarray(img)[..., list(indices), :])
