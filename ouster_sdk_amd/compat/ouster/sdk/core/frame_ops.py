"""`ouster.sdk.core.frame_ops`: the reference's Python call shapes (python/src/ouster/sdk/core/frame_ops.py) over
ouster_sdk_amd.core.  Validation raises ValueError with the reference's messages and needs no GPU; the pixel work runs on
the GPU in place on the frame's storage (csrc/k_frame_ops.hip) and raises without one.

Two spellings of one error exist, as in the reference: clip / filter_field resolve their fields in C++ and name a non-pixel field
as `[NAME]`; filter_xyz resolves in Python and prints the list repr `['NAME']`.  mask's size message is the reference's with its
f-string mended (the reference prints the braces literally)."""
import math

import numpy as np

from ouster_sdk_amd import core as _core
from ouster_sdk_amd.core import clip, filter_field  # noqa: F401  (same call shapes as the reference's bindings)

_SECOND_RETURN_FIELDS = frozenset(("RANGE2", "SIGNAL2", "REFLECTIVITY2", "FLAGS2"))


def _pixel_fields(frame, filtered_fields):
    """Fields an op works on: pixel fields only.  A listed field the frame lacks is skipped; a listed field that is present
    but no pixel field is an error; no list means every pixel field present."""
    is_pixel = {ft.name: ft.field_class == _core.FieldClass.PIXEL_FIELD for ft in frame.field_types}
    names = list(frame.fields) if filtered_fields is None else [f for f in filtered_fields if frame.has_field(f)]
    rejected = [f for f in names if not is_pixel.get(f, False)]
    if filtered_fields is not None and rejected:
        raise ValueError(f"Only PIXEL_FIELD frame fields are supported here; requested non-pixel fields: {rejected}")
    return [f for f in names if is_pixel.get(f, False)]


def _index_bound(value, extent):
    """A float bound of filter_uv: -inf / +inf are the ends, a value in [0, 1] a fraction of the extent."""
    if not isinstance(value, float):
        return value
    if math.isinf(value):
        return 0 if value < 0 else extent
    return int(extent * value) if 0 <= value <= 1 else int(value)


def filter_uv(frame, coord_2d, lower, upper, invalid=0, filtered_fields=None):
    """Pixels of the rows ('u') or destaggered columns ('v') in [lower, upper) become `invalid`."""
    if coord_2d not in ("u", "v"):
        raise ValueError(f"coord_2d == {coord_2d} must be either 'u' or 'v'")
    extent = frame.h if coord_2d == "u" else frame.w
    lower, upper = _index_bound(lower, extent), _index_bound(upper, extent)
    if lower < 0 or upper > extent:
        raise ValueError(f"lower == {lower} and upper == {upper} must be in the range [0, {extent}]")
    if lower > upper:
        raise ValueError(f"lower == {lower} must be less than upper == {upper}")
    _core._frame_ops_filter_uv(frame, coord_2d, lower, upper, invalid, filtered_fields or [], filtered_fields is not None)


def filter_xyz(frame, xyzlut, axis_idx, lower=float("-inf"), upper=float("inf"), invalid=0, filtered_fields=None,
               dewarp_points=False):
    """Pixels whose X / Y / Z (axis_idx 0 / 1 / 2) lies inside [lower, upper] become `invalid`.  `xyzlut` is any callable from
    a range image to (h, w, 3) points; the masks are built from its output in numpy and applied on the GPU.  Second-return
    fields follow RANGE2's points where the frame has RANGE2, all others RANGE's; either falls back to the other."""
    if axis_idx < 0 or axis_idx > 2:
        raise ValueError(f"axis_idx == {axis_idx} must be in the range [0, 2]")
    keep = {}
    for name in ("RANGE", "RANGE2"):
        if not frame.has_field(name):
            continue
        pts = np.asarray(xyzlut(frame.field(name)))
        if dewarp_points:
            pts = np.asarray(_core.dewarp(pts.reshape(frame.h, frame.w, 3), frame.body_to_world))
        coord = pts.reshape(frame.h, frame.w, 3)[:, :, axis_idx]
        with np.errstate(invalid="ignore"):
            keep[name] = np.ascontiguousarray(~((coord >= lower) & (coord <= upper)), dtype=np.uint8)
    if not keep:
        return
    groups = {}
    for field in _pixel_fields(frame, filtered_fields):
        first, second = ("RANGE2", "RANGE") if field in _SECOND_RETURN_FIELDS else ("RANGE", "RANGE2")
        groups.setdefault(first if first in keep else second, []).append(field)
    for source, fields in groups.items():
        _apply_keep_mask(frame, fields, keep[source], invalid)


def _apply_keep_mask(frame, fields, keep, invalid):
    """the mask mode of the invalidate kernel, writing `invalid` instead of 0"""
    _core._frame_ops_mask(frame, fields, keep, invalid)


def mask(frame, fields, mask):
    """Pixels where mask == 0 become 0.  mask has shape (frame.h, frame.w)."""
    if mask.shape[0] != frame.h or mask.shape[1] != frame.w:
        raise ValueError(f"Used mask size {mask.shape} doesn't match frame size ({frame.h}, {frame.w})")
    _core._frame_ops_mask(frame, list(fields) if fields else [], np.ascontiguousarray(mask, dtype=np.uint8))


def _check_beam_indices(indices, height):
    if not indices:
        raise ValueError("beam indices can't be empty")
    if len(set(indices)) != len(indices):
        raise ValueError("beam indices can't contain duplicates")
    outside = [i for i in indices if not 0 <= i < height]
    if outside:
        raise ValueError(f"beam indices {outside} must be in the range [0, {height})")


def _check_factor(factor, height):
    if factor <= 0:
        raise ValueError(f"factor == {factor} can't be negative")
    if height % factor:
        raise ValueError(f"factor == {factor} must be a divisor of {height}")


def select_by_index_metadata(metadata, indices):
    """The SensorInfo of an arbitrary subset of beams."""
    _check_beam_indices(indices, metadata.h)
    return _core.select_by_index_metadata(metadata, indices)


def select_by_index(frame, indices, update_metadata=False):
    """A new frame with the given beam rows of every pixel field."""
    _check_beam_indices(indices, frame.h)
    return _core.select_by_index(frame, indices, update_metadata)


def reduce_by_factor_metadata(metadata, factor):
    _check_factor(factor, metadata.h)
    return _core.reduce_by_factor_metadata(metadata, factor)


def reduce_by_factor(frame, factor, update_metadata=False):
    """Every factor-th beam row (the middle row alone when factor == frame.h)."""
    _check_factor(factor, frame.h)
    return _core.reduce_by_factor(frame, factor, update_metadata)
