"""Hand-computed cases that pin tests/frame_ops_model.py (the yardstick of the GPU tests).  No GPU, no product code."""
import numpy as np
import pytest

import frame_ops_model as M

INF = float("inf")


def test_filter_field_invalidates_inside_the_range():
    key = np.array([[0, 5, 10, 11, 20]], dtype=np.uint32)
    m = M.key_invalidated(key, 5, 10)
    assert m.tolist() == [[False, True, True, False, False]]
    tgt = np.array([[7, 8, 9, 10, 11]], dtype=np.uint16)
    assert M.apply(tgt, m, 3).tolist() == [[7, 3, 3, 10, 11]]


def test_nan_is_replaced_by_clip_and_kept_as_key():
    img = np.array([[np.nan, 1.0, -1.0, 2.0]], dtype=np.float32)
    assert M.clip(img, 0.0, 1.5, 9).tolist() == [[9.0, 1.0, 9.0, 9.0]]
    assert M.key_invalidated(img, -INF, INF).tolist() == [[False, True, True, True]]


def test_infinite_bounds():
    img = np.array([[0, 1, 254, 255]], dtype=np.uint8)
    assert M.clip(img, -INF, INF, 7).tolist() == [[0, 1, 254, 255]]
    assert M.clip(img, 1, INF, 7).tolist() == [[7, 1, 254, 255]]
    assert M.clip(img, -INF, 254, 7).tolist() == [[0, 1, 254, 7]]
    f = np.array([[-INF, 0.0, INF]], dtype=np.float64)
    assert M.clip(f, -INF, INF, 1).tolist() == [[-INF, 0.0, INF]]
    assert M.clip(f, -1e300, 1e300, 1).tolist() == [[1.0, 0.0, 1.0]]


def test_u64_next_to_2_pow_53_the_double_conversion_decides():
    p = 2 ** 53
    # p + 1 is a tie between p and p + 2: round to nearest even gives p; p + 3 ties between p + 2 and p + 4: gives p + 4
    img = np.array([[p - 1, p, p + 1, p + 2, p + 3]], dtype=np.uint64)
    got = M.clip(img, 0.0, float(p), 0)
    assert got.tolist() == [[p - 1, p, p + 1, 0, 0]]   # p + 1 compares as p: kept, though its integer value is above the bound
    got = M.clip(img, float(p + 2), float(p + 2), 0)
    assert got.tolist() == [[0, 0, 0, p + 2, 0]]
    i = np.array([[-p - 1, -p]], dtype=np.int64)
    assert M.clip(i, float(-p), 0.0, 5).tolist() == [[-p - 1, -p]]


def test_filter_uv_v_on_3x8_with_wrap():
    shifts = [0, 3, -2]
    m = M.cols_invalidated(3, 8, shifts, 6, 8)
    # row 0: columns 6, 7.  row 1: (c + 3) mod 8 in {6, 7} -> c in {3, 4}.  row 2: (c - 2) mod 8 in {6, 7} -> c in {0, 1}
    want = np.zeros((3, 8), dtype=bool)
    want[0, [6, 7]] = True
    want[1, [3, 4]] = True
    want[2, [0, 1]] = True
    assert np.array_equal(m, want)
    m = M.cols_invalidated(3, 8, shifts, 0, 2)
    # row 1: (c + 3) mod 8 in {0, 1} -> c in {5, 6}; row 2: (c - 2) mod 8 in {0, 1} -> c in {2, 3}
    want = np.zeros((3, 8), dtype=bool)
    want[0, [0, 1]] = True
    want[1, [5, 6]] = True
    want[2, [2, 3]] = True
    assert np.array_equal(m, want)
    for lo, hi in [(0, 0), (0, 8), (6, 8), (0, 2), (3, 4), (5, 5)]:
        assert np.array_equal(M.cols_invalidated(3, 8, shifts, lo, hi), M.cols_invalidated_via_destagger(3, 8, shifts, lo, hi))
    big = [8 + 3, -8 - 2, 7]
    for lo, hi in [(1, 6), (7, 8)]:
        assert np.array_equal(M.cols_invalidated(3, 8, big, lo, hi), M.cols_invalidated_via_destagger(3, 8, big, lo, hi))


def test_destagger_direction():
    img = np.arange(8, dtype=np.uint16)[None, :]
    assert M.destagger(img, [3]).tolist() == [[5, 6, 7, 0, 1, 2, 3, 4]]   # destaggered[(c + 3) mod 8] = img[c]
    assert np.array_equal(M.destagger(M.destagger(img, [3]), [3], inverse=True), img)


def test_lower_equal_upper_is_a_noop_for_uv():
    assert not M.rows_invalidated(4, 5, 2, 2).any()
    assert not M.cols_invalidated(4, 5, [0, 1, 2, 3], 3, 3).any()
    assert M.rows_invalidated(4, 5, 1, 3)[:, 0].tolist() == [False, True, True, False]


def test_mask_zero_means_invalidate():
    m = np.array([[0, 1], [2, 0]], dtype=np.uint8)
    assert M.apply(np.full((2, 2), 9, np.int16), M.mask_invalidated(m), 0).tolist() == [[0, 9], [9, 0]]


def test_reduce_factor_to_indices():
    assert M.reduce_factor_to_indices(128, 128) == [64]
    assert M.reduce_factor_to_indices(4, 16) == [0, 4, 8, 12]
    assert M.reduce_factor_to_indices(1, 3) == [0, 1, 2]
    with pytest.raises(ValueError, match="factor == 0 can't be negative"):
        M.reduce_factor_to_indices(0, 16)
    with pytest.raises(ValueError, match="factor == 3 must be a divisor of 16"):
        M.reduce_factor_to_indices(3, 16)


def test_beam_index_validation_and_selection():
    with pytest.raises(ValueError, match="can't be empty"):
        M.validate_beam_indices([], 4)
    with pytest.raises(ValueError, match="duplicates"):
        M.validate_beam_indices([1, 1], 4)
    with pytest.raises(ValueError, match=r"beam indices \[4, 9\] must be in the range \[0, 4\)"):
        M.validate_beam_indices([0, 4, 9], 4)
    img = np.arange(12).reshape(4, 3)
    assert M.select_rows(img, [3, 0]).tolist() == [[9, 10, 11], [0, 1, 2]]


def test_filter_xyz_field_routing():
    assert M.xyz_source("RANGE", True, True) == "RANGE"
    assert M.xyz_source("SIGNAL2", True, True) == "RANGE2"
    assert M.xyz_source("FLAGS2", True, False) == "RANGE"
    assert M.xyz_source("REFLECTIVITY", False, True) == "RANGE2"
    assert M.xyz_source("NEAR_IR", True, True) == "RANGE"
    assert M.xyz_source("RANGE2", False, False) is None


def test_xyz_predicate():
    xyz = np.array([[0, 0, -1], [0, 0, 0.5], [0, 0, np.nan], [0, 0, 2]], dtype=np.float32)
    assert M.xyz_invalidated(xyz, 2, 0.0, 1.0, 2, 2).tolist() == [[False, True], [False, False]]


def test_invalid_truncates_toward_zero_and_must_fit():
    assert M.cast_invalid(-0.9, "uint8") == 0
    assert M.cast_invalid(255.9, "uint8") == 255
    assert M.cast_invalid(-128.9, "int8") == -128
    assert M.cast_invalid(2.5, "float32") == np.float32(2.5)
    for bad, dt in [(256, "uint8"), (-1, "uint16"), (float("nan"), "int32"), (2.0 ** 64, "uint64"), (2.0 ** 63, "int64"),
                    (1e39, "float32"), (INF, "uint32")]:
        with pytest.raises(ValueError):
            M.cast_invalid(bad, dt)
    assert np.isnan(M.cast_invalid(float("nan"), "float32"))
    assert M.cast_invalid(INF, "float32") == np.float32(INF)


def test_uv_bound_fractions():
    assert M.uv_bound(0.25, 128) == 32
    assert M.uv_bound(float("-inf"), 128) == 0
    assert M.uv_bound(float("inf"), 128) == 128
    assert M.uv_bound(17.0, 128) == 17
    assert M.uv_bound(5, 128) == 5
