"""Pins the yardstick: tests/image_model.py against hand-computed cases and the properties a display image must have.
No product code is involved (CPU only)."""
import numpy as np
import pytest

from image_model import AutoExposureModel, BeamUniformityModel, compute_dark_count, dark_row_medians


def test_dark_count_of_a_4x8_image_by_hand():
    # columns 6 and 7 are empty (an azimuth window): n_cols = 6, the "median" is the 3rd smallest (0-based) of 6 differences
    img = np.array([[10, 10, 10, 10, 10, 10, 0, 0],
                    [12, 13, 11, 12, 14, 12, 0, 0],     # differences 2 3 1 2 4 2   -> sorted 1 2 2 2 3 4   -> 2
                    [17, 18, 16, 17, 20, 16, 0, 0],     # differences 5 5 5 5 6 4   -> sorted 4 5 5 5 5 6   -> 5
                    [16, 17, 15, 15, 20, 15, 0, 0]],    # differences -1 -1 -1 -2 0 -1 -> sorted -2 -1 -1 -1 -1 0 -> -1
                   np.float32)
    med, n_cols = dark_row_medians(img)
    assert n_cols == 6 and med.tolist() == [2.0, 5.0, -1.0]
    # running sum 0 2 7 6; the line through the first and last entry has slope 6 / 3 = 2 -> 0 0 3 0; minimum 0
    assert compute_dark_count(img).tolist() == [0.0, 0.0, 3.0, 0.0]
    m = BeamUniformityModel()
    out = img.copy()
    m.update(out)
    assert m.dark_count.tolist() == [0.0, 0.0, 3.0, 0.0]
    assert out[2].tolist() == [14, 15, 13, 14, 17, 13, 0, 0] and np.array_equal(out[[0, 1, 3]], img[[0, 1, 3]])
    assert compute_dark_count(np.zeros((4, 8), np.float64)).tolist() == [0.0] * 4      # no column at all


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_percentiles_of_a_100x8_ramp_by_hand(dtype):
    img = np.arange(1, 801, dtype=dtype).reshape(100, 8)
    m = AutoExposureModel()
    m.update(img)
    # every 4th element: 1, 5, 9, ... (n = 200); indices floor(200 * 0.1) = 20 and 200 - 20 - 1 = 179
    assert (m.lo, m.hi) == (1.0 + 4 * 20, 1.0 + 4 * 179) == (81.0, 717.0)
    assert m.lo_state == pytest.approx(81.0, rel=1e-14) and m.hi_state == pytest.approx(717.0, rel=1e-14)
    assert m.branches == ["affine"]      # 0.8 / 636 * -81 + 0.1 = -0.0019 <= 0: the affine map keeps 0 at or below 0
    assert img.min() == 0 and img.max() == 1.0 and img[0, 0] == 0
    assert img[50, 0] == pytest.approx((401 - 81) * 0.8 / 636 + 0.1, rel=1e-5)


def test_constant_image_takes_the_inf_branch_and_stays_constant():
    img = np.full((100, 8), 5.0, np.float32)
    m = AutoExposureModel()
    m.update(img)
    assert m.branches == ["inf"] and (m.lo, m.hi) == (5.0, 5.0)
    assert np.all(img == img[0, 0]) and img[0, 0] == pytest.approx(0.5, abs=1e-6)


def test_display_image_properties():
    rng = np.random.default_rng(1)
    img = rng.normal(100, 10, (64, 128)).astype(np.float32)
    img[5:9, 10:40] = 0                  # dropped pixels
    img[20, 20] = 1e6                    # outliers
    img[21, 21] = 1e-3
    zeros = img == 0
    a, b = AutoExposureModel(), AutoExposureModel()
    out = img.copy()
    a.update(out)
    assert a.branches == ["affine"]
    assert out.min() >= 0 and out.max() <= 1 and out[20, 20] == 1 and out[21, 21] == 0
    assert np.all(out[zeros] == 0)
    # few positive samples: nothing happens, not even the counter
    c = AutoExposureModel()
    sparse = np.zeros((16, 16), np.float32)
    sparse[0, :40 // 4] = 3
    keep = sparse.copy()
    c.update(sparse)
    assert c.branches == ["early"] and np.array_equal(sparse, keep) and c.counter == 0 and not c.initialized
    # two objects with different histories map the same image differently
    b.update((img * 3).copy())
    x, y = img.copy(), img.copy()
    a.update(x, update_state=False)
    b.update(y, update_state=False)
    assert not np.array_equal(x, y)
    # update_state = False leaves the state alone
    s = (a.lo_state, a.hi_state, a.counter)
    a.update(img.copy(), update_state=False)
    assert s == (a.lo_state, a.hi_state, a.counter)


def test_beam_uniformity_state_machine():
    rng = np.random.default_rng(2)
    m = BeamUniformityModel()
    first = rng.normal(50, 5, (8, 64))
    m.update(first.copy(), update_state=False)       # computed on the first call whatever update_state says
    d0 = m.dark_count.copy()
    assert d0.size == 8 and d0.min() == 0 and m.counter == 1
    for _ in range(7):
        m.update(rng.normal(50, 5, (8, 64)))
    assert np.array_equal(m.dark_count, d0) and m.counter == 0     # smoothed only when the counter is back at 0
    m.update(rng.normal(50, 5, (8, 64)))
    assert not np.array_equal(m.dark_count, d0)
    m.update(rng.normal(50, 5, (5, 64)))             # a change of h starts over
    assert m.dark_count.size == 5
    out = rng.normal(50, 5, (5, 64))
    m.update(out)
    assert out.min() >= 0
