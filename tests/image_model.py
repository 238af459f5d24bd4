"""Plain-numpy model of ouster::sdk::core::image::AutoExposure and BeamUniformityCorrector (single-channel overloads), written
from the description of their semantics, not from the product: exact order statistics through np.partition, every arithmetic
step a separately rounded operation in the image's dtype, the carried state in float64.  No product import."""
import numpy as np

AE_STRIDE = 4
AE_MIN_NONZERO_POINTS = 100
BUC_DAMPING = 0.92
BUC_UPDATE_EVERY = 8


def kth(values, k):
    """k-th smallest (0-based) of a 1-D array: what nth_element leaves at position k."""
    return np.partition(values, k)[k]


class AutoExposureModel:
    def __init__(self, lo_percentile=0.1, hi_percentile=0.1, update_every=3, damping=0.9):
        self.lo_percentile, self.hi_percentile = float(lo_percentile), float(hi_percentile)
        self.update_every, self.damping = int(update_every), float(damping)
        self.lo_state = self.hi_state = self.lo = self.hi = -1.0
        self.initialized = False
        self.counter = 0
        self.branches = []   # per call: "early", "uninit", "inf", "affine" or "hi"

    def update(self, image, update_state=True):
        T = image.dtype.type
        flat = image.reshape(-1)
        if self.counter == 0 and update_state:
            sample = flat[::AE_STRIDE]
            kept = sample[sample > 0]
            n = kept.size
            if n < AE_MIN_NONZERO_POINTS:
                self.branches.append("early")
                return
            k_lo = int(float(n) * self.lo_percentile)
            k_hi = n - int(float(n) * self.hi_percentile) - 1
            self.lo = float(kth(kept, k_lo))
            self.hi = float(kth(kept, k_hi))
            if not self.initialized:
                self.initialized = True
                self.lo_state, self.hi_state = self.lo, self.hi
        if not self.initialized:
            self.branches.append("uninit")
            return
        if update_state:
            self.lo_state = self.damping * self.lo_state + (1.0 - self.damping) * self.lo
            self.hi_state = self.damping * self.hi_state + (1.0 - self.damping) * self.hi
        with np.errstate(divide="ignore", invalid="ignore"):
            scale = np.float64(1.0 - (self.lo_percentile + self.hi_percentile)) / np.float64(self.hi_state - self.lo_state)
        with np.errstate(over="ignore", invalid="ignore"):
            if np.isinf(scale) or np.isnan(scale):
                self.branches.append("inf")
                flat[:] = flat * T(0.5 / self.hi_state)
            elif scale * (0.0 - self.lo_state) + self.lo_percentile <= 0.0:
                self.branches.append("affine")
                flat[:] = flat - T(self.lo_state)
                flat[:] = flat * T(scale)
                flat[:] = flat + T(self.lo_percentile)
            else:
                self.branches.append("hi")
                flat[:] = flat * T((1.0 - self.hi_percentile) / self.hi_state)
        flat[:] = np.where(flat < 0, T(0), flat)
        flat[:] = np.where(flat > 1, T(1), flat)
        if update_state:
            self.counter = (self.counter + 1) % self.update_every


def dark_row_medians(image):
    """(medians of the row differences over the non-empty columns [h - 1], n_cols)"""
    mask = (image != 0).any(axis=0)
    n_cols = int(mask.sum())
    h = image.shape[0]
    if n_cols == 0:
        return np.zeros(max(h - 1, 0), image.dtype), 0
    diffs = image[1:, mask] - image[:-1, mask]          # one rounding in T
    return np.array([kth(diffs[i], n_cols // 2) for i in range(h - 1)], image.dtype), n_cols


def compute_dark_count(image):
    T = image.dtype.type
    h = image.shape[0]
    med, n_cols = dark_row_medians(image)
    d = np.zeros(h, image.dtype)
    if n_cols == 0 or h < 2:
        return d
    for i in range(1, h):
        d[i] = d[i - 1] + med[i - 1]
    slope = d[h - 1] / T(h - 1)                          # the line through the first (0) and the last entry
    d = d - np.arange(h).astype(image.dtype) * slope
    return d - d.min()


class BeamUniformityModel:
    def __init__(self):
        self.counter = 0
        self.dark_count = np.zeros(0, np.float64)

    def update(self, image, update_state=True):
        h = image.shape[0]
        if self.dark_count.size != h:
            self.dark_count = compute_dark_count(image).astype(np.float64)
        elif update_state and self.counter == 0:
            new = compute_dark_count(image).astype(np.float64)
            self.dark_count = self.dark_count * BUC_DAMPING
            self.dark_count = self.dark_count + new * (1.0 - BUC_DAMPING)
        self.counter = (self.counter + 1) % BUC_UPDATE_EVERY
        x = image - self.dark_count.astype(image.dtype)[:, None]
        image[:] = np.where(x < 0, image.dtype.type(0), x)
