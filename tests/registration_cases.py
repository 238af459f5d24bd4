"""Inputs of the registration tests (tests/test_gpu_registration.py, tests/test_registration_api_cpu.py) and what they rely on;
tests/test_registration_cases_cpu.py asserts the preconditions on the model alone.  Every coordinate of a special row is a multiple
of 1 / 8, so that its distances are exact."""
import ctypes as C
import functools
import math

import numpy as np

import registration_model as R
import voxel_map_model as M

F32, F64 = 9, 10   # OUSTER_HIP_F32 / OUSTER_HIP_F64 (tests/voxel_map_cases.py)

STEP_VOXEL, STEP_MAX_DISTANCE, STEP_KERNEL = 0.5, 0.5, 0.125
ROW_COUNTS = (1, 255, 256, 257, 1023, 1024, 1025, 2049, 4100)
# the estimate a step applies first where it applies one: a few centimetres, under a degree
STEP_ESTIMATE = R.se3_exp([0.03, -0.02, 0.01, 0.004, -0.006, 0.008])

# map points of the special rows, each group far from the cloud and from the other groups
AT_BOUND_POINT = (20.25, 20.25, 20.25)
TWO_POINTS = ((30.25, 30.25, 30.25), (30.75, 30.25, 30.25))
FOUR_POINTS = ((40.25, 40.25, 40.25), (40.75, 40.25, 40.25), (40.25, 40.75, 40.25), (40.75, 40.75, 40.25))
SPECIAL_ROWS = (
    ("at_bound", (20.75, 20.25, 20.25)),        # exactly max_distance from its only neighbour: no correspondence
    ("inside_bound", (20.625, 20.25, 20.25)),   # a step nearer: one
    ("tie_two", (30.5, 30.25, 30.25)),
    ("tie_four", (40.5, 40.5, 40.25)),
    ("nan", (float("nan"), 1.0, 1.0)),
    ("off_grid", (1e300, 1.0, 1.0)),
)


def step_map_points(seed=5):
    """a few hundred voxels: 700 points in an 8 x 8 x 2 box, then the special groups"""
    rng = np.random.default_rng(seed)
    cloud = rng.uniform([-4.0, -4.0, -1.0], [4.0, 4.0, 1.0], size=(700, 3))
    return np.vstack([cloud, [AT_BOUND_POINT], TWO_POINTS, FOUR_POINTS])


@functools.lru_cache(maxsize=None)
def step_model(max_points):
    m = M.VoxelHashMap3d(STEP_VOXEL, 100.0, max_points)
    m.add_points(step_map_points())
    return m


def step_rows(n, seed=None):
    """n rows near the map's cloud (most within reach of a point, some not); from 16 rows on the last six are SPECIAL_ROWS"""
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    pts = step_map_points()[:700]
    rows = pts[rng.integers(0, len(pts), size=n)] + rng.normal(scale=0.15, size=(n, 3))
    rows[3::10, 2] += 3.0                     # every tenth row above the cloud, out of every point's reach
    if n >= 16:
        rows[n - len(SPECIAL_ROWS):] = [p for _, p in SPECIAL_ROWS]
    return rows


def special_index(n, name):
    return n - len(SPECIAL_ROWS) + [k for k, _ in SPECIAL_ROWS].index(name)


def widened(rows, dtype):
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    with np.errstate(over="ignore"):         # the row off the grid is an infinity in float32
        return rows.astype(np.float32).astype(np.float64) if dtype == F32 else rows


def model_step(rows, dtype, estimate, max_points, max_distance=STEP_MAX_DISTANCE, kernel_scale=STEP_KERNEL, fold=R.left_fold,
               sums_override=None):
    """the model's pass over the rows as the map sees them -> (moved [n][3], pass dict)"""
    moved = [tuple(float(c) for c in p) for p in widened(rows, dtype)]
    p = R.one_pass(moved, estimate, step_model(max_points), max_distance, kernel_scale, fold, sums_override)
    return np.array(moved, dtype=np.float64).reshape(-1, 3), p


def sum_bound(n, term_rows):
    """per sum: (ceil(N / 1024) + 40) * 2^-53 * sum |t| -- the bound of tests/test_gpu_icp.py for the same tree"""
    a = np.abs(np.array(term_rows, dtype=np.float64).reshape(-1, R.N_SUMS))
    return (math.ceil(n / 1024) + 40) * 2.0 ** -53 * np.array([math.fsum(a[:, k]) for k in range(R.N_SUMS)])


def non_finite_rows(moved):
    """mask of the rows with a coordinate that is not finite (tests/test_registration_cases_cpu.py: only the nan and off_grid rows)"""
    return ~np.isfinite(np.asarray(moved, dtype=np.float64).reshape(-1, 3)).all(axis=1)


def same_bytes(got, want, what, nan_rows=None):
    """bit for bit.  nan_rows (a mask over the rows, for the moved rows only): the rows whose input is not finite, where a NaN equals
    a NaN -- IEEE 754 leaves the sign and payload of the NaN an invalid operation makes to the hardware (inf * 0 is a negative quiet
    NaN on x86 and a positive one on the GPU).  A NaN anywhere else is compared by its bytes like any value."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s vs %s %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    if nan_rows is not None:
        nan_rows = np.asarray(nan_rows, dtype=bool)
        assert (np.isnan(got) == np.isnan(want)).all(), what + ": NaNs in other places"
        got, want = got.copy(), want.copy()
        got[nan_rows] = np.where(np.isnan(got[nan_rows]), np.nan, got[nan_rows])
        want[nan_rows] = np.where(np.isnan(want[nan_rows]), np.nan, want[nan_rows])
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.view(np.uint8).reshape(-1) != want.view(np.uint8).reshape(-1))
        raise AssertionError("%s: differs from byte %d on (%d bytes differ)" % (what, bad[0], len(bad)))


# ---- the realistic pair
SCENE_VOXEL, SCENE_POINTS = 0.5, 20
SCENE_ROWS = 2400
SCENE_MOTION = [0.04, -0.03, 0.02, 0.006, -0.004, 0.01]   # (upsilon, omega): centimetres, 0.7 degrees
SCENE_NOISE = 0.01
SCENE_CONVERGENCE, SCENE_MAX_ITERATIONS = 1e-4, 50


def scene(seed, n=SCENE_ROWS):
    """a floor, two walls and clutter, sampled with `seed`"""
    rng = np.random.default_rng(seed)
    k = n // 8
    floor = np.column_stack([rng.uniform(-8, 8, 3 * k), rng.uniform(-8, 8, 3 * k), np.zeros(3 * k)])
    wall_x = np.column_stack([np.full(2 * k, 8.0), rng.uniform(-8, 8, 2 * k), rng.uniform(0, 3, 2 * k)])
    wall_y = np.column_stack([rng.uniform(-8, 8, 2 * k), np.full(2 * k, -8.0), rng.uniform(0, 3, 2 * k)])
    clutter = rng.uniform([-6, -6, 0], [6, 6, 2], size=(n - 7 * k, 3))
    return np.vstack([floor, wall_x, wall_y, clutter])


@functools.lru_cache(maxsize=None)
def scene_map_points():
    pts = scene(100)
    pts.setflags(write=False)
    return pts


def scene_model():
    m = M.VoxelHashMap3d(SCENE_VOXEL, 100.0, SCENE_POINTS)
    m.add_points(scene_map_points())
    return m


def scene_parameters():
    """max_distance = 3 sigma, kernel_scale = sigma / 3 with sigma of a fresh AdaptiveThreshold"""
    sigma = R.AdaptiveThreshold(100.0).compute_threshold()
    return 3.0 * sigma, sigma / 3.0


@functools.lru_cache(maxsize=None)
def scene_frame(seed):
    """the scene sampled anew with noise, seen from a sensor that moved by SCENE_MOTION: aligning it gives about that motion"""
    rng = np.random.default_rng(seed)
    pts = scene(200 + seed) + rng.normal(scale=SCENE_NOISE, size=(SCENE_ROWS, 3))
    inv = R.se3_exp([-c for c in SCENE_MOTION])
    frame = np.array([R.apply(inv, p) for p in pts])
    frame.setflags(write=False)
    return frame


@functools.lru_cache(maxsize=None)
def scene_run(seed, exact):
    """-> (pose, passes, count, converged, trace) of the model with left-fold (exact: math.fsum) sums"""
    trace = []
    max_distance, kernel_scale = scene_parameters()
    out = R.align(scene_frame(seed), scene_model(), SCENE_MAX_ITERATIONS, SCENE_CONVERGENCE, max_distance, kernel_scale,
                  math.fsum if exact else R.left_fold, trace)
    return out + (trace,)


def pose_difference(a, b):
    """the largest element difference of the two poses' matrices"""
    return float(np.abs(R.matrix(a) - R.matrix(b)).max())


# The largest pose_difference over seeds 1 - 5 between align(left fold) and align(fsum), measured on the model alone:
#   seed  passes  correspondences  difference
#   1     23      2380             8.74e-16
#   2     25      2387             2.43e-16
#   3     26      2392             1.11e-16
#   4     31      2391             7.77e-16
#   5     20      2377             9.71e-17
# (both folds take the same passes and pick the same correspondences in every pass, for every seed).
# tests/test_registration_cases_cpu.py asserts that seed 1 still gives its figure.
MEASURED_POSE_DIFFERENCE = 8.743006318923108e-16


# ---- the C ABI from Python
class Step:
    """ouster_hip_registration_step / _step_ref over numpy (host=True) or device arrays, with guard rows behind every output"""
    GUARD, SENTINEL = 4, -7.25

    def __init__(self, capi, to_device=None, from_device=None):
        self.capi, self.L = capi, capi.load_hip()
        self.to_device, self.from_device = to_device, from_device

    def _put(self, a):
        if self.to_device:
            t = self.to_device(a)
            return t, t.data_ptr()
        return a, a.ctypes.data

    def _get(self, holder):
        return self.from_device(holder) if self.to_device else holder

    def run(self, map_handle, rows, dtype=F64, stride=3, estimate=None, max_distance=STEP_MAX_DISTANCE, kernel_scale=STEP_KERNEL):
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
        n, G = len(rows), self.GUARD
        a = np.full((n, stride), 7.5, dtype=np.float32 if dtype == F32 else np.float64)
        with np.errstate(over="ignore"):
            a[:, :3] = rows
        src, src_p = self._put(a)
        outs = {}
        for name, cols, dt in (("moved", 3, np.float64), ("flags", 1, np.uint8), ("neighbours", 3, np.float64), ("dist_sq", 1, np.float64)):
            host = np.full((n + 2 * G, cols), 7 if dt == np.uint8 else self.SENTINEL, dtype=dt)
            outs[name] = self._put(host) + (cols, dt)
        io = self.capi.RegistrationStepIo()
        io.points, io.n, io.row_stride, io.dtype = src_p, n, stride, dtype
        io.has_estimate = estimate is not None
        io.estimate = (C.c_double * 7)(*(estimate if estimate is not None else R.IDENTITY))
        io.max_distance, io.kernel_scale = max_distance, kernel_scale
        for name, (_, p, cols, dt) in outs.items():
            setattr(io, name, p + G * cols * np.dtype(dt).itemsize)
        fn = self.L.ouster_hip_registration_step if self.to_device else self.L.ouster_hip_registration_step_ref
        self.capi.check(fn(map_handle, C.byref(io)))
        got = {}
        for name, (holder, _, cols, dt) in outs.items():
            h = self._get(holder)
            guard = 7 if dt == np.uint8 else self.SENTINEL
            assert (h[:G] == guard).all() and (h[G + n:] == guard).all(), "%s: written outside its %d rows" % (name, n)
            got[name] = h[G:G + n].copy()
        got["flags"], got["dist_sq"] = got["flags"][:, 0], got["dist_sq"][:, 0]
        got["sums"], got["count"] = np.array(io.sums[:]), int(io.count)
        got["dx"], got["next_estimate"] = list(io.dx[:]), tuple(io.next_estimate[:])
        del src
        return got


def check_step(got, moved, p, what, exact_sums, nan_rows=None):
    """a pass's outputs against the model's: rows, flags, neighbours, distances and the count bit for bit; the sums bit for bit
    (exact_sums: the left fold of the host form) or within sum_bound of math.fsum of the terms; dx and the estimate are solve6 and
    se3_exp of the pass's own sums"""
    n = len(moved)
    if nan_rows is None:      # the rows the model itself moves to something not finite: the nan and off_grid special rows, no others
        nan_rows = non_finite_rows(moved)
    same_bytes(got["moved"], moved, what + ": moved rows", nan_rows=nan_rows)
    assert np.isfinite(got["sums"]).all(), what + ": a sum is not finite"
    assert got["flags"].tolist() == [int(f) for f in p["flags"]], what + ": flags"
    same_bytes(got["neighbours"], np.array(p["neighbours"], dtype=np.float64).reshape(-1, 3), what + ": neighbours")
    same_bytes(got["dist_sq"], np.array(p["dist_sq"], dtype=np.float64), what + ": squared distances")
    assert got["count"] == p["count"], what + ": count"
    if exact_sums:
        same_bytes(got["sums"], np.array(p["sums"]), what + ": sums")
    else:
        exact = np.array([math.fsum(t[k] for t in p["terms"]) for k in range(R.N_SUMS)])
        err, bound = np.abs(got["sums"] - exact), sum_bound(n, p["terms"])
        print("%s: sums |error| / bound = %s" % (what, np.array2string(err / np.where(bound > 0, bound, 1.0), precision=3)))
        assert (err <= bound).all(), "%s: sums off by %s, bound %s" % (what, err, bound)
    jtj, jtr = R.system_of_sums(list(got["sums"]))
    dx = R.solve6(jtj, jtr)
    assert got["dx"] == dx, what + ": dx is not solve6 of the pass's own sums"
    assert got["next_estimate"] == R.se3_exp(dx), what + ": the estimate is not se3_exp(dx)"


def align_capi(capi, map_handle, rows, dtype=F64, stride=3, max_iterations=50, convergence=1e-4, max_distance=1.0, kernel_scale=0.1,
               pointer=None, host=True, flags=0):
    """ouster_hip_registration_align_host (host) / _align on `pointer` -> (pose 4x4, iterations, correspondences, converged)"""
    L = capi.load_hip()
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    a = np.full((len(rows), stride), 7.5, dtype=np.float32 if dtype == F32 else np.float64)
    a[:, :3] = rows
    d = capi.RegistrationDesc()
    d.max_iterations, d.flags, d.convergence_criterion, d.max_distance, d.kernel_scale = max_iterations, flags, convergence, max_distance, kernel_scale
    fn = L.ouster_hip_registration_align_host if host else L.ouster_hip_registration_align
    p = pointer if pointer is not None else (a.ctypes.data if len(a) else None)
    capi.check(fn(map_handle, p, dtype, len(rows), stride, C.byref(d)))
    return np.array(d.pose[:]).reshape(4, 4), int(d.iterations), int(d.correspondences), bool(d.converged)
