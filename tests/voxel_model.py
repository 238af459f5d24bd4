"""The yardstick of voxel down-sampling: the reference's core::voxel_downsample_3d / _xd (ouster_core/src/voxel_hash_map.cpp,
include/ouster/core/voxel_hash_map.h) and algorithm::voxel_downsample_with_normals (ouster_algorithm/src/voxel_downsample.cpp)
restated statement for statement in Python floats and ints: every multiply, add, divide and sqrt is one IEEE double operation.

One thing is ours: the order of the output rows.  The reference emits voxels in the iteration order of a robin-hood hash map;
here voxels come in first-seen order (by the input index of their first contributing point), and a voxel's points, where a
strategy keeps several, consecutively in admission order.  Compare with anything recorded from the reference through
sorted_rows()."""
import math

import numpy as np

FIRST_N_POINT, AVERAGE_POINT, RANDOM = 0, 1, 2
STRATEGIES = (FIRST_N_POINT, AVERAGE_POINT, RANDOM)

MSG_3D = "voxel_downsample_3d: frame must be Nx3"
MSG_XD = "voxel_downsample_xd: frame must be Nx>=3 (x,y,z + optional attributes)"
MSG_MAX_POINTS = "max_points_per_voxel must be greater than 0"
MSG_VOXEL_SIZE = "voxel_size must be greater than 0"
MSG_STRATEGY = "voxel_downsample: unknown strategy"
MSG_GRID = "voxel_downsample: point outside the int32 voxel grid"
MSG_WN_SHAPE = "voxel_downsample_with_normals expects Nx3 inputs"
MSG_WN_ROWS = "voxel_downsample_with_normals points/normals size mismatch"
MSG_WN_SIZE = "voxel_downsample_with_normals voxel_size must be > 0"

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def point_to_voxel(p, inv):
    """VoxelHashMap::point_to_voxel: one multiply, one floor, one conversion per axis.  The conversion of a value no int32
    holds is undefined in the reference; here it is refused (a documented deviation)."""
    v = []
    for k in range(3):
        f = float(p[k]) * inv
        if not math.isfinite(f):
            raise ValueError(MSG_GRID)
        i = int(math.floor(f))
        if i < INT32_MIN or i > INT32_MAX:
            raise ValueError(MSG_GRID)
        v.append(i)
    return tuple(v)


class Xorshift32:
    """random_selection_strategy::fast_rand, one state per call of voxel_downsample_*"""

    def __init__(self, seed=42):
        self.state = seed

    def __call__(self):
        s = self.state
        s ^= (s << 13) & 0xFFFFFFFF
        s ^= s >> 17
        s ^= (s << 5) & 0xFFFFFFFF
        self.state = s
        return s


def _downsample(frame, voxel_size, max_points_per_voxel, min_pts_threshold, strategy):
    """frame: (N, 3 + A) float64, N > 0; the VoxelHashMap constructor's checks, add_points, pointcloud()"""
    if strategy not in STRATEGIES:
        raise ValueError(MSG_STRATEGY)
    if not max_points_per_voxel > 0:
        raise ValueError(MSG_MAX_POINTS)
    if not (voxel_size > 0.0) or not math.isfinite(voxel_size):   # non-finite: ours, undefined in the reference
        raise ValueError(MSG_VOXEL_SIZE)
    n, cols = frame.shape
    inv = 1.0 / voxel_size
    resolution_sq = voxel_size * voxel_size / float(max_points_per_voxel)
    rand = Xorshift32()
    order = []          # voxels, first seen first
    buckets = {}
    for i in range(n):
        p = [float(x) for x in frame[i]]
        key = point_to_voxel(p, inv)
        b = buckets.get(key)
        if b is None:
            b = buckets[key] = {"sum": [0.0] * cols, "count": 0, "points": []}
            order.append(key)
        if strategy == AVERAGE_POINT:
            for c in range(cols):
                b["sum"][c] = b["sum"][c] + p[c]
            b["count"] += 1
        elif strategy == FIRST_N_POINT:
            if len(b["points"]) == max_points_per_voxel:
                continue
            if any(((q[0] - p[0]) * (q[0] - p[0]) + (q[1] - p[1]) * (q[1] - p[1])) + (q[2] - p[2]) * (q[2] - p[2]) < resolution_sq
                   for q in b["points"]):
                continue
            b["points"].append(p)
        else:
            if len(b["points"]) < max_points_per_voxel:
                b["points"].append(p)
            else:
                j = (rand() * max_points_per_voxel) >> 32
                b["points"][j] = p
    rows = []
    for key in order:
        b = buckets[key]
        if strategy == AVERAGE_POINT:
            if b["count"] >= min_pts_threshold:
                rows.append([s / float(b["count"]) for s in b["sum"]])
        else:
            rows.extend(b["points"])   # DefaultVoxelBucket does not look at min_pts_threshold
    return np.array(rows, np.float64).reshape(len(rows), cols)


def voxel_downsample_xd(frame, voxel_size, max_points_per_voxel=1, min_pts_threshold=1, strategy=RANDOM):
    frame = np.asarray(frame, np.float64)
    if frame.ndim != 2 or frame.shape[1] < 3:
        raise ValueError(MSG_XD)
    if frame.shape[0] == 0:
        return np.zeros((0, frame.shape[1]))
    return _downsample(frame, voxel_size, max_points_per_voxel, min_pts_threshold, strategy)


def voxel_downsample_3d(frame, voxel_size, max_points_per_voxel=1, min_pts_threshold=1, strategy=RANDOM):
    frame = np.asarray(frame, np.float64)
    if frame.ndim != 2 or frame.shape[1] != 3:
        raise ValueError(MSG_3D)
    if frame.shape[0] == 0:
        return np.zeros((0, 3))
    return _downsample(frame, voxel_size, max_points_per_voxel, min_pts_threshold, strategy)


def last_point_wins(frame, voxel_size):
    """what RANDOM with max_points_per_voxel == 1 comes to: (rand * 1) >> 32 is 0, every later point replaces the only slot"""
    frame = np.asarray(frame, np.float64)
    inv = 1.0 / voxel_size
    last, order = {}, []
    for i in range(frame.shape[0]):
        key = point_to_voxel(frame[i], inv)
        if key not in last:
            order.append(key)
        last[key] = i
    return frame[[last[k] for k in order]].reshape(len(order), frame.shape[1])


def voxel_downsample_with_normals(points, normals, voxel_size):
    points, normals = np.asarray(points, np.float64), np.asarray(normals, np.float64)
    if points.ndim != 2 or normals.ndim != 2 or points.shape[1] != 3 or normals.shape[1] != 3:
        raise ValueError(MSG_WN_SHAPE)
    if points.shape[0] != normals.shape[0]:
        raise ValueError(MSG_WN_ROWS)
    if not (voxel_size > 0.0) or not math.isfinite(voxel_size):
        raise ValueError(MSG_WN_SIZE)
    inv = 1.0 / voxel_size
    order, buckets = [], {}
    for i in range(points.shape[0]):
        p = [float(x) for x in points[i]]
        m = [float(x) for x in normals[i]]
        if not all(math.isfinite(x) for x in p) or not all(math.isfinite(x) for x in m):
            continue
        length = math.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
        if length <= 1e-12:
            continue
        m = [x / length for x in m]
        key = point_to_voxel(p, inv)
        b = buckets.get(key)
        if b is None:
            b = buckets[key] = {"p": [0.0] * 3, "n": [0.0] * 3, "count": 0}
            order.append(key)
        for c in range(3):
            b["p"][c] = b["p"][c] + p[c]
            b["n"][c] = b["n"][c] + m[c]
        b["count"] += 1
    out_p, out_n = [], []
    for key in order:
        b = buckets[key]
        s = b["n"]
        length = math.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
        if length <= 1e-12:
            continue
        out_p.append([x / float(b["count"]) for x in b["p"]])
        out_n.append([x / length for x in s])
    return np.array(out_p, np.float64).reshape(len(out_p), 3), np.array(out_n, np.float64).reshape(len(out_n), 3)


def sorted_rows(a):
    """rows in lexicographic order: the comparison with results recorded from the reference, whose row order is its hash map's"""
    a = np.asarray(a, np.float64)
    if a.shape[0] == 0:
        return a
    return a[np.lexsort(a.T[::-1])]


def same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))
    assert bad[0].size == 0, (what, "first difference at", [int(b[0]) for b in bad], got[tuple(b[0] for b in bad)],
                              want[tuple(b[0] for b in bad)])
