"""The yardstick of the resident voxel map: the reference's core::VoxelHashMap3d (ouster_core/include/ouster/core/voxel_hash_map.h,
ouster_core/src/voxel_hash_map.cpp; Vector3i / Vector3d / DefaultVoxelBucket / first_n_point) restated statement for statement in
Python floats and ints: every multiply, add and subtract is one IEEE double operation.

What is ours and not the reference's:
  * the row order of pointcloud() and extract_voxels_far_from_location(): voxels in creation order (earlier calls first, first-seen
    input order within a call), a voxel's points in admission order, survivors of a removal in their old relative order.  The
    reference emits its robin-hood map's iteration order;
  * a squared distance is ((dx dx + dy dy) + dz dz), the project's fixed rounding order; Eigen's squaredNorm leaves it open;
  * what is undefined there is refused or defined here: a non-finite voxel_size / max_distance, ceil(max_distance / voxel_size) + 1
    above int32, a point or origin outside the int32 voxel grid (the whole call is refused and the map is unchanged), a
    neighbour cell outside int32 (skipped), a query outside the grid (no neighbour); the cell distance of a removal is exact
    (64-bit on the device), equal to the reference wherever its 32-bit arithmetic does not overflow;
  * update() checks its position before it adds anything: a refused call leaves the map unchanged."""
import math

import numpy as np

MSG_MAX_POINTS = "max_points_per_voxel must be greater than 0"
MSG_VOXEL_SIZE = "voxel_size must be greater than 0"
MSG_MAX_DISTANCE = "max_distance must be greater than 0"
MSG_ATTRIBUTES = "num_attributes must be 0 for a fixed-size PointType"
MSG_RANGE = "voxel map: max_distance / voxel_size exceeds the int32 voxel grid"
MSG_GRID = "voxel map: point outside the int32 voxel grid"

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
DBL_MAX = float(np.finfo(np.float64).max)

# voxel_hash_map.cpp:158-166
VOXEL_SHIFTS = (
    (0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 0), (1, -1, 0), (-1, 1, 0), (-1, -1, 0),
    (1, 0, 1), (1, 0, -1), (-1, 0, 1), (-1, 0, -1), (0, 1, 1), (0, 1, -1), (0, -1, 1), (0, -1, -1), (1, 1, 1), (1, 1, -1), (1, -1, 1),
    (1, -1, -1), (-1, 1, 1), (-1, 1, -1), (-1, -1, 1), (-1, -1, -1))


def axis_to_voxel(p, inv):
    """int(floor(p * inv)), or None where no int32 holds it (NaN and the infinities included)"""
    f = float(p) * inv
    if not math.isfinite(f):
        return None
    i = math.floor(f)
    if i < INT32_MIN or i > INT32_MAX:
        return None
    return int(i)


def point_to_voxel(p, inv):
    """VoxelHashMap::point_to_voxel(point, inv_voxel_size); None outside the grid"""
    v = tuple(axis_to_voxel(p[k], inv) for k in range(3))
    return None if None in v else v


def dist_sq(a, b):
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return (dx * dx + dy * dy) + dz * dz


class VoxelHashMap3d:
    def __init__(self, voxel_size, max_distance=100.0, max_points_per_voxel=20, min_pts_threshold=1, num_attributes=0):
        if max_points_per_voxel == 0:
            raise ValueError(MSG_MAX_POINTS)
        if not (voxel_size > 0.0) or not math.isfinite(voxel_size):
            raise ValueError(MSG_VOXEL_SIZE)
        if not (max_distance > 0.0) or not math.isfinite(max_distance):
            raise ValueError(MSG_MAX_DISTANCE)
        if num_attributes != 0:
            raise ValueError(MSG_ATTRIBUTES)
        self.voxel_size = float(voxel_size)
        self.max_distance = float(max_distance)
        self.max_points_per_voxel = int(max_points_per_voxel)
        self.min_pts_threshold = int(min_pts_threshold)   # no effect with this bucket type
        self.map_resolution_sq = self.voxel_size * self.voxel_size / float(self.max_points_per_voxel)
        self.inv = 1.0 / self.voxel_size
        reach = self.max_distance * self.inv
        if not math.isfinite(reach) or math.ceil(reach) + 1 > INT32_MAX:
            raise ValueError(MSG_RANGE)
        self.max_voxel_dist = int(math.ceil(reach)) + 1
        self.cells = []     # creation order
        self.buckets = []   # per voxel: its points (x, y, z) in admission order
        self.index = {}

    # ---- admission
    def add_points(self, rows):
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
        pts = [tuple(float(c) for c in r) for r in rows]
        cells = [point_to_voxel(p, self.inv) for p in pts]
        if None in cells:
            raise ValueError(MSG_GRID)
        for p, cell in zip(pts, cells):
            v = self.index.get(cell)
            if v is None:
                v = self.index[cell] = len(self.cells)
                self.cells.append(cell)
                self.buckets.append([])
            bucket = self.buckets[v]
            if len(bucket) == self.max_points_per_voxel or any(dist_sq(q, p) < self.map_resolution_sq for q in bucket):
                continue
            bucket.append(p)

    def rejected_by(self, p):
        """why add_points would turn p away now: None (admitted), "capacity" or "distance" """
        p = tuple(float(c) for c in p)
        bucket = self.buckets[self.index[point_to_voxel(p, self.inv)]] if point_to_voxel(p, self.inv) in self.index else []
        if len(bucket) == self.max_points_per_voxel:
            return "capacity"
        return "distance" if any(dist_sq(q, p) < self.map_resolution_sq for q in bucket) else None

    # ---- eviction
    def _origin(self, origin):
        cell = point_to_voxel([float(c) for c in origin], self.inv)
        if cell is None:
            raise ValueError(MSG_GRID)
        return cell

    def is_far(self, cell, origin_cell):
        d = [cell[k] - origin_cell[k] for k in range(3)]
        return d[0] * d[0] + d[1] * d[1] + d[2] * d[2] >= self.max_voxel_dist * self.max_voxel_dist

    def extract_voxels_far_from_location(self, origin):
        o = self._origin(origin)
        far = [self.is_far(c, o) for c in self.cells]
        evicted = [p for v, b in enumerate(self.buckets) if far[v] for p in b]
        self.cells = [c for v, c in enumerate(self.cells) if not far[v]]
        self.buckets = [b for v, b in enumerate(self.buckets) if not far[v]]
        self.index = {c: v for v, c in enumerate(self.cells)}
        return np.array(evicted, dtype=np.float64).reshape(-1, 3)

    def remove_voxels_far_from_location(self, origin):
        self.extract_voxels_far_from_location(origin)

    def update(self, rows, position):
        self._origin(position)
        self.add_points(rows)
        self.remove_voxels_far_from_location(position)

    # ---- reading
    def empty(self):
        return not self.cells

    def clear(self):
        self.cells, self.buckets, self.index = [], [], {}

    def pointcloud(self):
        return np.array([p for b in self.buckets for p in b], dtype=np.float64).reshape(-1, 3)

    def num_voxels(self):
        return len(self.cells)

    def num_points(self):
        return sum(len(b) for b in self.buckets)

    def get_closest_neighbor(self, query, max_distance_sq=DBL_MAX):
        """voxel_hash_map.cpp:170-215.  -> ((x, y, z), distance_sq); no neighbour: ((0, 0, 0), max_distance_sq)"""
        q = tuple(float(c) for c in query)
        best, best_sq = (0.0, 0.0, 0.0), float(max_distance_sq)
        voxel = point_to_voxel(q, self.inv)
        if voxel is None:
            return best, best_sq
        for shift in VOXEL_SHIFTS:
            cell = tuple(voxel[k] + shift[k] for k in range(3))
            if min(cell) < INT32_MIN or max(cell) > INT32_MAX:
                continue
            lb_sq = 0.0
            for d in range(3):
                lo = float(cell[d]) * self.voxel_size
                hi = lo + self.voxel_size
                if q[d] < lo:
                    delta = lo - q[d]
                    lb_sq = lb_sq + delta * delta
                elif q[d] > hi:
                    delta = q[d] - hi
                    lb_sq = lb_sq + delta * delta
            if lb_sq >= best_sq:
                continue
            v = self.index.get(cell)
            if v is None:
                continue
            for p in self.buckets[v]:
                d2 = dist_sq(p, q)
                if d2 < best_sq:
                    best, best_sq = p, d2
        return best, best_sq

    def get_closest_neighbors(self, queries, max_distance_sq=DBL_MAX):
        queries = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
        pts = np.zeros((len(queries), 3))
        d2 = np.zeros(len(queries))
        for i, q in enumerate(queries):
            p, d = self.get_closest_neighbor(q, max_distance_sq)
            pts[i], d2[i] = p, d
        return pts, d2


def voxel_hash(cell):
    """voxel_hash of csrc/voxel_dev.h: which slot of its table a cell starts probing at (tests that build long or wrapping chains)"""
    m = 0xFFFFFFFF
    h = ((cell[0] & m) * 73856093 & m) ^ ((cell[1] & m) * 19349669 & m) ^ ((cell[2] & m) * 83492791 & m)
    h ^= h >> 16
    h = h * 0x85ebca6b & m
    h ^= h >> 13
    h = h * 0xc2b2ae35 & m
    h ^= h >> 16
    return h
