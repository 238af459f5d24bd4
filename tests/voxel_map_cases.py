"""Inputs of the voxel map tests (tests/test_voxel_map_cases_cpu.py asserts each one's precondition on tests/voxel_map_model.py;
tests/test_voxel_map_api_cpu.py and tests/test_gpu_voxel_map.py run them through the C ABI), CapiMap -- the C ABI behind the
model's method names, with guard rows behind every output -- and the script runner both sides go through."""
import ctypes as C
import math

import numpy as np

import voxel_map_model as M

F32, F64 = 9, 10   # OUSTER_HIP_F32 / OUSTER_HIP_F64 (include/ouster_hip.h)
GUARD = 3         # rows before and behind every output that must keep their sentinel
SENTINEL = -12345.678


def next_down(x):
    return float(np.nextafter(x, -np.inf))


def next_up(x):
    return float(np.nextafter(x, np.inf))


# ---- admission
def admission_boundary(max_points):
    """-> (held, at, nearer): rows in voxel (0, 0, 0) of a voxel-8.0 map; dist_sq(held, at) >= res_sq > dist_sq(held, nearer),
    with `at` the nearest representable offset that is not closer than the resolution"""
    voxel = 8.0
    res_sq = voxel * voxel / float(max_points)
    r = math.sqrt(res_sq)
    lo = r
    while lo * lo >= res_sq:
        lo = next_down(lo)
    hi = next_up(lo)
    held = (0.0, 0.5, 0.5)   # dx = offset - 0.0 is the offset itself: no rounding in the subtraction
    if max_points == 1:      # the resolution is the voxel's edge: no offset along an axis reaches it, and the voxel is full anyway
        hi = 4.0
        lo = next_down(hi)
    return voxel, res_sq, held, (hi, 0.5, 0.5), (lo, 0.5, 0.5)


def distant_in_one_voxel(count, voxel=100.0):
    """`count` <= 64 points of one voxel on a lattice of pitch voxel / 4: every pair is voxel^2 / 16 or more apart, which is no
    closer than map_resolution_sq for max_points_per_voxel >= 16"""
    pts = [(voxel * (0.1 + 0.25 * i), voxel * (0.1 + 0.25 * j), voxel * (0.1 + 0.25 * k)) for i in range(4) for j in range(4) for k in range(4)]
    assert count <= len(pts)
    return np.array(pts[:count])


def uniform_cloud(n, seed, extent=5.0):
    return np.random.default_rng(seed).uniform(-extent, extent, (n, 3))


def one_voxel_candidates(n, seed):
    """n candidates of voxel (0, 0, 0) of a voxel-1.0 map"""
    return np.random.default_rng(seed).uniform(0.001, 0.999, (n, 3))


def distinct_voxels(n, start=0):
    """n rows, one voxel each (voxel 1.0), on a line through negative and positive cells"""
    i = np.arange(start, start + n, dtype=np.float64)
    return np.stack([i - n // 2 + 0.5, (i % 7) + 0.25, -(i % 3) - 0.75], axis=1)


def cells_starting_at(slot, mask, count, avoid=()):
    """`count` distinct cells whose probe starts at `slot` of a table of mask + 1 slots: a chain that runs on past that slot"""
    out, x = [], 0
    while len(out) < count:
        cell = (x, x // 5 - 3, -x)
        if (M.voxel_hash(cell) & mask) == slot and cell not in avoid:
            out.append(cell)
        x += 1
    return out


# ---- removal
def removal_boundary():
    """voxel 1.0, max_distance 3.0: max_voxel_dist 4.  Origin cell (0, 0, 0); a voxel at cell (4, 0, 0) is removed (16 >= 16), one
    at (3, 2, 1) kept (14 < 16), one at (2, 2, 2) kept (12), one at (0, -4, 0) removed, one at (-3, -2, -2) removed (17)"""
    cells = [(4, 0, 0), (3, 2, 1), (2, 2, 2), (0, -4, 0), (-3, -2, -2), (0, 0, 0)]
    rows = np.array([[c[0] + 0.5, c[1] + 0.5, c[2] + 0.5] for c in cells])
    rows = np.vstack([rows, rows + 0.3])   # two points per voxel (further apart than sqrt(1 / 20))
    return 1.0, 3.0, rows, (0.5, 0.5, 0.5), cells


# ---- queries
def lattice_ties():
    """voxel 1.0, P 1: the 8 corners of a cube of edge 1 around (0, 0, 0) -- one point per voxel at (+-0.5, +-0.5, +-0.5).  Queries:
    the centre (8 equal distances), an edge midpoint (4), a face centre... each distance exactly equal, so the order decides"""
    pts = np.array([[sx * 0.5, sy * 0.5, sz * 0.5] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    queries = np.array([[0.0, 0.0, 0.0],      # 8 ties; the query's own cell (0, 0, 0) holds (0.5, 0.5, 0.5)
                        [0.0, 0.0, 0.5],      # 4 ties among z = +0.5
                        [0.0, 0.5, 0.5],      # 2 ties
                        [-0.25, 0.0, 0.0],    # 4 ties among x = -0.5, and the query's own cell is (-1, 0, 0)
                        [0.0, -0.25, -0.5]])  # 2 ties
    return pts, queries


def face_edge_corner_queries():
    """queries exactly on the faces, edges and corners of voxels (voxel 0.5), around a cloud"""
    q = []
    for x in (-1.0, -0.5, 0.0, 0.5, 1.0):
        q += [[x, 0.123, -0.377], [x, 0.5, -0.377], [x, 0.5, -0.5], [0.123, x, 1.0], [x, x, x]]
    return np.array(q)


# ---- the C ABI behind the model's names
class CapiMap:
    """ouster_hip_voxel_map_* with arrays in host memory (the _host forms), or -- with to_device / from_device -- in device memory"""

    def __init__(self, capi, ctx, voxel_size, max_distance=100.0, max_points_per_voxel=20, min_pts_threshold=1, num_attributes=0,
                 host=False, to_device=None, from_device=None, dtype=F64, stride=3):
        self.capi, self.L = capi, capi.load_hip()
        self.to_device, self.from_device = to_device, from_device
        self.dtype, self.stride = dtype, stride
        d = capi.VoxelMapDesc(voxel_size, max_distance, max_points_per_voxel, min_pts_threshold, num_attributes,
                              capi.VOXEL_MAP_HOST if host else 0, 0)
        h = C.c_void_p()
        capi.check(self.L.ouster_hip_voxel_map_create(None if host else ctx, C.byref(d), C.byref(h)))
        self.h = h
        self.keep = []

    def close(self):
        if self.h:
            self.L.ouster_hip_voxel_map_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _fn(self, name):
        return getattr(self.L, "ouster_hip_voxel_map_" + name + ("" if self.to_device else "_host"))

    def _rows(self, rows):
        """-> (pointer, n, holder): the rows as [n][stride] of the map's dtype"""
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
        a = np.full((len(rows), self.stride), 7.5, dtype=np.float32 if self.dtype == F32 else np.float64)
        a[:, :3] = rows
        if self.to_device:
            t = self.to_device(a)
            return C.c_void_p(t.data_ptr() if len(a) else 0), len(a), t
        return C.c_void_p(a.ctypes.data if len(a) else 0), len(a), a

    def _out(self, rows, cols):
        """room for `rows` rows with GUARD rows of sentinels before and behind -> (pointer to the first row, holder)"""
        a = np.full((rows + 2 * GUARD, cols), SENTINEL)
        if self.to_device:
            t = self.to_device(a)
            return C.c_void_p(t.data_ptr() + GUARD * cols * 8), t
        return C.c_void_p(a.ctypes.data + GUARD * cols * 8), a

    def _back(self, holder, rows, what):
        a = self.from_device(holder) if self.to_device else holder
        assert (a[:GUARD] == SENTINEL).all() and (a[GUARD + rows:] == SENTINEL).all(), "%s: written outside its %d rows" % (what, rows)
        return a[GUARD:GUARD + rows].copy()

    @staticmethod
    def _point(p):
        return (C.c_double * 3)(*[float(c) for c in p])

    def widened(self, rows):
        """what the map sees of `rows`: through float32 where that is the dtype"""
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
        return rows.astype(np.float32).astype(np.float64) if self.dtype == F32 else rows

    def add_points(self, rows):
        p, n, hold = self._rows(rows)
        self.capi.check(self._fn("add_points")(self.h, p, self.dtype, n, self.stride))

    def update(self, rows, position):
        p, n, hold = self._rows(rows)
        self.capi.check(self._fn("update")(self.h, p, self.dtype, n, self.stride, self._point(position)))

    def remove_voxels_far_from_location(self, origin):
        self.capi.check(self.L.ouster_hip_voxel_map_remove_far(self.h, self._point(origin)))

    def extract_voxels_far_from_location(self, origin, capacity=None):
        cap = self.info()["points"] if capacity is None else capacity
        p, hold = self._out(cap, 3)
        n = C.c_uint64(0)
        rc = self._fn("extract_far")(self.h, self._point(origin), p, cap, C.byref(n))
        self.last_n = int(n.value)
        if rc != 0:
            assert (self._back(hold, 0, "extract (refused)").size == 0)
        self.capi.check(rc)
        return self._back(hold, self.last_n, "extract")

    def pointcloud(self, capacity=None):
        cap = self.info()["points"] if capacity is None else capacity
        p, hold = self._out(cap, 3)
        n = C.c_uint64(0)
        rc = self._fn("pointcloud")(self.h, p, cap, C.byref(n))
        self.last_n = int(n.value)
        if rc != 0:
            assert (self._back(hold, 0, "pointcloud (refused)").size == 0)
        self.capi.check(rc)
        return self._back(hold, self.last_n, "pointcloud")

    def get_closest_neighbors(self, queries, max_distance_sq=M.DBL_MAX):
        p, n, hold = self._rows(queries)
        op, oh = self._out(n, 3)
        dp, dh = self._out(n, 1)
        self.capi.check(self._fn("closest")(self.h, p, self.dtype, n, self.stride, max_distance_sq, op, dp))
        return self._back(oh, n, "closest points"), self._back(dh, n, "closest distances")[:, 0]

    def get_closest_neighbor(self, query, max_distance_sq=M.DBL_MAX):
        pts, d2 = self.get_closest_neighbors([query], max_distance_sq)
        return tuple(pts[0]), float(d2[0])

    def info(self):
        i = self.capi.VoxelMapInfo()
        self.capi.check(self.L.ouster_hip_voxel_map_info_read(self.h, C.byref(i)))
        return {n: int(getattr(i, n)) for n, _ in self.capi.VoxelMapInfo._fields_}

    def reserve(self, voxels):
        self.capi.check(self.L.ouster_hip_voxel_map_reserve(self.h, voxels))

    def clear(self):
        self.capi.check(self.L.ouster_hip_voxel_map_clear(self.h))

    def empty(self):
        return self.info()["voxels"] == 0

    def num_voxels(self):
        return self.info()["voxels"]

    def num_points(self):
        return self.info()["points"]


def same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got.view(np.uint64) != want.view(np.uint64)).reshape(len(got), -1).any(axis=1))[0]   # -0.0 and NaN count
        raise AssertionError("%s: %d of %d rows differ, first %d: %r != %r" % (what, len(bad), len(got), bad[0], got[bad[0]], want[bad[0]]))


def run_script(m, script):
    """every operation of `script` on m (the model or a CapiMap); -> what each one returned, as arrays"""
    out = []
    for op in script:
        name, args = op[0], op[1:]
        if name == "add":
            m.add_points(*args)
        elif name == "update":
            m.update(*args)
        elif name == "remove":
            m.remove_voxels_far_from_location(*args)
        elif name == "extract":
            out.append(("extract", np.asarray(m.extract_voxels_far_from_location(*args))))
        elif name == "clear":
            m.clear()
        elif name == "cloud":
            out.append(("cloud", np.asarray(m.pointcloud())))
        elif name == "closest":
            pts, d2 = m.get_closest_neighbors(*args)
            out.append(("closest points", np.asarray(pts)))
            out.append(("closest distances", np.asarray(d2)))
        elif name == "counts":
            out.append(("counts", np.array([m.num_voxels(), m.num_points(), int(m.empty())], dtype=np.float64)))
        else:
            raise ValueError(name)
    return out


def check_script(got_map, model, script, what=""):
    got, want = run_script(got_map, script), run_script(model, script)
    assert len(got) == len(want)
    for k, ((name, g), (_, w)) in enumerate(zip(got, want)):
        same_bytes(g.reshape(w.shape) if g.size == w.size else g, w, "%s step %d (%s)" % (what, k, name))


def moving_script(seed, calls=6, n=600, extent=6.0, step=1.5):
    """a map that follows a moving position: update, query, extract, add, clear in turn"""
    rng = np.random.default_rng(seed)
    script, pos = [], np.zeros(3)
    for k in range(calls):
        rows = pos + rng.uniform(-extent, extent, (n, 3))
        script.append(("update", rows, tuple(pos)))
        script.append(("counts",))
        script.append(("closest", pos + rng.uniform(-extent, extent, (97, 3)), 4.0 if k % 2 else M.DBL_MAX))
        if k == 3:
            script.append(("extract", tuple(pos + np.array([2.0 * extent, 0, 0]))))
            script.append(("cloud",))
        pos = pos + np.array([step, -0.5 * step, 0.25 * step])
    script += [("cloud",), ("add", np.zeros((0, 3))), ("remove", tuple(pos)), ("cloud",), ("clear",), ("counts",), ("cloud",),
               ("add", rng.uniform(-1, 1, (50, 3))), ("cloud",), ("counts",)]
    return script
