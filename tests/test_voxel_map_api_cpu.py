"""The public surface of the voxel map (ouster_hip_voxel_map_*, core::VoxelHashMap3d, ouster_sdk_amd.core.VoxelHashMap3d), checked
without a GPU: symbols and struct layout; a map made with OUSTER_HIP_VOXEL_MAP_HOST against tests/voxel_map_model.py, bit for bit,
over scripted sequences of every operation; every refusal through the C ABI (before a GPU is asked for: ctx is NULL throughout),
through Python and through C++ (tests/cpp/voxel_map_snippet.cpp); the plain C++ half under ASan / UBSan in a program of its own
(tests/cpp/voxel_map_ref_main.cpp)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cpp_tools
import voxel_map_cases as K
import voxel_map_model as M
from conftest import ROOT, has_gpu
from ouster_sdk_amd import _capi as capi

sys.path.insert(0, os.path.join(ROOT, "ouster_sdk_amd", "compat"))

INT_FUNCS = ["create", "clear", "reserve", "info_read", "add_points", "add_points_host", "remove_far", "extract_far", "extract_far_host",
             "update", "update_host", "pointcloud", "pointcloud_host", "closest", "closest_host"]
MSG_CAPACITY = "voxel map: out_capacity is too small"


def last_error():
    return capi.load_hip().ouster_hip_last_error().decode()


def host_map(*a, **kw):
    return K.CapiMap(capi, None, *a, host=True, **kw)


def test_symbols_are_declared_and_exported():
    L = capi.load_hip()
    header = open(os.path.join(ROOT, "include", "ouster_hip.h")).read()
    for name in INT_FUNCS:
        full = "ouster_hip_voxel_map_" + name
        assert full in capi.ABI_SYMBOLS and hasattr(L, full) and ("int " + full + "(") in header, full
    assert "void ouster_hip_voxel_map_destroy(ouster_hip_voxel_map* map);" in header and "ouster_hip_voxel_map_destroy" in capi.ABI_SYMBOLS
    assert C.sizeof(capi.VoxelMapDesc) == 2 * 8 + 3 * 8 + 2 * 4 and capi.VoxelMapDesc.flags.offset == 40
    assert C.sizeof(capi.VoxelMapInfo) == 5 * 8
    assert "#define OUSTER_HIP_VOXEL_MAP_HOST 1u" in header and capi.VOXEL_MAP_HOST == 1
    L.ouster_hip_voxel_map_destroy(None)       # a no-op


def test_create_refusals_in_order_before_the_gpu():
    """ctx is NULL and no host flag: a validation error must win over "ctx is NULL"; *out is NULL afterwards"""
    L = capi.load_hip()
    nan, inf = float("nan"), float("inf")
    cases = [(M.MSG_MAX_POINTS, (0.0, -1.0, 0, 1, 5)), (M.MSG_VOXEL_SIZE, (0.0, -1.0, 20, 1, 5)), (M.MSG_VOXEL_SIZE, (-1.0, 100.0, 20, 1, 0)),
             (M.MSG_VOXEL_SIZE, (nan, 100.0, 20, 1, 0)), (M.MSG_VOXEL_SIZE, (inf, 100.0, 20, 1, 0)), (M.MSG_MAX_DISTANCE, (1.0, 0.0, 20, 1, 5)),
             (M.MSG_MAX_DISTANCE, (1.0, nan, 20, 1, 0)), (M.MSG_MAX_DISTANCE, (1.0, inf, 20, 1, 0)), (M.MSG_ATTRIBUTES, (1.0, 100.0, 20, 1, 5)),
             (M.MSG_RANGE, (1.0, float(2 ** 31 - 1), 20, 1, 0)), (M.MSG_RANGE, (1e-300, 1e300, 20, 1, 0))]
    for message, args in cases:
        with pytest.raises(ValueError) as e:       # the model refuses the same, with the same words
            M.VoxelHashMap3d(*args)
        assert str(e.value) == message
        for flags in (0, capi.VOXEL_MAP_HOST, 2):
            d = capi.VoxelMapDesc(args[0], args[1], args[2], args[3], args[4], flags, 0)
            h = C.c_void_p(5)
            assert L.ouster_hip_voxel_map_create(None, C.byref(d), C.byref(h)) == capi.ERR_INVALID_ARGUMENT
            assert last_error() == message and h.value is None, (message, last_error())
    good = (1.0, 100.0, 20, 1, 0)
    h = C.c_void_p(5)
    assert L.ouster_hip_voxel_map_create(None, C.byref(capi.VoxelMapDesc(*good, 2, 0)), C.byref(h)) == capi.ERR_INVALID_ARGUMENT
    assert last_error() == "voxel map: unknown flags" and h.value is None
    assert L.ouster_hip_voxel_map_create(None, C.byref(capi.VoxelMapDesc(*good, 0, 0)), C.byref(h)) == capi.ERR_INVALID_ARGUMENT
    assert last_error() == "ctx is NULL" and h.value is None
    assert L.ouster_hip_voxel_map_create(None, None, C.byref(h)) == capi.ERR_INVALID_ARGUMENT and last_error() == "NULL argument"
    assert L.ouster_hip_voxel_map_create(None, C.byref(capi.VoxelMapDesc(*good, 1, 0)), None) == capi.ERR_INVALID_ARGUMENT
    with host_map(1.0, float(2 ** 31 - 2)) as m:      # the largest reach there is
        assert m.empty()


def test_call_refusals_leave_the_map_and_the_outputs_alone():
    L = capi.load_hip()
    with host_map(1.0, 3.0, 20) as m:
        rows = K.removal_boundary()[2]
        m.add_points(rows)
        before = m.pointcloud().tobytes()
        a = np.ascontiguousarray(rows)
        p, o = C.c_void_p(a.ctypes.data), (C.c_double * 3)(0.5, 0.5, 0.5)
        n = C.c_uint64(77)
        out = np.full((40, 3), K.SENTINEL)
        op = C.c_void_p(out.ctypes.data)
        for fn in (L.ouster_hip_voxel_map_add_points, L.ouster_hip_voxel_map_add_points_host):
            assert fn(None, p, K.F64, 12, 3) == capi.ERR_INVALID_ARGUMENT and last_error() == "map is NULL"
            assert fn(m.h, p, 3, 12, 3) == capi.ERR_INVALID_ARGUMENT and last_error() == "dtype must be F32 or F64"
            assert fn(m.h, p, K.F64, 12, 2) == capi.ERR_INVALID_ARGUMENT and last_error() == "row_stride is smaller than 3"
            assert fn(m.h, None, K.F64, 12, 3) == capi.ERR_INVALID_ARGUMENT and last_error() == "NULL pointer"
            assert fn(m.h, p, K.F64, (1 << 30) + 1, 3) == capi.ERR_UNSUPPORTED
            assert fn(m.h, None, K.F64, 0, 0) == capi.OK             # an empty call is a no-op
        for fn in (L.ouster_hip_voxel_map_update, L.ouster_hip_voxel_map_update_host):
            assert fn(m.h, p, K.F64, 12, 1, o) == capi.ERR_INVALID_ARGUMENT and last_error() == "row_stride is smaller than 3"
            assert fn(m.h, p, K.F64, 12, 3, None) == capi.ERR_INVALID_ARGUMENT and last_error() == "NULL argument"
            assert fn(m.h, p, K.F64, 12, 3, (C.c_double * 3)(float("nan"), 0, 0)) == capi.ERR_INVALID_ARGUMENT and last_error() == M.MSG_GRID
        assert L.ouster_hip_voxel_map_remove_far(m.h, (C.c_double * 3)(0, float("inf"), 0)) == capi.ERR_INVALID_ARGUMENT and last_error() == M.MSG_GRID
        assert L.ouster_hip_voxel_map_remove_far(m.h, (C.c_double * 3)(0, 0, 3e9)) == capi.ERR_INVALID_ARGUMENT and last_error() == M.MSG_GRID
        assert L.ouster_hip_voxel_map_remove_far(None, o) == capi.ERR_INVALID_ARGUMENT
        for fn in (L.ouster_hip_voxel_map_extract_far, L.ouster_hip_voxel_map_extract_far_host):
            assert fn(m.h, (C.c_double * 3)(-1e300, 0, 0), op, 40, C.byref(n)) == capi.ERR_INVALID_ARGUMENT and last_error() == M.MSG_GRID
            assert fn(m.h, o, op, 40, None) == capi.ERR_INVALID_ARGUMENT and last_error() == "NULL argument"
            assert fn(m.h, o, op, 5, C.byref(n)) == capi.ERR_INVALID_ARGUMENT and last_error() == MSG_CAPACITY and n.value == 6
        for fn in (L.ouster_hip_voxel_map_pointcloud, L.ouster_hip_voxel_map_pointcloud_host):
            assert fn(m.h, op, 11, C.byref(n)) == capi.ERR_INVALID_ARGUMENT and last_error() == MSG_CAPACITY and n.value == 12
            assert fn(m.h, None, 12, C.byref(n)) == capi.ERR_INVALID_ARGUMENT and last_error() == "NULL pointer"
        for fn in (L.ouster_hip_voxel_map_closest, L.ouster_hip_voxel_map_closest_host):
            assert fn(m.h, p, 0, 12, 3, 1.0, op, op) == capi.ERR_INVALID_ARGUMENT and last_error() == "dtype must be F32 or F64"
            assert fn(m.h, p, K.F64, 12, 3, 1.0, None, op) == capi.ERR_INVALID_ARGUMENT and last_error() == "NULL pointer"
            assert fn(m.h, p, K.F64, (1 << 30) + 1, 3, 1.0, op, op) == capi.ERR_UNSUPPORTED
            assert fn(m.h, None, K.F64, 0, 3, 1.0, None, None) == capi.OK
        assert (out == K.SENTINEL).all()
        bad = rows.copy()
        bad[7, 1] = float("nan")
        with pytest.raises(ValueError, match=M.MSG_GRID):
            m.add_points(bad)
        bad[7, 1] = -2.0 ** 31 - 1.0
        with pytest.raises(ValueError, match=M.MSG_GRID):
            m.update(bad, (0, 0, 0))
        assert m.pointcloud().tobytes() == before and m.info()["voxels"] == 6


@pytest.mark.parametrize("voxel_size, max_distance, max_points, seed", [(0.5, 4.0, 3, 5), (1.0, 100.0, 20, 6), (0.25, 2.0, 1, 7)])
def test_host_map_equals_the_model_over_scripts(voxel_size, max_distance, max_points, seed):
    with host_map(voxel_size, max_distance, max_points) as m:
        K.check_script(m, M.VoxelHashMap3d(voxel_size, max_distance, max_points), K.moving_script(seed), "host map")


@pytest.mark.parametrize("dtype, stride", [(K.F32, 5), (K.F64, 3), (K.F64, 4)])
def test_host_map_dtypes_and_strides(dtype, stride):
    with host_map(1.0, 100.0, 20, dtype=dtype, stride=stride) as m:
        model = M.VoxelHashMap3d(1.0, 100.0, 20)
        rows, queries = K.uniform_cloud(2000, 42), K.uniform_cloud(500, 43)
        script = [("add", m.widened(rows)), ("cloud",), ("closest", m.widened(queries), M.DBL_MAX), ("closest", m.widened(queries), 4.0)]
        got = K.run_script(m, [("add", rows), ("cloud",), ("closest", queries, M.DBL_MAX), ("closest", queries, 4.0)])
        want = K.run_script(model, script)
        for (name, g), (_, w) in zip(got, want):
            K.same_bytes(g, w, name)


def test_host_map_special_cases():
    for max_points in (1, 2, 20):
        voxel, res_sq, held, at, nearer = K.admission_boundary(max_points)
        with host_map(voxel, 100.0, max_points) as m:
            K.check_script(m, M.VoxelHashMap3d(voxel, 100.0, max_points), [("add", [held, nearer, at]), ("cloud",), ("counts",)], "boundary")
            assert m.num_points() == (1 if max_points == 1 else 2)
    voxel, max_distance, rows, origin, cells = K.removal_boundary()
    with host_map(voxel, max_distance) as m:
        K.check_script(m, M.VoxelHashMap3d(voxel, max_distance), [("add", rows), ("extract", origin), ("cloud",), ("counts",),
                                                                   ("add", rows[:3]), ("cloud",), ("remove", (1e6, 0, 0)), ("counts",)], "removal")
    pts, queries = K.lattice_ties()
    with host_map(1.0, 100.0, 1) as m:
        K.check_script(m, M.VoxelHashMap3d(1.0, 100.0, 1), [("add", pts), ("closest", queries, M.DBL_MAX), ("closest", queries, 0.75),
                                                            ("closest", queries, 0.5)], "ties")
    top = float(2 ** 31 - 1)
    with host_map(1.0) as m:
        edge = [("add", [(top + 0.5, 0.5, 0.5), (top - 0.5, 0.5, 0.5)]),
                ("closest", [(top + 0.25, 0.5, 0.5), (float("nan"), 0.5, 0.5), (top + 1.5, 0.5, 0.5), (-top - 1.5, 0, 0)], 7.0)]
        K.check_script(m, M.VoxelHashMap3d(1.0), edge, "grid edge")


def test_python_face_names_defaults_and_errors():
    import ouster.sdk.core as core
    from ouster_sdk_amd import core as amd
    assert core.VoxelHashMap3d is amd.VoxelHashMap3d
    for args, message in (((1.0, 100.0, 0), M.MSG_MAX_POINTS), ((0.0,), M.MSG_VOXEL_SIZE), ((1.0, -1.0), M.MSG_MAX_DISTANCE),
                          ((float("nan"),), M.MSG_VOXEL_SIZE), ((1.0, 3e9), M.MSG_RANGE)):
        for host in (False, True):           # refused before a GPU is asked for
            with pytest.raises(ValueError) as e:
                amd.VoxelHashMap3d(*args, host=host)
            assert str(e.value) == message
    m = amd.VoxelHashMap3d(0.5, 4.0, 3, host=True)
    assert m.empty and m.max_points_per_voxel == 3 and m.min_pts_threshold == 1 and m.device == -1 and m.num_points == 0
    assert amd.VoxelHashMap3d(host=True).max_points_per_voxel == 20          # the binding's defaults: 0.1, 100, 20, 1
    p, d = m.get_closest_neighbor(np.array([0.5, 0.5, 0.5]))
    assert p.tolist() == [0.0, 0.0, 0.0] and d == M.DBL_MAX
    for bad in (np.zeros((4, 2)), np.zeros(3), np.zeros((2, 3, 1))):
        with pytest.raises(ValueError, match="^add_points expects an Nx3 array$"):
            m.add_points(bad)
    for call in (m.remove_voxels_far_from_location, m.extract_voxels_far_from_location, m.get_closest_neighbor):
        for bad in (np.zeros(2), np.zeros(4), np.zeros((1, 3))):
            with pytest.raises(ValueError, match="^VoxelHashMap method expects a 3-element point$"):
                call(bad)
    with pytest.raises(ValueError, match=M.MSG_GRID):
        m.add_points(np.array([[0.0, float("inf"), 0.0]]))
    with pytest.raises(ValueError, match=M.MSG_GRID):
        m.remove_voxels_far_from_location(np.array([0.0, float("nan"), 0.0]))
    assert amd.VoxelHashMap3d.point_to_voxel(np.array([-0.5, 1.5, 2.0]), 2.0) == (-1, 3, 4)
    # the Python face over a script, against the model

    class Face:
        def __init__(self, m):
            self.m = m
            self.add_points, self.update, self.clear = m.add_points, m.update, m.clear
            self.pointcloud = m.point_cloud
            self.get_closest_neighbors = m.get_closest_neighbors

        def remove_voxels_far_from_location(self, o):
            self.m.remove_voxels_far_from_location(np.asarray(o, dtype=np.float64))

        def extract_voxels_far_from_location(self, o):
            return self.m.extract_voxels_far_from_location(np.asarray(o, dtype=np.float64))

        def update(self, rows, pos):
            self.m.update(rows, np.asarray(pos, dtype=np.float64))

        def num_voxels(self):
            return self.m.num_voxels

        def num_points(self):
            return self.m.num_points

        def empty(self):
            return self.m.empty

    K.check_script(Face(m), M.VoxelHashMap3d(0.5, 4.0, 3), K.moving_script(11, calls=4, n=300), "python face")
    m.add_points(K.uniform_cloud(200, 1))
    q = K.uniform_cloud(20, 2)
    pts, d2 = m.get_closest_neighbors(q, 2.0)
    for i in range(20):                                       # batched equals single
        p, d = m.get_closest_neighbor(q[i], 2.0)
        assert p.tobytes() == pts[i].tobytes() and d == d2[i]
    if not has_gpu():
        with pytest.raises(RuntimeError):                     # no quiet fall-back to the host map
            amd.VoxelHashMap3d(0.5)


def test_cpp_caller_compiles_links_and_runs():
    """tests/cpp/voxel_map_snippet.cpp, built by tests/cpp/Makefile with the flags of the other C++ callers (-Werror)"""
    p = cpp_tools.run("voxel_map_snippet", [], timeout=300)
    assert "validation ok" in p.stdout and "host map ok" in p.stdout, p.stdout
    assert p.stdout.splitlines()[-1].startswith("ok" if has_gpu() else "no-gpu"), p.stdout


def test_host_half_under_the_sanitizers():
    """tests/cpp/voxel_map_ref_main.cpp: csrc/host/voxel_map_util.cpp in a program of its own, built with
    -fsanitize=address,undefined (tests/cpp/Makefile: _build/voxel_map_ref_sanitized) and run directly"""
    exe = cpp_tools.build("voxel_map_ref_sanitized")[0]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("voxel_map_ref_main: ok"), p.stdout + p.stderr
