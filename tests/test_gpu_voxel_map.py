"""The resident voxel map on the GPU (csrc/k_voxel_map.hip through ouster_hip_voxel_map_* and the Python face) against
tests/voxel_map_model.py: bit for bit, row order included, with guard rows behind every output.  Shapes are the smallest at which a
path can go wrong: around one workgroup, one voxel offered thousands of candidates (the serial walk), growth from a tiny reserve,
probe chains that wrap past the table's last slot, removal exactly at max_voxel_dist, ties, the edge of the int32 grid.  The inputs
are those of tests/voxel_map_cases.py, whose preconditions tests/test_voxel_map_cases_cpu.py asserts on the model."""
import functools
import os
import sys

import numpy as np
import pytest

import voxel_map_cases as K
import voxel_map_model as M
from conftest import ROOT, has_gpu

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "ouster_sdk_amd", "compat"))


@pytest.fixture(scope="module")
def gpu():
    import torch
    from ouster_sdk_amd import _capi as capi
    assert has_gpu()
    ctx = capi.Context(0)
    yield capi, ctx, torch
    ctx.close()


def device_map(gpu, *a, **kw):
    """every array of every call in device memory"""
    capi, ctx, torch = gpu
    return K.CapiMap(capi, ctx.h, *a, to_device=lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda(),
                     from_device=lambda t: t.cpu().numpy(), **kw)


def foreign_map(gpu, *a, **kw):
    """every array of every call in pageable host memory: the _host forms, staged through the context's scratch"""
    capi, ctx, _ = gpu
    return K.CapiMap(capi, ctx.h, *a, **kw)


def model_info(m, model):
    i = m.info()
    assert (i["voxels"], i["points"], i["points_per_voxel"]) == (model.num_voxels(), model.num_points(), model.max_points_per_voxel)
    assert i["voxel_capacity"] >= i["voxels"] and (i["device_bytes"] > 0) == (i["voxel_capacity"] > 0)
    return i


@functools.lru_cache(maxsize=None)
def brute_case():
    """the 2 000 / 500 case of the reference's test: rows, queries, the model fed the rows"""
    rows, queries = K.uniform_cloud(2000, 42), K.uniform_cloud(500, 43)
    rows.setflags(write=False), queries.setflags(write=False)
    model = M.VoxelHashMap3d(1.0, 100.0, 20)
    model.add_points(rows)
    return rows, queries, model


# ---- admission
@pytest.mark.parametrize("max_points", [1, 2, 20])
def test_admission_at_the_resolution_and_a_step_nearer(gpu, max_points):
    voxel, res_sq, held, at, nearer = K.admission_boundary(max_points)
    with device_map(gpu, voxel, 100.0, max_points) as m:
        model = M.VoxelHashMap3d(voxel, 100.0, max_points)
        K.check_script(m, model, [("add", [held, nearer, at]), ("cloud",), ("counts",)], "one call")
        assert model.num_points() == (1 if max_points == 1 else 2)
    with device_map(gpu, voxel, 100.0, max_points) as m:      # the held point from an earlier call gates the later ones
        K.check_script(m, M.VoxelHashMap3d(voxel, 100.0, max_points),
                       [("add", [held]), ("add", [nearer]), ("counts",), ("add", [at]), ("cloud",), ("counts",)], "three calls")


@pytest.mark.parametrize("max_points", [1, 2, 20])
def test_candidates_beyond_capacity_duplicates_and_two_calls(gpu, max_points):
    pts = K.distant_in_one_voxel(3 * 20)
    dup = np.vstack([pts[:5], pts[:5], pts[2:3], pts[2:3]])
    with device_map(gpu, 100.0, 1000.0, max_points) as m:
        model = M.VoxelHashMap3d(100.0, 1000.0, max_points)
        script = [("add", dup), ("cloud",), ("counts",),                      # duplicates: distance 0 < resolution
                  ("add", pts[:max_points // 2 + 1]), ("cloud",),              # a voxel filled across two calls ...
                  ("add", pts), ("cloud",), ("counts",), ("add", pts[::-1]), ("cloud",)]   # ... stops at P and stays there
        K.check_script(m, model, script, "P %d" % max_points)
        assert model.num_voxels() == 1 and model.num_points() <= max_points
        if max_points == 20:
            assert model.num_points() == 20


def test_one_voxel_offered_5000_candidates(gpu):
    cand = K.one_voxel_candidates(5000, 3)
    with device_map(gpu, 1.0, 100.0, 20) as m:
        K.check_script(m, M.VoxelHashMap3d(1.0, 100.0, 20), [("add", cand), ("cloud",), ("counts",), ("add", cand[::-1]), ("cloud",)], "5000")
    with device_map(gpu, 1.0, 100.0, 300) as m:         # and a voxel that keeps hundreds: a long walk against a long list
        K.check_script(m, M.VoxelHashMap3d(1.0, 100.0, 300), [("add", cand[:1200]), ("cloud",), ("counts",)], "P 300")


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 65537])
def test_row_counts_around_the_workgroup(gpu, n):
    rows = K.uniform_cloud(n, n + 1, extent=40.0 if n > 1000 else 4.0)
    with device_map(gpu, 1.0, 100.0, 3) as m:
        model = M.VoxelHashMap3d(1.0, 100.0, 3)
        K.check_script(m, model, [("add", rows), ("cloud",), ("counts",), ("add", rows[: n // 2] + 0.31), ("cloud",), ("counts",)], "n %d" % n)
        model_info(m, model)


@pytest.mark.parametrize("dtype, stride", [(K.F32, 5), (K.F64, 3)])
@pytest.mark.parametrize("memory", ["device", "foreign", "pool"])
def test_dtypes_strides_and_memories(gpu, dtype, stride, memory):
    import ctypes as C
    capi, ctx, torch = gpu
    rows, queries = K.uniform_cloud(3000, 8), K.uniform_cloud(300, 9)
    make = device_map if memory == "device" else foreign_map
    with make(gpu, 0.5, 100.0, 4, dtype=dtype, stride=stride) as m:
        model = M.VoxelHashMap3d(0.5, 100.0, 4)
        if memory == "pool":      # pooled page-locked memory: the GPU works on it in place
            L = capi.load_hip()
            nbytes = len(rows) * stride * (4 if dtype == K.F32 else 8)
            base = L.ouster_hip_host_alloc(nbytes, 0)
            assert base and L.ouster_hip_host_is_pinned(base, nbytes)
            try:
                buf = (C.c_char * nbytes).from_address(base)
                a = np.frombuffer(buf, dtype=np.float32 if dtype == K.F32 else np.float64).reshape(len(rows), stride)
                a[:] = 7.5
                a[:, :3] = rows
                capi.check(L.ouster_hip_voxel_map_add_points_host(m.h, base, dtype, len(rows), stride))
                del a, buf
            finally:
                L.ouster_hip_host_free(base)
        else:
            m.add_points(rows)
        model.add_points(m.widened(rows))
        K.same_bytes(m.pointcloud(), model.pointcloud(), "cloud")
        got = m.get_closest_neighbors(queries, 1.0)
        want = model.get_closest_neighbors(m.widened(queries), 1.0)
        K.same_bytes(got[0], want[0], "neighbours")
        K.same_bytes(got[1], want[1], "distances")


def test_a_refused_call_leaves_the_map_unchanged(gpu):
    rows = K.uniform_cloud(700, 5)
    with device_map(gpu, 1.0, 100.0, 3) as m:
        m.add_points(rows)
        before, info = m.pointcloud().tobytes(), m.info()
        for bad_value in (float("nan"), float("inf"), 3e9, -2.0 ** 31 - 1.0):
            bad = K.uniform_cloud(600, 6, extent=30.0)        # new voxels too: none of them may appear
            bad[431, 2] = bad_value
            with pytest.raises(ValueError, match=M.MSG_GRID):
                m.add_points(bad)
            with pytest.raises(ValueError, match=M.MSG_GRID):
                m.update(bad, (0.0, 0.0, 0.0))
        with pytest.raises(ValueError, match=M.MSG_GRID):
            m.update(rows, (float("nan"), 0.0, 0.0))
        with pytest.raises(ValueError, match=M.MSG_GRID):
            m.remove_voxels_far_from_location((0.0, 1e300, 0.0))
        assert m.pointcloud().tobytes() == before and m.info() == info
        q = m.get_closest_neighbors(rows[:50])
        assert (q[1] < M.DBL_MAX).all()                         # and is still searchable


# ---- table and growth
def test_growth_from_a_small_reserve(gpu):
    with device_map(gpu, 1.0, 1e6, 2) as m:
        model = M.VoxelHashMap3d(1.0, 1e6, 2)
        m.reserve(16)
        assert m.info()["voxel_capacity"] == 16 and m.info()["voxels"] == 0
        script = [("add", K.distinct_voxels(1000)), ("counts",)]
        for k in range(40):
            script.append(("add", np.vstack([K.distinct_voxels(60, start=1000 + 45 * k), K.distinct_voxels(30, start=20 * k) + 0.2])))
        script += [("cloud",), ("counts",), ("closest", K.distinct_voxels(2900)[::7] + 0.1, 3.0)]
        K.check_script(m, model, script, "growth")
        i = model_info(m, model)
        assert i["voxels"] > 2000 and i["voxel_capacity"] >= i["voxels"]
        cap = i["voxel_capacity"]
        m.reserve(10)                                            # never shrinks
        assert m.info()["voxel_capacity"] == cap
        m.clear()
        assert m.info()["voxels"] == 0 and m.info()["voxel_capacity"] == cap and m.pointcloud().shape == (0, 3)
        model.clear()
        K.check_script(m, model, [("add", K.distinct_voxels(100)), ("cloud",), ("closest", K.distinct_voxels(100), 1.0)], "after clear")


def test_probe_chains_wrap_past_the_last_slot(gpu):
    """reserve(16): 32 slots.  Cells that all start at the last slot, and at the one before: their chains run round to slot 0"""
    cells = K.cells_starting_at(31, 31, 5) + K.cells_starting_at(30, 31, 4)
    rows = np.array([[c[0] + 0.5, c[1] + 0.5, c[2] + 0.5] for c in cells])
    with device_map(gpu, 1.0, 1e6, 2) as m:
        model = M.VoxelHashMap3d(1.0, 1e6, 2)
        m.reserve(16)
        script = [("add", rows[:4]), ("add", rows[2:]), ("counts",), ("cloud",), ("closest", rows + 0.1, 0.5), ("add", rows + 0.3), ("cloud",),
                  ("extract", tuple(rows[0] + 2e6)), ("counts",), ("add", rows[::-1]), ("cloud",), ("closest", rows + 0.1, 0.5)]
        K.check_script(m, model, script, "wrap")
        assert m.info()["voxel_capacity"] == 16


def test_a_reserved_map_allocates_nothing(gpu):
    capi, ctx, _ = gpu
    rng = np.random.default_rng(21)
    with device_map(gpu, 0.5, 6.0, 4) as m:
        model = M.VoxelHashMap3d(0.5, 6.0, 4)
        m.reserve(60000)
        frames = [(np.array([0.4 * k, 0.1 * k, 0.0]) + rng.uniform(-5.0, 5.0, (4000, 3)), (0.4 * k, 0.1 * k, 0.0)) for k in range(21)]
        m.update(*frames[0])                                      # the context's workspace and scratch reach their size
        m.pointcloud()
        model.update(*frames[0])
        a = capi.alloc_stats()
        for rows, pos in frames[1:]:
            m.update(rows, pos)
            model.update(rows, pos)
        b = capi.alloc_stats()
        assert b["device_allocs"] - a["device_allocs"] == 0 and b["pinned_allocs"] - a["pinned_allocs"] == 0
        K.same_bytes(m.pointcloud(), model.pointcloud(), "after 20 updates")
        i = model_info(m, model)
        assert i["voxel_capacity"] == 60000 and len(model.cells) < 60000


# ---- removal
def test_removal_at_max_voxel_dist(gpu):
    voxel, max_distance, rows, origin, cells = K.removal_boundary()
    for extract in (False, True):
        with device_map(gpu, voxel, max_distance) as m:
            model = M.VoxelHashMap3d(voxel, max_distance)
            op = "extract" if extract else "remove"
            script = [("add", rows), (op, origin), ("cloud",), ("counts",),
                      (op, origin), ("counts",),                                        # remove none
                      ("add", rows[:4] + 0.1), ("cloud",), ("counts",),                 # ids continue, survivors are still found
                      ("closest", rows, 0.5),
                      (op, (1e5, 0.0, 0.0)), ("counts",), ("cloud",),                    # remove all
                      ("add", rows[::-1]), ("cloud",), ("closest", rows + 0.05, M.DBL_MAX)]
            K.check_script(m, model, script, op)


def test_extract_one_row_short_writes_nothing(gpu):
    voxel, max_distance, rows, origin, cells = K.removal_boundary()
    for make in (device_map, foreign_map):
        with make(gpu, voxel, max_distance) as m:
            m.add_points(rows)
            before = m.pointcloud().tobytes()
            with pytest.raises(ValueError, match="voxel map: out_capacity is too small"):
                m.extract_voxels_far_from_location(origin, capacity=5)     # CapiMap checks that every row kept its sentinel
            assert m.last_n == 6 and m.pointcloud().tobytes() == before and m.info()["voxels"] == 6
            with pytest.raises(ValueError, match="voxel map: out_capacity is too small"):
                m.pointcloud(capacity=11)
            assert m.last_n == 12
            assert len(m.extract_voxels_far_from_location(origin, capacity=6)) == 6 and m.info()["points"] == 6


def test_removal_over_many_voxels_keeps_the_order(gpu):
    rows = K.uniform_cloud(30000, 17, extent=20.0)
    with device_map(gpu, 0.5, 8.0, 3) as m:
        model = M.VoxelHashMap3d(0.5, 8.0, 3)
        K.check_script(m, model, [("add", rows), ("extract", (6.0, -3.0, 1.0)), ("cloud",), ("counts",), ("update", rows[:5000] * 0.5, (-4.0, 0.0, 0.0)),
                                  ("cloud",), ("closest", rows[::40], 1.0)], "many")
        assert 0 < model.num_voxels() < 30000


# ---- queries
@pytest.mark.parametrize("q", [0, 1, 257, 100000])
def test_query_counts(gpu, q):
    rows, _, model = brute_case()
    queries = K.uniform_cloud(q, 100 + q, extent=5.5)
    with device_map(gpu, 1.0, 100.0, 20) as m:
        m.add_points(rows)
        pts, d2 = m.get_closest_neighbors(queries, 2.0)
        assert pts.shape == (q, 3) and d2.shape == (q,)
        check = np.arange(q) if q <= 257 else np.random.default_rng(1).choice(q, 400, replace=False)   # the model is a Python loop
        want = model.get_closest_neighbors(queries[check], 2.0)
        K.same_bytes(pts[check], want[0], "neighbours")
        K.same_bytes(d2[check], want[1], "distances")
        if q == 100000:      # every row against the host map, which tests/test_voxel_map_api_cpu.py holds to the model
            capi = gpu[0]
            with K.CapiMap(capi, None, 1.0, 100.0, 20, host=True) as h:
                h.add_points(rows)
                every = h.get_closest_neighbors(queries, 2.0)
            K.same_bytes(pts, every[0], "all neighbours")
            K.same_bytes(d2, every[1], "all distances")
            miss = d2 == 2.0
            assert (pts[miss] == 0.0).all() and (d2[~miss] < 2.0).all() and miss.any() and not miss.all()


@pytest.mark.parametrize("bound", [None, 2.0])
def test_the_brute_force_case_of_the_reference(gpu, bound):
    rows, queries, model = brute_case()
    b2 = M.DBL_MAX if bound is None else bound * bound
    with device_map(gpu, 1.0, 100.0, 20) as m:
        m.add_points(rows)
        held = m.pointcloud()
        K.same_bytes(held, model.pointcloud(), "cloud")
        pts, d2 = m.get_closest_neighbors(queries, b2)
        want = model.get_closest_neighbors(queries, b2)
        K.same_bytes(pts, want[0], "neighbours")
        K.same_bytes(d2, want[1], "distances")
        brute = ((held[None, :, :] - queries[:, None, :]) ** 2).sum(axis=2).min(axis=1)
        near = brute < b2
        assert np.abs(d2[near] - brute[near]).max() <= 1e-12 and (d2[~near] >= b2).all()
        for i in range(0, 500, 25):                                # batched equals single
            p, d = m.get_closest_neighbor(queries[i], b2)
            assert np.array(p).tobytes() == pts[i].tobytes() and d == d2[i]


def test_faces_edges_corners_and_ties(gpu):
    pts, queries = K.lattice_ties()
    with device_map(gpu, 1.0, 100.0, 1) as m:
        K.check_script(m, M.VoxelHashMap3d(1.0, 100.0, 1), [("add", pts), ("closest", queries, M.DBL_MAX), ("closest", queries, 0.75),   # d^2 == bound
                                                            ("closest", queries, 0.5), ("closest", queries, 0.7500000000000001)], "ties")
    cloud = K.uniform_cloud(4000, 12, extent=1.5)
    with device_map(gpu, 0.5, 100.0, 5) as m:
        K.check_script(m, M.VoxelHashMap3d(0.5, 100.0, 5), [("add", cloud), ("closest", K.face_edge_corner_queries(), M.DBL_MAX),
                                                            ("closest", K.face_edge_corner_queries(), 0.01)], "faces")


def test_empty_map_grid_edge_and_nan(gpu):
    top = float(2 ** 31 - 1)
    queries = [(top + 0.25, 0.5, 0.5), (float("nan"), 0.5, 0.5), (top + 1.5, 0.5, 0.5), (-top - 1.5, 0.0, 0.0), (0.5, float("inf"), 0.5),
               (-top - 0.75, 0.5, 0.5), (top - 0.25, 0.5, 0.5)]
    with device_map(gpu, 1.0) as m:
        model = M.VoxelHashMap3d(1.0)
        script = [("closest", queries, 7.0), ("closest", queries, M.DBL_MAX), ("cloud",), ("counts",), ("remove", (0, 0, 0)), ("extract", (0, 0, 0)),
                  ("add", [(top + 0.5, 0.5, 0.5), (top - 0.5, 0.5, 0.5), (-top - 0.5, 0.5, 0.5)]),     # cells 2^31 - 1, 2^31 - 2 and -2^31
                  ("closest", queries, 7.0), ("closest", queries, M.DBL_MAX), ("closest", queries, float("nan")),
                  ("extract", (top, 0.0, 0.0)), ("cloud",),                                          # a cell distance of 2^32 - 1: far, exactly
                  ("extract", (-top, 0.0, 0.0)), ("counts",)]
        K.check_script(m, model, script, "edge")


# ---- order and replay
def test_the_same_script_twice_gives_the_same_bytes(gpu):
    script = K.moving_script(31, calls=6, n=5000, extent=8.0)
    with device_map(gpu, 0.5, 6.0, 4) as a, foreign_map(gpu, 0.5, 6.0, 4) as b:
        first, again = K.run_script(a, script), K.run_script(b, script)
        want = K.run_script(M.VoxelHashMap3d(0.5, 6.0, 4), script)
        for (name, x), (_, y), (_, w) in zip(first, again, want):
            assert x.tobytes() == y.tobytes(), name
            K.same_bytes(x.reshape(w.shape), w, name)


# ---- the Python face
def test_python_face(gpu):
    import ouster.sdk.core as core
    from ouster_sdk_amd import core as amd
    assert core.VoxelHashMap3d is amd.VoxelHashMap3d
    rows, queries, model = brute_case()
    m = amd.VoxelHashMap3d(1.0, 100.0, 20)
    assert m.empty and m.device == 0 and m.device_bytes == 0
    m.add_points(rows)
    assert not m.empty and m.num_voxels == model.num_voxels() and m.num_points == model.num_points() and m.device_bytes > 0
    K.same_bytes(m.point_cloud(), model.pointcloud(), "point_cloud")
    pts, d2 = m.get_closest_neighbors(queries, 4.0)
    want = model.get_closest_neighbors(queries, 4.0)
    K.same_bytes(pts, want[0], "neighbours")
    K.same_bytes(d2, want[1], "distances")
    p, d = m.get_closest_neighbor(queries[3])
    assert (tuple(p), d) == model.get_closest_neighbor(queries[3])
    origin = np.array([150.0, 0.0, 0.0])
    far = model.extract_voxels_far_from_location(origin)
    assert len(far) > 0
    K.same_bytes(m.extract_voxels_far_from_location(origin), far, "extract")
    m.update(rows[:100] + 3.0, np.array([1.0, 2.0, 3.0]))
    model.update(rows[:100] + 3.0, (1.0, 2.0, 3.0))
    m.remove_voxels_far_from_location(np.array([50.0, 50.0, 50.0]))
    model.remove_voxels_far_from_location((50.0, 50.0, 50.0))
    K.same_bytes(m.point_cloud(), model.pointcloud(), "after update and removal")
    with pytest.raises(ValueError, match="^add_points expects an Nx3 array$"):
        m.add_points(np.zeros((3, 4)))
    with pytest.raises(ValueError, match="^VoxelHashMap method expects a 3-element point$"):
        m.get_closest_neighbor(np.zeros(4))
    with pytest.raises(ValueError, match=M.MSG_GRID):
        m.add_points(np.array([[0.0, 0.0, float("nan")]]))
    K.same_bytes(m.point_cloud(), model.pointcloud(), "after a refusal")
    m.clear()
    assert m.empty and m.point_cloud().shape == (0, 3)
