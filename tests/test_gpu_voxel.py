"""Voxel down-sampling on the GPU (csrc/k_voxel.hip through ouster_hip_voxel_downsample / _host and the Python face) against
tests/voxel_model.py: bit for bit, row order included, with guard rows behind every output.  Shapes are the smallest at which a
path can go wrong: around one wave, few voxels under heavy atomic traffic, long probe chains, one voxel holding everything (the
serial fold, a sort with one key), more than 65 536 voxels (three sort digits), and a context reused across sizes."""
import functools
import os
import sys

import numpy as np
import pytest

import voxel_cases as K
import voxel_model as M
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


def device_call(gpu, frame, voxel_size, **kw):
    capi, ctx, torch = gpu
    return K.call(capi.load_hip().ouster_hip_voxel_downsample, ctx.h, frame, voxel_size,
                  to_device=lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda(), from_device=lambda t: t.cpu().numpy(), **kw)


def host_call(gpu, frame, voxel_size, **kw):
    capi, ctx, _ = gpu
    return K.call(capi.load_hip().ouster_hip_voxel_downsample_host, ctx.h, frame, voxel_size, **kw)


@functools.lru_cache(maxsize=None)
def big_cloud():
    a = K.uniform_cloud(100003, cols=3, seed=7)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def big_want(voxel_size, strategy):
    return K.want(big_cloud(), voxel_size, strategy=strategy)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65])
def test_around_one_wave(gpu, n):
    cloud = K.uniform_cloud(n, cols=3, seed=n, extent=2.0)
    for strategy in M.STRATEGIES:
        K.check_rows(device_call(gpu, cloud, 0.9, strategy=strategy), K.want(cloud, 0.9, strategy=strategy), 3, "n %d strategy %d" % (n, strategy))


def test_recorded_case_of_the_reference(gpu):
    frame, recorded = K.recorded_case()
    for voxel_size, rows in recorded:
        res = device_call(gpu, frame, voxel_size, strategy=M.AVERAGE_POINT)
        K.check_rows(res, K.want(frame, voxel_size, strategy=M.AVERAGE_POINT), 5, "voxel %g" % voxel_size)
        assert np.array_equal(M.sorted_rows(res[2][:res[1]]), M.sorted_rows(rows))


@pytest.mark.parametrize("min_pts", [1, 2, 5])
def test_few_voxels_many_points(gpu, min_pts):
    cloud = K.clustered_cloud(4096, clusters=7)
    extra = np.array([[90.5, 0.5, 0.5]] * 1 + [[91.5, 0.5, 0.5]] * 2 + [[92.5, 0.5, 0.5]] * 4)   # voxels of 1, 2 and 4 points
    cloud = np.vstack([cloud[:2000], extra, cloud[2000:]])
    K.check_rows(device_call(gpu, cloud, 1.0, min_pts=min_pts, strategy=M.AVERAGE_POINT),
                 K.want(cloud, 1.0, 1, min_pts, M.AVERAGE_POINT), 3, "min_pts %d" % min_pts)
    for strategy in (M.FIRST_N_POINT, M.RANDOM):   # the selecting strategies do not look at the threshold
        K.check_rows(device_call(gpu, cloud, 1.0, min_pts=min_pts, strategy=strategy), K.want(cloud, 1.0, 1, min_pts, strategy), 3,
                     "strategy %d" % strategy)


@pytest.mark.parametrize("diagonal", [False, True])
def test_distinct_voxels_in_a_row(gpu, diagonal):
    cloud = K.line_cloud(4096, diagonal)
    for strategy in (M.AVERAGE_POINT, M.RANDOM):
        for log2 in (0, 13, 22):    # automatic, 8192 slots, a very sparse table
            K.check_rows(device_call(gpu, cloud, 1.0, strategy=strategy, table_log2=log2), K.want(cloud, 1.0, strategy=strategy), 3,
                         "strategy %d table 2^%d" % (strategy, log2))


def test_faces_negative_coordinates_and_zeros(gpu):
    cloud = K.face_cloud()
    for strategy in M.STRATEGIES:
        K.check_rows(device_call(gpu, cloud, 0.5, strategy=strategy), K.want(cloud, 0.5, strategy=strategy), 3, "strategy %d" % strategy)
    lone = np.array([[-0.0, -0.0, -0.0]])
    res = device_call(gpu, lone, 1.0, strategy=M.AVERAGE_POINT)
    K.check_rows(res, K.want(lone, 1.0, strategy=M.AVERAGE_POINT), 3, "a lone -0.0")
    assert not np.signbit(res[2][0]).any()


def test_everything_in_one_voxel(gpu):
    rng = np.random.default_rng(9)
    cloud = rng.uniform(0.01, 0.99, (65536, 4))
    cloud[:, 3] = rng.uniform(-1.0, 1.0, 65536) * 10.0 ** rng.integers(-8, 9, 65536)   # a sum whose bits depend on its order
    for strategy in M.STRATEGIES:
        K.check_rows(device_call(gpu, cloud, 1.0, strategy=strategy), K.want(cloud, 1.0, strategy=strategy), 4, "strategy %d" % strategy)


@pytest.mark.parametrize("voxel_size", [0.5, 4.0])
def test_large_uniform_cloud(gpu, voxel_size):
    expect = big_want(voxel_size, M.AVERAGE_POINT)
    assert (len(expect) > 65536) == (voxel_size == 0.5)
    first = device_call(gpu, big_cloud(), voxel_size, strategy=M.AVERAGE_POINT)
    K.check_rows(first, expect, 3, "average")
    again = device_call(gpu, big_cloud(), voxel_size, strategy=M.AVERAGE_POINT)
    assert again[1] == first[1] and again[2].tobytes() == first[2].tobytes()      # the same call twice: the same bytes
    K.check_rows(device_call(gpu, big_cloud(), voxel_size, strategy=M.RANDOM), big_want(voxel_size, M.RANDOM), 3, "last wins")
    # the hash table nearly full (131 072 slots for 100 003 rows) and very sparse: the same bytes as the automatic size
    for log2 in (17, 22):
        K.check_rows(device_call(gpu, big_cloud(), voxel_size, strategy=M.AVERAGE_POINT, table_log2=log2), expect, 3, "table 2^%d" % log2)


@pytest.mark.parametrize("cols", [3, 4, 5, 9])
def test_attribute_columns_strides_and_float_input(gpu, cols):
    cloud = K.clustered_cloud(3000, clusters=40, cols=cols, seed=cols)
    for strategy in M.STRATEGIES:
        expect = K.want(cloud, 1.0, strategy=strategy)
        K.check_rows(device_call(gpu, cloud, 1.0, strategy=strategy), expect, cols, "dense, strategy %d" % strategy)
        K.check_rows(device_call(gpu, cloud, 1.0, strategy=strategy, row_stride=cols + 3), expect, cols, "strided, strategy %d" % strategy)
    f32 = cloud.astype(np.float32)
    K.check_rows(device_call(gpu, f32, 1.0, strategy=M.AVERAGE_POINT, dtype=np.float32, row_stride=cols + 1),
                 K.want(f32, 1.0, strategy=M.AVERAGE_POINT), cols, "float input")


def test_with_normals(gpu):
    pts, nrm = K.normals_cloud()
    expect = K.want(pts, 1.0, normals=nrm)
    assert 0 < len(expect[0]) < len(pts)
    K.check_rows(device_call(gpu, pts, 1.0, normals=nrm), expect, 3, "with normals")
    K.check_rows(host_call(gpu, pts, 1.0, normals=nrm), expect, 3, "with normals, host arrays")
    f32 = pts.astype(np.float32)
    K.check_rows(device_call(gpu, f32, 1.0, normals=nrm, dtype=np.float32), K.want(f32, 1.0, normals=nrm), 3, "float points")
    # nothing but rows that are skipped, and a voxel whose normals cancel: no row at all
    K.check_rows(device_call(gpu, pts[:2], 1.0, normals=np.zeros((2, 3))), (np.zeros((0, 3)), np.zeros((0, 3))), 3, "all skipped")
    # a skipped row may lie outside the grid; one that takes part may not
    far, keep = pts.copy(), nrm.copy()
    far[0], keep[0] = 1e13, 0.0
    K.check_rows(device_call(gpu, far, 1.0, normals=keep), K.want(far, 1.0, normals=keep), 3, "skipped row outside the grid")
    keep[0] = [0.0, 0.0, 1.0]
    capi = gpu[0]
    K.check_untouched(device_call(gpu, far, 1.0, normals=keep), capi.ERR_INVALID_ARGUMENT, "row outside the grid")
    assert M.MSG_GRID in capi.load_hip().ouster_hip_last_error().decode()


def test_refusals_leave_the_output_untouched(gpu):
    capi = gpu[0]
    last_error = lambda: capi.load_hip().ouster_hip_last_error().decode()
    cloud = K.clustered_cloud(500, clusters=6, seed=33)
    for bad in (1e13, np.nan):
        c = cloud.copy()
        c[321, 2] = bad
        for strategy in M.STRATEGIES:
            for fn in (device_call, host_call):
                K.check_untouched(fn(gpu, c, 0.5, strategy=strategy), capi.ERR_INVALID_ARGUMENT, "bad %r" % bad)
                assert M.MSG_GRID in last_error()
    expect = K.want(cloud, 1.0, strategy=M.AVERAGE_POINT)
    for fn in (device_call, host_call):
        short = fn(gpu, cloud, 1.0, strategy=M.AVERAGE_POINT, capacity=len(expect) - 1)
        assert K.check_untouched(short, capi.ERR_INVALID_ARGUMENT, "one row short") == len(expect)
        K.check_rows(fn(gpu, cloud, 1.0, strategy=M.AVERAGE_POINT, capacity=len(expect)), expect, 3, "exactly enough rows")
    # the two sequential combinations: not on the device, the right answer from the host form
    for strategy in (M.FIRST_N_POINT, M.RANDOM):
        K.check_untouched(device_call(gpu, cloud, 1.0, max_points=3, strategy=strategy), capi.ERR_UNSUPPORTED, "n > 1 on the device")
        K.check_rows(host_call(gpu, cloud, 1.0, max_points=3, strategy=strategy), K.want(cloud, 1.0, 3, 1, strategy), 3, "n > 1, host form")
    K.check_untouched(device_call(gpu, cloud, 1.0, strategy=M.AVERAGE_POINT, table_log2=8), capi.ERR_INVALID_ARGUMENT, "table of 256 slots")


def test_one_context_across_sizes(gpu):
    """the stale-table and stale-workspace case: a large call, a tiny one, a middling one on the same context"""
    capi, _, _ = gpu
    ctx = capi.Context(0)
    try:
        own = (capi, ctx, gpu[2])
        K.check_rows(device_call(own, big_cloud(), 4.0, strategy=M.AVERAGE_POINT), big_want(4.0, M.AVERAGE_POINT), 3, "100 003 rows")
        small = K.uniform_cloud(10, seed=4, extent=1.0)
        K.check_rows(device_call(own, small, 0.5, strategy=M.AVERAGE_POINT), K.want(small, 0.5, strategy=M.AVERAGE_POINT), 3, "10 rows")
        mid = K.clustered_cloud(4096, clusters=7)
        K.check_rows(device_call(own, mid, 1.0, strategy=M.AVERAGE_POINT), K.want(mid, 1.0, strategy=M.AVERAGE_POINT), 3, "4096 rows")
        pts, nrm = K.normals_cloud()
        K.check_rows(device_call(own, pts, 1.0, normals=nrm), K.want(pts, 1.0, normals=nrm), 3, "with normals after the rest")
    finally:
        ctx.close()


def test_host_forms_on_pooled_and_foreign_memory(gpu):
    import ctypes as C
    capi, ctx, _ = gpu
    L = capi.load_hip()
    cloud = K.clustered_cloud(3000, clusters=40, cols=5, seed=8)
    expect = K.want(cloud, 1.0, strategy=M.AVERAGE_POINT)
    K.check_rows(host_call(gpu, cloud, 1.0, strategy=M.AVERAGE_POINT), expect, 5, "foreign memory")
    K.check_rows(host_call(gpu, cloud.astype(np.float32), 1.0, strategy=M.RANDOM, dtype=np.float32, row_stride=6),
                 K.want(cloud.astype(np.float32), 1.0), 5, "foreign memory, float, strided")
    n, cols = cloud.shape
    cap, rows = n, len(expect)      # room for every row: the pool pins allocations of 2 KiB and more only
    bytes_in, bytes_out = cloud.nbytes, (cap + K.GUARD_ROWS) * cols * 8
    p_in, p_out = L.ouster_hip_host_alloc(bytes_in, 1), L.ouster_hip_host_alloc(bytes_out, 1)
    try:
        assert L.ouster_hip_host_is_pinned(p_in, bytes_in) == 1 and L.ouster_hip_host_is_pinned(p_out, bytes_out) == 1
        src = np.frombuffer((C.c_uint8 * bytes_in).from_address(p_in), np.float64).reshape(n, cols)
        out = np.frombuffer((C.c_uint8 * bytes_out).from_address(p_out), np.float64).reshape(cap + K.GUARD_ROWS, cols)
        src[:], out[:] = cloud, K.GUARD
        d = capi.VoxelDesc()
        d.points, d.out, d.n, d.cols, d.out_capacity = p_in, p_out, n, cols, cap
        d.dtype, d.voxel_size, d.max_points_per_voxel, d.min_pts_threshold, d.strategy = capi.F64, 1.0, 1, 1, M.AVERAGE_POINT
        n_out = C.c_uint64()
        capi.check(L.ouster_hip_voxel_downsample_host(ctx.h, C.byref(d), C.byref(n_out)))
        assert n_out.value == rows
        M.same_bits(out[:rows], expect, "pool memory in place")
        assert (out[rows:] == K.GUARD).all()
    finally:
        L.ouster_hip_host_free(p_in)
        L.ouster_hip_host_free(p_out)


def test_phase_times_of_a_timed_call(gpu):
    import ctypes as C
    capi, _, _ = gpu
    L = capi.load_hip()
    ctx = capi.Context(0)
    try:
        own = (capi, ctx, gpu[2])
        ms = (C.c_float * len(capi.VOXEL_PHASES))()
        cloud = K.clustered_cloud(4096, clusters=7)
        expect = K.want(cloud, 1.0, strategy=M.AVERAGE_POINT)
        K.check_rows(device_call(own, cloud, 1.0, strategy=M.AVERAGE_POINT), expect, 3, "untimed")
        assert L.ouster_hip_voxel_phase_ms(ctx.h, ms) == capi.ERR_INVALID_ARGUMENT       # no timed call yet
        capi.check(L.ouster_hip_voxel_timing(ctx.h, 1))
        assert L.ouster_hip_voxel_phase_ms(ctx.h, ms) == capi.ERR_INVALID_ARGUMENT
        K.check_rows(device_call(own, cloud, 1.0, strategy=M.AVERAGE_POINT), expect, 3, "timed: the same rows")
        capi.check(L.ouster_hip_voxel_phase_ms(ctx.h, ms))
        assert all(0.0 <= t < 1000.0 for t in ms) and sum(ms) > 0.0, list(ms)
        capi.check(L.ouster_hip_voxel_timing(ctx.h, 0))
        assert L.ouster_hip_voxel_phase_ms(ctx.h, ms) == capi.ERR_INVALID_ARGUMENT
    finally:
        ctx.close()


def test_python_face(gpu):
    import ouster.sdk.core as core
    from ouster_sdk_amd import core as amd
    assert core.voxel_downsample_xd is amd.voxel_downsample_xd and core.voxel_downsample is amd.voxel_downsample_xd
    S = core.VoxelDownsampleStrategy
    frame, recorded = K.recorded_case()
    for voxel_size, rows in recorded:
        got = core.voxel_downsample_xd(frame, voxel_size, 1, 1, S.AVERAGE_POINT)
        M.same_bits(got, K.want(frame, voxel_size, strategy=M.AVERAGE_POINT), "recorded case")
        assert np.array_equal(M.sorted_rows(got), M.sorted_rows(rows))
    cloud = K.clustered_cloud(3000, clusters=40, cols=5, seed=8)
    M.same_bits(core.voxel_downsample_xd(cloud, 1.0), K.want(cloud, 1.0), "defaults: RANDOM, one point")
    M.same_bits(core.voxel_downsample_3d(cloud[:, :3], 1.0, strategy=S.FIRST_N_POINT, max_points_per_voxel=4),
                M.voxel_downsample_3d(cloud[:, :3], 1.0, 4, 1, M.FIRST_N_POINT), "the host-routed combination")
    M.same_bits(core.voxel_downsample_3d(cloud[:, :3], 1.0, min_pts_threshold=80, strategy=S.AVERAGE_POINT),
                M.voxel_downsample_3d(cloud[:, :3], 1.0, 1, 80, M.AVERAGE_POINT), "3d, threshold")
    pts, nrm = K.normals_cloud()
    got = amd.voxel_downsample_with_normals(pts, nrm, 1.0)
    expect = K.want(pts, 1.0, normals=nrm)
    M.same_bits(got[0], expect[0], "with normals: points")
    M.same_bits(got[1], expect[1], "with normals: normals")
    bad = cloud.copy()
    bad[5, 0] = np.inf
    with pytest.raises(ValueError, match="outside the int32 voxel grid"):
        core.voxel_downsample_xd(bad, 1.0, strategy=S.AVERAGE_POINT)
