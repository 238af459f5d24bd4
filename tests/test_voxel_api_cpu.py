"""The public surface of voxel down-sampling, checked without a GPU: C ABI symbols and struct layout, the host restatement
(ouster_hip_voxel_downsample_ref) bit for bit against tests/voxel_model.py including row order, every error through the C ABI,
through Python and through C++ (tests/cpp/voxel_snippet.cpp, compiled and linked against the two headers), the loud failure of
the GPU entry points without a GPU, and the two host-routed combinations, which work without one."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import cpp_tools
import voxel_cases as K
import voxel_model as M
from conftest import ROOT, has_gpu
from ouster_sdk_amd import _capi as capi

sys.path.insert(0, os.path.join(ROOT, "ouster_sdk_amd", "compat"))

SYMBOLS = ["ouster_hip_voxel_downsample", "ouster_hip_voxel_downsample_host", "ouster_hip_voxel_downsample_ref",
           "ouster_hip_voxel_timing", "ouster_hip_voxel_phase_ms"]


def ref(frame, voxel_size, **kw):
    return K.call(capi.load_hip().ouster_hip_voxel_downsample_ref, False, frame, voxel_size, **kw)


def last_error():
    return capi.load_hip().ouster_hip_last_error().decode()


def test_symbols_are_declared_and_exported():
    L = capi.load_hip()
    header = open(os.path.join(ROOT, "include", "ouster_hip.h")).read()
    for name in SYMBOLS:
        assert name in capi.ABI_SYMBOLS and hasattr(L, name) and ("int " + name + "(") in header, name
    assert C.sizeof(capi.VoxelDesc) == 4 * 8 + 5 * 8 + 8 + 4 * 4
    assert (capi.VOXEL_FIRST_N_POINT, capi.VOXEL_AVERAGE_POINT, capi.VOXEL_RANDOM) == (M.FIRST_N_POINT, M.AVERAGE_POINT, M.RANDOM)
    assert "#define OUSTER_HIP_VOXEL_PHASES %d" % len(capi.VOXEL_PHASES) in header
    ms = (C.c_float * len(capi.VOXEL_PHASES))()
    assert L.ouster_hip_voxel_timing(None, 1) == capi.ERR_INVALID_ARGUMENT and L.ouster_hip_voxel_phase_ms(None, ms) == capi.ERR_INVALID_ARGUMENT
    for name, value in (("FIRST_N_POINT", 0), ("AVERAGE_POINT", 1), ("RANDOM", 2)):
        assert "#define OUSTER_HIP_VOXEL_%s %d" % (name, value) in header


@pytest.mark.parametrize("strategy", M.STRATEGIES)
@pytest.mark.parametrize("max_points", [1, 3])
@pytest.mark.parametrize("cols", [3, 5, 9])
def test_ref_equals_the_model_bit_for_bit(strategy, max_points, cols):
    cloud = K.clustered_cloud(1500, clusters=30, cols=cols, seed=cols + max_points)
    for min_pts in (1, 40):
        K.check_rows(ref(cloud, 1.0, max_points=max_points, min_pts=min_pts, strategy=strategy),
                     K.want(cloud, 1.0, max_points, min_pts, strategy), cols, "min_pts %d" % min_pts)
    f32 = cloud.astype(np.float32)
    K.check_rows(ref(f32, 0.7, max_points=max_points, strategy=strategy, dtype=np.float32, row_stride=cols + 2),
                 K.want(f32, 0.7, max_points, 1, strategy), cols, "float, strided")


def test_ref_on_the_recorded_case_faces_and_normals():
    frame, recorded = K.recorded_case()
    for voxel_size, rows in recorded:
        res = ref(frame, voxel_size, strategy=M.AVERAGE_POINT)
        K.check_rows(res, K.want(frame, voxel_size, strategy=M.AVERAGE_POINT), 5, "recorded")
        assert np.array_equal(M.sorted_rows(res[2][:res[1]]), M.sorted_rows(rows))
    faces = K.face_cloud()
    for strategy in M.STRATEGIES:
        K.check_rows(ref(faces, 0.5, strategy=strategy), K.want(faces, 0.5, strategy=strategy), 3, "faces")
    pts, nrm = K.normals_cloud()
    K.check_rows(ref(pts, 1.0, normals=nrm), K.want(pts, 1.0, normals=nrm), 3, "with normals")
    K.check_rows(ref(np.zeros((0, 3)), 1.0, normals=np.zeros((0, 3))), (np.zeros((0, 3)), np.zeros((0, 3))), 3, "with normals, empty")
    K.check_rows(ref(np.zeros((0, 4)), -1.0, max_points=0), np.zeros((0, 4)), 4, "empty: before any check")


def test_ref_refusals_leave_the_output_untouched():
    cloud = K.clustered_cloud(300, clusters=5, seed=2)
    for bad in (1e13, np.nan, np.inf):
        c = cloud.copy()
        c[123, 0] = bad
        for strategy in M.STRATEGIES:
            K.check_untouched(ref(c, 0.5, max_points=2, strategy=strategy), capi.ERR_INVALID_ARGUMENT, "bad %r" % bad)
            assert last_error() == M.MSG_GRID
    for strategy, max_points in ((M.AVERAGE_POINT, 1), (M.FIRST_N_POINT, 3), (M.RANDOM, 3)):
        expect = K.want(cloud, 1.0, max_points, 1, strategy)
        assert K.check_untouched(ref(cloud, 1.0, max_points=max_points, strategy=strategy, capacity=len(expect) - 1),
                                 capi.ERR_INVALID_ARGUMENT, "one row short") == len(expect)
        K.check_rows(ref(cloud, 1.0, max_points=max_points, strategy=strategy, capacity=len(expect)), expect, 3, "exactly enough")


def test_c_abi_validation_comes_before_the_gpu():
    """ctx is NULL in every call of the two GPU forms: a validation error must win over it, which shows that nothing touched the
    GPU.  The host restatement refuses the same way."""
    L = capi.load_hip()
    good, nrm = np.zeros((4, 3)), np.ones((4, 3))
    nan, inf = float("nan"), float("inf")
    cases = [
        (M.MSG_XD, dict(frame=np.zeros((4, 2)), voxel_size=1.0)),
        (M.MSG_MAX_POINTS, dict(frame=good, voxel_size=-1.0, max_points=0)),              # before the voxel size
        (M.MSG_VOXEL_SIZE, dict(frame=good, voxel_size=0.0)),
        (M.MSG_VOXEL_SIZE, dict(frame=good, voxel_size=-1.0, strategy=M.AVERAGE_POINT)),
        (M.MSG_VOXEL_SIZE, dict(frame=good, voxel_size=nan)),
        (M.MSG_VOXEL_SIZE, dict(frame=good, voxel_size=inf, max_points=3)),
        (M.MSG_STRATEGY, dict(frame=good, voxel_size=1.0, strategy=3)),
        (M.MSG_WN_SHAPE, dict(frame=np.zeros((4, 4)), voxel_size=1.0, normals=nrm)),
        (M.MSG_WN_SIZE, dict(frame=good, voxel_size=0.0, normals=nrm)),
        (M.MSG_WN_SIZE, dict(frame=good, voxel_size=inf, normals=nrm)),
        (M.MSG_WN_SHAPE, dict(frame=np.zeros((4, 5)), voxel_size=-1.0, normals=nrm)),     # shapes before the voxel size
    ]
    for message, kw in cases:
        frame, voxel_size = kw.pop("frame"), kw.pop("voxel_size")
        for fn, ctx in ((L.ouster_hip_voxel_downsample, None), (L.ouster_hip_voxel_downsample_host, None),
                        (L.ouster_hip_voxel_downsample_ref, False)):
            K.check_untouched(K.call(fn, ctx, frame, voxel_size, **kw), capi.ERR_INVALID_ARGUMENT, message)
            assert last_error() == message
    # table_log2: 2^table_log2 must exceed n
    for fn in (L.ouster_hip_voxel_downsample, L.ouster_hip_voxel_downsample_host):
        K.check_untouched(K.call(fn, None, good, 1.0, table_log2=2), capi.ERR_INVALID_ARGUMENT, "table_log2")
        assert "table_log2" in last_error()
        # an empty frame is an empty result before any check, without a context
        rc, n_out, _, _ = K.call(fn, None, np.zeros((0, 3)), -1.0, max_points=0)
        assert rc == capi.OK and n_out == 0


def test_sequential_combinations_are_host_code():
    """FIRST_N_POINT and RANDOM keeping several points: UNSUPPORTED on device pointers, the model's rows from the _host form --
    with no context at all, so no GPU was asked for."""
    L = capi.load_hip()
    cloud = K.clustered_cloud(800, clusters=12, cols=4, seed=6)
    for strategy in (M.FIRST_N_POINT, M.RANDOM):
        for max_points in (2, 5):
            K.check_untouched(K.call(L.ouster_hip_voxel_downsample, None, cloud, 1.0, max_points=max_points, strategy=strategy),
                              capi.ERR_UNSUPPORTED, "device form")
            K.check_rows(K.call(L.ouster_hip_voxel_downsample_host, None, cloud, 1.0, max_points=max_points, strategy=strategy),
                         K.want(cloud, 1.0, max_points, 1, strategy), 4, "host form, no context")


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_gpu_entry_points_without_a_gpu_fail_loudly():
    L = capi.load_hip()
    cloud = K.clustered_cloud(100, clusters=3)
    with pytest.raises(capi.OusterHipError):
        capi.Context(0)
    for fn in (L.ouster_hip_voxel_downsample, L.ouster_hip_voxel_downsample_host):
        for kw in (dict(strategy=M.AVERAGE_POINT), dict(strategy=M.RANDOM), dict(normals=np.ones((100, 3)))):
            K.check_untouched(K.call(fn, None, cloud, 1.0, **kw), capi.ERR_INVALID_ARGUMENT, "no context can exist")
            assert last_error() == "ctx is NULL"
    from ouster_sdk_amd import core as amd
    for call in (lambda: amd.voxel_downsample_xd(cloud, 1.0), lambda: amd.voxel_downsample_3d(cloud, 1.0, strategy=amd.VoxelDownsampleStrategy.AVERAGE_POINT),
                 lambda: amd.voxel_downsample_with_normals(cloud, np.ones((100, 3)), 1.0)):
        with pytest.raises(RuntimeError):
            call()


def test_python_face_names_defaults_and_errors():
    import ouster.sdk.core as core
    from ouster_sdk_amd import core as amd
    assert core.voxel_downsample_3d is amd.voxel_downsample_3d and core.voxel_downsample_xd is amd.voxel_downsample_xd
    assert core.voxel_downsample is amd.voxel_downsample_xd and core.VoxelDownsampleStrategy is amd.VoxelDownsampleStrategy
    S = core.VoxelDownsampleStrategy
    assert (int(S.FIRST_N_POINT), int(S.AVERAGE_POINT), int(S.RANDOM)) == (0, 1, 2)
    good = np.zeros((4, 3))
    cases = [
        (M.MSG_3D, lambda: core.voxel_downsample_3d(np.zeros((4, 4)), 1.0)),
        (M.MSG_3D, lambda: core.voxel_downsample_3d(np.zeros(3), 1.0)),
        (M.MSG_XD, lambda: core.voxel_downsample_xd(np.zeros((4, 2)), 1.0)),
        (M.MSG_XD, lambda: core.voxel_downsample(np.zeros((0, 2)), 1.0)),
        (M.MSG_MAX_POINTS, lambda: core.voxel_downsample_xd(good, -1.0, 0)),
        (M.MSG_MAX_POINTS, lambda: core.voxel_downsample_3d(frame=good, voxel_size=1.0, max_points_per_voxel=0, min_pts_threshold=1,
                                                            strategy=S.AVERAGE_POINT)),
        (M.MSG_VOXEL_SIZE, lambda: core.voxel_downsample_3d(good, 0.0)),
        (M.MSG_VOXEL_SIZE, lambda: core.voxel_downsample_xd(good, float("nan"), strategy=S.AVERAGE_POINT)),
        (M.MSG_VOXEL_SIZE, lambda: core.voxel_downsample_xd(good, -1.0, 4, 1, S.FIRST_N_POINT)),
        (M.MSG_WN_SHAPE, lambda: amd.voxel_downsample_with_normals(np.zeros((4, 4)), good, 1.0)),
        (M.MSG_WN_SHAPE, lambda: amd.voxel_downsample_with_normals(good, np.zeros(3), 1.0)),
        (M.MSG_WN_ROWS, lambda: amd.voxel_downsample_with_normals(good, np.zeros((5, 3)), 1.0)),
        (M.MSG_WN_SIZE, lambda: amd.voxel_downsample_with_normals(points=good, normals=good, voxel_size=0.0)),
    ]
    for message, call in cases:
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == message
    for fn in (core.voxel_downsample_3d, core.voxel_downsample_xd):
        assert fn(np.zeros((0, 3)), -1.0, 0).shape == (0, 3)
    # the host-routed combinations give the model's rows on any machine
    cloud = K.clustered_cloud(800, clusters=12, cols=4, seed=6)
    M.same_bits(core.voxel_downsample_xd(cloud, 1.0, 3, 1, S.FIRST_N_POINT), K.want(cloud, 1.0, 3, 1, M.FIRST_N_POINT), "FIRST_N_POINT, 3")
    M.same_bits(core.voxel_downsample_3d(cloud[:, :3], 1.0, max_points_per_voxel=2), M.voxel_downsample_3d(cloud[:, :3], 1.0, 2), "RANDOM, 2")
    far = cloud.copy()
    far[7, 1] = -1e13
    with pytest.raises(ValueError, match=M.MSG_GRID):
        core.voxel_downsample_xd(far, 0.5, 2)


def test_cpp_caller_compiles_links_and_runs():
    """tests/cpp/voxel_snippet.cpp, built by tests/cpp/Makefile with the flags of the other C++ tests and -Werror"""
    p = cpp_tools.run("voxel_snippet", [], timeout=300)
    assert "validation ok" in p.stdout and "host route ok" in p.stdout, p.stdout
    assert p.stdout.splitlines()[-1].startswith("ok" if has_gpu() else "no-gpu"), p.stdout
