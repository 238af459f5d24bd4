"""ICPRegistration on host maps (OUSTER_HIP_VOXEL_MAP_HOST: csrc/host/registration_util.cpp on one core, left-fold sums) against
tests/registration_model.py bit for bit; every refusal through the C ABI, C++ (tests/cpp/registration_snippet.cpp) and Python; the
reference's Python scenarios through ouster.sdk.mapping.  No GPU."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import cpp_tools
import registration_cases as K
import registration_model as R
import voxel_map_cases as VK
import voxel_map_model as M
from conftest import ROOT
from ouster_sdk_amd import _capi as capi

sys.path.insert(0, os.path.join(ROOT, "ouster_sdk_amd", "compat"))


def host_map(points, voxel=K.STEP_VOXEL, max_points=20):
    m = VK.CapiMap(capi, None, voxel, 100.0, max_points, host=True)
    m.add_points(points)
    return m


@pytest.mark.parametrize("n, dtype, stride, estimate, max_points", [
    (1, K.F64, 3, False, 20), (255, K.F32, 4, True, 1), (257, K.F64, 7, True, 3), (1025, K.F32, 3, False, 20), (2049, K.F64, 4, True, 3)])
def test_step_ref_equals_the_model(n, dtype, stride, estimate, max_points):
    rows = K.step_rows(n)
    est = K.STEP_ESTIMATE if estimate else None
    moved, p = K.model_step(rows, dtype, est, max_points)
    with host_map(K.step_map_points(), max_points=max_points) as m:
        got = K.Step(capi).run(m.h, rows, dtype, stride, est)
    K.check_step(got, moved, p, "n %d" % n, exact_sums=True)
    assert got["dx"] == p["dx"] and got["next_estimate"] == p["estimate"]


def test_align_equals_the_model_pass_by_pass():
    rows = K.step_rows(300, seed=77)[:294] + np.array([0.03, -0.02, 0.015])      # the ordinary rows, moved by centimetres
    model = K.step_model(20)
    trace = []
    want = R.align(rows, model, 30, 1e-4, K.STEP_MAX_DISTANCE, K.STEP_KERNEL, trace=trace)
    assert 2 <= want[1] <= 30
    with host_map(K.step_map_points()) as m:
        pose, iterations, count, converged = K.align_capi(capi, m.h, rows, max_iterations=30, convergence=1e-4,
                                                          max_distance=K.STEP_MAX_DISTANCE, kernel_scale=K.STEP_KERNEL)
        K.same_bytes(pose, R.matrix(want[0]), "pose")
        assert (iterations, count, converged) == want[1:]
        # the same loop a pass at a time: every pass's rows, sums, dx and estimate
        step, cloud, est = K.Step(capi), rows, None
        for j, p in enumerate(trace):
            got = step.run(m.h, cloud, estimate=est)
            K.same_bytes(got["sums"], np.array(p["sums"]), "pass %d: sums" % j)
            assert got["count"] == p["count"] and got["dx"] == p["dx"] and got["next_estimate"] == p["estimate"]
            cloud, est = got["moved"], got["next_estimate"]
        # the same frame with fewer iterations than it needs: not converged, the pose of that many passes
        pose2, it2, _, conv2 = K.align_capi(capi, m.h, rows, max_iterations=2, max_distance=K.STEP_MAX_DISTANCE, kernel_scale=K.STEP_KERNEL)
        short = R.align(rows, model, 2, 1e-4, K.STEP_MAX_DISTANCE, K.STEP_KERNEL)
        K.same_bytes(pose2, R.matrix(short[0]), "pose after 2 passes")
        assert (it2, conv2) == (2, False)


def test_build_linear_system_ref_is_the_left_fold():
    rng = np.random.default_rng(11)
    s, t = rng.normal(size=(500, 3)), rng.normal(size=(500, 3))
    L = capi.load_hip()
    jtj, jtr = np.full(36, 7.5), np.full(6, 7.5)
    dp = C.POINTER(C.c_double)
    capi.check(L.ouster_hip_build_linear_system_ref(s.ctypes.data_as(dp), t.ctypes.data_as(dp), 500, 0.3, jtj.ctypes.data_as(dp), jtr.ctypes.data_as(dp)))
    _, want_jtj, want_jtr = R.linear_system([R.terms(a, b, 0.3) for a, b in zip(s, t)], R.left_fold)
    K.same_bytes(jtj.reshape(6, 6), np.array(want_jtj), "jtj")
    K.same_bytes(jtr, np.array(want_jtr), "jtr")
    assert not np.triu(jtj.reshape(6, 6), 1).any()                               # the upper triangle stays zero
    capi.check(L.ouster_hip_build_linear_system_ref(None, None, 0, 0.3, jtj.ctypes.data_as(dp), jtr.ctypes.data_as(dp)))
    assert not jtj.any() and not jtr.any()
    from ouster.sdk.mapping import build_linear_system
    pj, pr = build_linear_system(s, t, 0.3)
    K.same_bytes(pj, np.array(want_jtj), "python jtj")
    K.same_bytes(pr, np.array(want_jtr), "python jtr")


def test_identity_for_an_empty_map_no_iterations_and_no_rows():
    rows = K.step_rows(20)
    with VK.CapiMap(capi, None, 0.5, 100.0, 20, host=True) as empty:
        assert K.align_capi(capi, empty.h, rows)[1:] == (0, 0, False)
        K.same_bytes(K.align_capi(capi, empty.h, rows)[0], np.eye(4), "empty map")
    with host_map(K.step_map_points()) as m:
        for kw in (dict(max_iterations=0), dict(max_iterations=-3)):
            pose, it, count, conv = K.align_capi(capi, m.h, rows, **kw)
            K.same_bytes(pose, np.eye(4), str(kw))
            assert (it, count, conv) == (0, 0, False)
        pose, it, count, conv = K.align_capi(capi, m.h, np.zeros((0, 3)))
        K.same_bytes(pose, np.eye(4), "no rows")
        assert (it, count, conv) == (0, 0, False)


def test_refusals_through_the_c_abi():
    L = capi.load_hip()
    rows = np.ascontiguousarray(K.step_rows(20))
    with host_map(K.step_map_points()) as m:
        def call(map_h=m.h, p=rows.ctypes.data, dtype=K.F64, n=20, stride=3, desc=True, **kw):
            d = capi.RegistrationDesc()
            d.max_iterations, d.convergence_criterion, d.max_distance, d.kernel_scale = 5, 1e-4, 0.5, 0.1
            for k, v in kw.items():
                setattr(d, k, v)
            for fn in (L.ouster_hip_registration_align, L.ouster_hip_registration_align_host):
                rc = fn(map_h, p, dtype, n, stride, C.byref(d) if desc else None)
                yield rc, L.ouster_hip_last_error().decode()

        def refused(code, text, **kw):
            for rc, msg in call(**kw):
                assert rc == code and text in msg, (kw, rc, msg)

        inv = capi.ERR_INVALID_ARGUMENT
        refused(inv, "map is NULL", map_h=None)
        refused(inv, "desc is NULL", desc=False)
        refused(inv, "dtype must be F32 or F64", dtype=4)
        refused(inv, "row_stride is smaller than 3", stride=2)
        refused(inv, "NULL pointer", p=None)
        for rc, msg in call(n=2 ** 30 + 1):
            assert rc not in (capi.OK, inv) and "more than 2^30 rows" in msg
        for field in ("max_distance", "kernel_scale", "convergence_criterion"):
            for bad in (-1.0, float("nan"), float("inf")):
                refused(inv, field, **{field: bad})
        refused(inv, "unknown flags", flags=2)
        for rc, _ in call(stride=0):                                           # 0 means 3
            assert rc == capi.OK
        # a step: the same checks, and its own
        io = capi.RegistrationStepIo()
        assert L.ouster_hip_registration_step_ref(m.h, None) == inv
        assert L.ouster_hip_registration_step_ref(m.h, C.byref(io)) == inv     # dtype 0
        io.dtype, io.n, io.points, io.max_distance, io.kernel_scale = K.F64, 0, rows.ctypes.data, 0.5, 0.1
        assert L.ouster_hip_registration_step_ref(m.h, C.byref(io)) == inv and "no rows" in L.ouster_hip_last_error().decode()
        io.n = 20
        assert L.ouster_hip_registration_step_ref(m.h, C.byref(io)) == inv and "NULL pointer" in L.ouster_hip_last_error().decode()
    dp = C.POINTER(C.c_double)
    out = np.zeros(36)
    assert L.ouster_hip_build_linear_system_ref(None, None, 3, 0.1, out.ctypes.data_as(dp), out.ctypes.data_as(dp)) == inv
    assert L.ouster_hip_build_linear_system_ref(None, None, 0, -0.1, out.ctypes.data_as(dp), out.ctypes.data_as(dp)) == inv


def test_refusals_through_python():
    from ouster.sdk.core import VoxelHashMap3d
    from ouster.sdk.mapping import ICPRegistration, build_linear_system
    vm = VoxelHashMap3d(voxel_size=0.5, max_distance=10.0, host=True)
    vm.add_points(np.eye(3))
    reg = ICPRegistration()
    frame = np.eye(3)
    for kw in (dict(max_distance=-1.0, kernel_scale=0.1), dict(max_distance=1.0, kernel_scale=float("nan")),
               dict(max_distance=float("inf"), kernel_scale=0.1)):
        with pytest.raises(ValueError):
            reg.align_points_to_map(frame, vm, **kw)
    with pytest.raises(ValueError, match="convergence_criterion"):
        ICPRegistration(convergence_criterion=-1.0).align_points_to_map(frame, vm, max_distance=1.0, kernel_scale=0.1)
    with pytest.raises(ValueError, match="Nx3"):
        reg.align_points_to_map(np.zeros((3, 4)), vm, max_distance=1.0, kernel_scale=0.1)
    with pytest.raises(ValueError):
        build_linear_system(frame, frame[:2], 0.1)
    with pytest.raises(ValueError):
        build_linear_system(frame, frame, -0.1)


def test_refusals_through_cpp():
    out = cpp_tools.run("registration_snippet", [], timeout=60)
    assert "registration_snippet: ok" in out.stdout


# ---- the reference's python/tests/test_registration.py, written anew, on host maps
def test_registration_defaults():
    from ouster.sdk.mapping import ICPRegistration
    reg = ICPRegistration()
    assert reg.max_num_iterations == 50 and reg.convergence_criterion == 0.0001 and reg.max_num_threads > 0
    assert ICPRegistration(max_num_iterations=5, max_num_threads=3).max_num_threads == 3


def test_identity_on_an_empty_map_through_python():
    from ouster.sdk.core import VoxelHashMap3d
    from ouster.sdk.mapping import ICPRegistration
    frame = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    T = ICPRegistration(max_num_iterations=5).align_points_to_map(frame, VoxelHashMap3d(voxel_size=0.5, max_distance=10.0, host=True),
                                                                  max_distance=1.0, kernel_scale=0.1)
    assert T.shape == (4, 4) and T.dtype == np.float64 and np.array_equal(T, np.eye(4))


def test_shifted_cloud_is_recovered_through_python():
    from ouster.sdk.core import VoxelHashMap3d
    from ouster.sdk.mapping import ICPRegistration
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    vm = VoxelHashMap3d(voxel_size=0.5, max_distance=10.0, host=True)
    vm.add_points(pts)
    shifted = pts + np.array([0.05, 0.02, -0.01])
    T = ICPRegistration(max_num_iterations=20).align_points_to_map(shifted, vm, max_distance=0.5, kernel_scale=0.1)
    assert np.allclose((T[:3, :3] @ shifted.T).T + T[:3, 3], pts, atol=0.05)
    model = M.VoxelHashMap3d(0.5, 10.0)
    model.add_points(pts)
    K.same_bytes(T, R.matrix(R.align(shifted, model, 20, 0.0001, 0.5, 0.1)[0]), "pose")


def test_adaptive_threshold_through_python():
    from ouster.sdk.mapping import AdaptiveThreshold
    t = AdaptiveThreshold(max_range=100.0)
    assert (t.max_range, t.min_motion_threshold, t.compute_threshold()) == (100.0, 0.01, 2.0)
    t, model = AdaptiveThreshold(max_range=100.0, initial_threshold=1.0), R.AdaptiveThreshold(100.0, 1.0)
    dev = np.eye(4)
    dev[:3, 3] = [2.0, 0.0, 0.0]
    t.update_model_deviation(dev)
    model.update_model_deviation(dev)
    assert t.compute_threshold() > 1.0 and t.compute_threshold() == model.compute_threshold()
    rng = np.random.default_rng(4)
    for _ in range(20):                                                        # rotations of every branch, translations, tiny motions
        pose = R.matrix(R.se3_exp(list(rng.normal(scale=0.02, size=3)) + list(rng.normal(scale=rng.choice([1e-4, 0.1, 2.0]), size=3))))
        t.update_model_deviation(pose)
        model.update_model_deviation(pose)
        assert t.compute_threshold() == model.compute_threshold()
    L = capi.load_hip()
    half = np.diag([-1.0, -1.0, 1.0, 1.0])                                       # a half turn: trace <= 0
    got = L.ouster_hip_registration_model_error(half.ctypes.data_as(C.POINTER(C.c_double)), 10.0)
    assert got == (2.0 * 10.0) * math.sin(R.rotation_angle(half[:3, :3]) / 2.0)
