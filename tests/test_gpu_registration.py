"""ICPRegistration on the GPU (csrc/k_registration.hip through ouster_hip_registration_* and the Python face) against
tests/registration_model.py.  A pass: moved rows, flags, neighbours, squared distances and the count bit for bit, with guard rows
behind every output; every sum within (ceil(N / 1024) + 40) * 2^-53 * sum |t| of math.fsum of the model's terms (the bound of
tests/test_gpu_icp.py, for the same tree); dx and the estimate are solve6 and se3_exp of the device's own sums.  The inputs are those
of tests/registration_cases.py, whose preconditions tests/test_registration_cases_cpu.py asserts on the model.

A whole call: the realistic pair of registration_cases.py, seed 1.  The pose tolerance was measured on the model alone as the
largest difference between align(left fold) and align(fsum) over seeds 1 - 5: 8.74e-16 (seed 1: 23 passes, 2380 correspondences;
the table is in registration_cases.py).  The GPU pose must lie within icp_cases.pose_margin of that (8 x, floor 8 * 2^-52 * max(1,
|t|)) of the exact-sum model, with equal iterations, correspondences and converged."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import icp_cases
import registration_cases as K
import registration_model as R
import voxel_map_cases as VK
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


def to_device_of(torch):
    return lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()


def device_map(gpu, points, voxel=K.STEP_VOXEL, max_points=20, max_distance=100.0):
    capi, ctx, torch = gpu
    m = VK.CapiMap(capi, ctx.h, voxel, max_distance, max_points, to_device=to_device_of(torch), from_device=lambda t: t.cpu().numpy())
    m.add_points(points)
    return m


def device_step(gpu):
    capi, _, torch = gpu
    return K.Step(capi, to_device=to_device_of(torch), from_device=lambda t: t.cpu().numpy())


@pytest.fixture(scope="module")
def step_maps(gpu):
    maps = {P: device_map(gpu, K.step_map_points(), max_points=P) for P in (1, 3, 20)}
    yield maps
    for m in maps.values():
        m.close()


def run_and_check(gpu, step_maps, n, dtype, stride, estimate, P):
    rows = K.step_rows(n)
    est = K.STEP_ESTIMATE if estimate else None
    moved, p = K.model_step(rows, dtype, est, P)
    got = device_step(gpu).run(step_maps[P].h, rows, dtype, stride, est)
    K.check_step(got, moved, p, "n %d dtype %d stride %d estimate %d P %d" % (n, dtype, stride, estimate, P), exact_sums=False)
    return rows, got


@pytest.mark.parametrize("n, dtype, stride, estimate, P", [
    (1, K.F64, 3, False, 20), (255, K.F32, 4, True, 1), (256, K.F64, 7, True, 3), (257, K.F32, 3, False, 20), (1023, K.F64, 4, False, 1),
    (1024, K.F32, 7, True, 3), (1025, K.F64, 3, True, 20), (2049, K.F32, 4, False, 3), (4100, K.F64, 7, True, 20), (4100, K.F32, 3, False, 1)])
def test_a_pass_at_every_row_count(gpu, step_maps, n, dtype, stride, estimate, P):
    rows, got = run_and_check(gpu, step_maps, n, dtype, stride, estimate, P)
    if n >= 16 and not estimate:      # the special rows are what their names say on the device too
        flags = [int(got["flags"][K.special_index(n, k)]) for k, _ in K.SPECIAL_ROWS]
        assert flags == [0, 1, 1, 1, 0, 0]
        assert tuple(got["neighbours"][K.special_index(n, "tie_two")]) == K.TWO_POINTS[1]
        assert tuple(got["neighbours"][K.special_index(n, "tie_four")]) == K.FOUR_POINTS[3]
        assert got["dist_sq"][K.special_index(n, "at_bound")] == K.STEP_MAX_DISTANCE ** 2


@pytest.mark.parametrize("P", [1, 3, 20])
@pytest.mark.parametrize("estimate", [False, True])
@pytest.mark.parametrize("dtype, stride", [(K.F32, 3), (K.F32, 4), (K.F32, 7), (K.F64, 3), (K.F64, 4), (K.F64, 7)])
def test_a_pass_of_every_input_form(gpu, step_maps, dtype, stride, estimate, P):
    run_and_check(gpu, step_maps, 1030, dtype, stride, estimate, P)


def test_two_calls_give_identical_bits(gpu, step_maps):
    rows = K.step_rows(4100)
    step = device_step(gpu)
    a = step.run(step_maps[20].h, rows, K.F64, 3, K.STEP_ESTIMATE)
    step.run(step_maps[3].h, K.step_rows(257), K.F32, 4, None)          # another call in between, on the same workspace
    b = step.run(step_maps[20].h, rows, K.F64, 3, K.STEP_ESTIMATE)
    for k in ("moved", "flags", "neighbours", "dist_sq", "sums"):
        K.same_bytes(a[k], b[k], k)
    assert (a["count"], a["dx"], a["next_estimate"]) == (b["count"], b["dx"], b["next_estimate"])


def chain_of_steps(gpu, map_handle, rows, passes, max_distance, kernel_scale):
    """the loop a pass at a time on the device -> (pose, last count)"""
    step, cloud, est, pose, count = device_step(gpu), rows, None, R.IDENTITY, 0
    for _ in range(passes):
        got = step.run(map_handle, cloud, estimate=est, max_distance=max_distance, kernel_scale=kernel_scale)
        cloud, est, count = got["moved"], got["next_estimate"], got["count"]
        pose = R.compose(est, pose)
    return pose, count


def test_whole_call_on_the_realistic_pair(gpu):
    capi, ctx, torch = gpu
    left, exact = K.scene_run(1, False), K.scene_run(1, True)
    # preconditions (tests/test_registration_cases_cpu.py has the rest): equal passes, identical correspondences
    assert left[1] == exact[1] and all(a["flags"] == b["flags"] and a["neighbours"] == b["neighbours"] for a, b in zip(left[4], exact[4]))
    max_distance, kernel_scale = K.scene_parameters()
    frame = np.array(K.scene_frame(1))
    kw = dict(max_iterations=K.SCENE_MAX_ITERATIONS, convergence=K.SCENE_CONVERGENCE, max_distance=max_distance, kernel_scale=kernel_scale)
    with device_map(gpu, K.scene_map_points(), voxel=K.SCENE_VOXEL, max_points=K.SCENE_POINTS) as m:
        t = to_device_of(torch)(frame)
        pose, iterations, count, converged = K.align_capi(capi, m.h, frame, pointer=t.data_ptr(), host=False, **kw)
        want = R.matrix(exact[0])
        margin = icp_cases.pose_margin(K.MEASURED_POSE_DIFFERENCE, want[:3, 3])
        diff = float(np.abs(pose - want).max())
        print("realistic pair: |gpu - exact model| = %.3e, margin %.3e, |gpu - left fold| = %.3e, passes %d, correspondences %d"
              % (diff, margin, float(np.abs(pose - R.matrix(left[0])).max()), iterations, count))
        assert (iterations, count, converged) == exact[1:4]
        assert diff <= margin
        # the call is its own passes: the same loop a step at a time gives the same bits
        chained, last = chain_of_steps(gpu, m.h, frame, iterations, max_distance, kernel_scale)
        K.same_bytes(pose, R.matrix(chained), "align against a chain of steps")
        assert last == count
        # the _host form on foreign (pageable) and on pooled memory, f32 rows with a stride among them
        K.same_bytes(K.align_capi(capi, m.h, frame, **kw)[0], pose, "foreign memory")
        L = capi.load_hip()
        nbytes = frame.size * 8
        base = L.ouster_hip_host_alloc(nbytes, 0)
        assert base and L.ouster_hip_host_is_pinned(base, nbytes)
        try:
            buf = (C.c_char * nbytes).from_address(base)
            np.frombuffer(buf, dtype=np.float64).reshape(frame.shape)[:] = frame
            K.same_bytes(K.align_capi(capi, m.h, frame, pointer=base, **kw)[0], pose, "pooled memory")
            del buf
        finally:
            L.ouster_hip_host_free(base)
        p32 = K.align_capi(capi, m.h, frame, dtype=K.F32, stride=5, **kw)
        w32 = to_device_of(torch)(np.column_stack([frame, np.zeros((len(frame), 2))]).astype(np.float32))
        K.same_bytes(K.align_capi(capi, m.h, frame, dtype=K.F32, stride=5, pointer=w32.data_ptr(), host=False, **kw)[0], p32[0], "f32 stride 5")
        assert np.abs(p32[0] - pose).max() < 1e-4
        # allocation counts stay flat over 20 calls after the first
        before = capi.alloc_stats()
        for _ in range(20):
            K.align_capi(capi, m.h, frame, pointer=t.data_ptr(), host=False, max_iterations=2, max_distance=max_distance, kernel_scale=kernel_scale)
        after = capi.alloc_stats()
        assert after["device_allocs"] == before["device_allocs"] and after["pinned_allocs"] == before["pinned_allocs"]


def test_python_face(gpu):
    capi, ctx, torch = gpu
    from ouster.sdk.core import VoxelHashMap3d
    from ouster.sdk.mapping import ICPRegistration
    rows = K.step_rows(600, seed=31)[:594] + np.array([0.03, -0.02, 0.015])
    vm = VoxelHashMap3d(voxel_size=K.STEP_VOXEL, max_distance=100.0)
    vm.add_points(K.step_map_points())
    T = ICPRegistration(max_num_iterations=30).align_points_to_map(rows, vm, max_distance=K.STEP_MAX_DISTANCE, kernel_scale=K.STEP_KERNEL)
    assert T.shape == (4, 4) and T.dtype == np.float64
    with device_map(gpu, K.step_map_points()) as m:
        pose, iterations, _, _ = K.align_capi(capi, m.h, rows, max_iterations=30, max_distance=K.STEP_MAX_DISTANCE, kernel_scale=K.STEP_KERNEL)
    K.same_bytes(T, pose, "python against the C ABI")
    assert iterations >= 2 and np.abs(T[:3, 3] + [0.03, -0.02, 0.015]).max() < 0.02
    empty = VoxelHashMap3d(voxel_size=0.5, max_distance=10.0)
    assert np.array_equal(ICPRegistration(max_num_iterations=5).align_points_to_map(rows, empty, max_distance=1.0, kernel_scale=0.1), np.eye(4))


def test_a_map_updated_and_evicted_between_two_calls(gpu):
    capi, ctx, torch = gpu
    first = K.step_map_points()[:700]
    second = first[:300] + np.array([9.0, 0.0, 0.0])                   # a second batch further along x
    model = M.VoxelHashMap3d(K.STEP_VOXEL, 6.0, 20)
    model.add_points(first)
    rows = K.step_rows(1500, seed=8)[:1494]
    rows2 = np.vstack([rows[:700], rows[700:] + np.array([9.0, 0.0, 0.0])])
    step = device_step(gpu)

    def check(m, cloud, what):
        moved = [tuple(float(c) for c in p) for p in cloud]
        p = R.one_pass(moved, K.STEP_ESTIMATE, model, K.STEP_MAX_DISTANCE, K.STEP_KERNEL)
        got = step.run(m.h, cloud, estimate=K.STEP_ESTIMATE)
        K.check_step(got, np.array(moved), p, what, exact_sums=False)
        return p["count"]

    with device_map(gpu, first, max_distance=6.0) as m:
        before = check(m, rows2, "before the update")
        voxels = model.num_voxels()
        position = (9.0, 0.0, 0.0)
        m.update(second, position)
        model.update(second, position)
        assert model.pointcloud()[:, 0].min() > 2.0 and voxels > 300                                # voxels were evicted
        assert m.info()["voxels"] == model.num_voxels()
        after = check(m, rows2, "after the update")
        assert after != before
        a = K.align_capi(capi, m.h, rows2, max_iterations=6, convergence=0.0, max_distance=K.STEP_MAX_DISTANCE, kernel_scale=K.STEP_KERNEL)
        chained, last = chain_of_steps(gpu, m.h, rows2, 6, K.STEP_MAX_DISTANCE, K.STEP_KERNEL)
        K.same_bytes(a[0], R.matrix(chained), "align on the updated map against a chain of steps")
        assert a[1:] == (6, last, False)


def test_refusals_come_before_the_gpu_and_identity_needs_no_launch(gpu):
    capi, ctx, torch = gpu
    L = capi.load_hip()
    rows = K.step_rows(20)
    with device_map(gpu, K.step_map_points()) as m:
        for kw in (dict(max_distance=-1.0), dict(kernel_scale=float("nan")), dict(convergence=float("inf")), dict(stride=2), dict(dtype=4),
                   dict(flags=2)):
            with pytest.raises(ValueError):
                K.align_capi(capi, m.h, rows, **kw)
        for kw in (dict(max_iterations=0), dict(max_iterations=-1)):
            pose, it, count, conv = K.align_capi(capi, m.h, rows, **kw)
            assert np.array_equal(pose, np.eye(4)) and (it, count, conv) == (0, 0, False)
        assert np.array_equal(K.align_capi(capi, m.h, np.zeros((0, 3)))[0], np.eye(4))
        # nothing within reach: dx = 0 after one pass, the identity, converged
        pose, it, count, conv = K.align_capi(capi, m.h, rows[:10] + 500.0, max_distance=0.5)
        assert np.array_equal(pose, np.eye(4)) and (it, count, conv) == (1, 0, True)
    capi_map = VK.CapiMap(capi, ctx.h, 0.5, 100.0, 20)
    with capi_map as empty:
        assert K.align_capi(capi, empty.h, rows)[1:] == (0, 0, False)
