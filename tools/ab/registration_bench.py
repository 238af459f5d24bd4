"""Times ICPRegistration against the resident voxel map, three routes in alternation in one process:
  (a) what a caller could do before ouster_hip_registration_align existed: per pass ouster_hip_voxel_map_closest on the moved cloud
      in HBM, download of the neighbours and squared distances, ouster_hip_build_linear_system_ref over the correspondences and the
      solve on the host (solve6 / se3_exp / compose of tests/registration_model.py), the cloud moved on the host and uploaded again;
  (b) ouster_hip_registration_align on rows resident in HBM;
  (c) the same call on a map made with OUSTER_HIP_VOXEL_MAP_HOST (csrc/host/registration_util.cpp, one core of the same machine).

Scenario: the map of tools/ab/voxel_map_bench.py (voxel 0.5, 20 points per voxel, max_distance 60; eight frames of 131 072 rows
uniform in +-40 m); the frame is 131 072 of the map's own points with 1 cm of noise, moved by a few centimetres and 0.7 degrees;
max_distance = 3 sigma, kernel_scale = sigma / 3 with sigma = 2 (a fresh AdaptiveThreshold); up to 50 passes, criterion 1e-4.
2 warm-up calls, median of 10 whole calls for (a) and (b); 2 calls for (c).  Every call is synchronous.

    python tools/ab/registration_bench.py         # writes profiles/registration_bench/registration_bench.json
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, EXTENT, VOXEL, MAX_DISTANCE, MAX_POINTS = 131072, 40.0, 0.5, 60.0, 20
BUILD_FRAMES, WARMUP, CALLS, HOST_CALLS = 8, 2, 10, 2
MOTION = [0.04, -0.03, 0.02, 0.006, -0.004, 0.01]
SIGMA, ITERATIONS, CONVERGENCE = 2.0, 50, 1e-4
# tests/registration_cases.py: the largest pose difference between left-fold and exact sums, and icp_cases.pose_margin of it
MEASURED_POSE_DIFFERENCE = 8.743006318923108e-16


def main():
    import torch
    import registration_model as R
    from ouster_sdk_amd import _capi as capi
    L = capi.load_hip()
    ctx = capi.Context(0)
    rng = np.random.default_rng(42)
    max_distance, kernel = 3.0 * SIGMA, SIGMA / 3.0
    bound = max_distance * max_distance
    dp = C.POINTER(C.c_double)

    def make(host):
        d = capi.VoxelMapDesc(VOXEL, MAX_DISTANCE, MAX_POINTS, 1, 0, capi.VOXEL_MAP_HOST if host else 0, 0)
        h = C.c_void_p()
        capi.check(L.ouster_hip_voxel_map_create(None if host else ctx.h, C.byref(d), C.byref(h)))
        return h

    gpu, host = make(False), make(True)
    capi.check(L.ouster_hip_voxel_map_reserve(gpu, 3 << 20))
    for _ in range(BUILD_FRAMES):
        rows = rng.uniform(-EXTENT, EXTENT, (N, 3))
        dev = torch.from_numpy(rows).cuda()
        capi.check(L.ouster_hip_voxel_map_add_points(gpu, dev.data_ptr(), capi.F64, N, 3))
        capi.check(L.ouster_hip_voxel_map_add_points(host, rows.ctypes.data, capi.F64, N, 3))
    i = capi.VoxelMapInfo()
    capi.check(L.ouster_hip_voxel_map_info_read(gpu, C.byref(i)))
    held = {n: int(getattr(i, n)) for n, _ in capi.VoxelMapInfo._fields_}
    cloud = torch.empty((held["points"], 3), dtype=torch.float64, device="cuda")
    n_out = C.c_uint64()
    capi.check(L.ouster_hip_voxel_map_pointcloud(gpu, cloud.data_ptr(), held["points"], C.byref(n_out)))
    pts = cloud.cpu().numpy()[rng.choice(held["points"], N, replace=False)] + rng.normal(scale=0.01, size=(N, 3))
    T = R.matrix(R.se3_exp([-c for c in MOTION]))
    frame = np.ascontiguousarray(pts @ T[:3, :3].T + T[:3, 3])
    frame_dev = torch.from_numpy(frame).cuda()
    nn_dev, d2_dev = torch.empty((N, 3), dtype=torch.float64, device="cuda"), torch.empty(N, dtype=torch.float64, device="cuda")

    def route_a():
        moved, moved_dev, pose, passes, count = frame.copy(), frame_dev.clone(), R.IDENTITY, 0, 0
        jtj, jtr = np.zeros(36), np.zeros(6)
        for _ in range(ITERATIONS):
            capi.check(L.ouster_hip_voxel_map_closest(gpu, moved_dev.data_ptr(), capi.F64, N, 3, bound, nn_dev.data_ptr(), d2_dev.data_ptr()))
            nn, d2 = nn_dev.cpu().numpy(), d2_dev.cpu().numpy()
            keep = d2 < bound
            s, t = np.ascontiguousarray(moved[keep]), np.ascontiguousarray(nn[keep])
            count = len(s)
            capi.check(L.ouster_hip_build_linear_system_ref(s.ctypes.data_as(dp), t.ctypes.data_as(dp), count, kernel,
                                                            jtj.ctypes.data_as(dp), jtr.ctypes.data_as(dp)))
            dx = R.solve6(jtj.reshape(6, 6).tolist(), jtr.tolist())
            est = R.se3_exp(dx)
            pose = R.compose(est, pose)
            passes += 1
            if R.squared_norm6(dx) < CONVERGENCE * CONVERGENCE:
                break
            E = R.matrix(est)
            moved = moved @ E[:3, :3].T + E[:3, 3]
            moved_dev = torch.from_numpy(moved).cuda()
        return R.matrix(pose), passes, count

    def route_align(map_handle, pointer, fn):
        d = capi.RegistrationDesc()
        d.max_iterations, d.convergence_criterion, d.max_distance, d.kernel_scale = ITERATIONS, CONVERGENCE, max_distance, kernel
        capi.check(fn(map_handle, pointer, capi.F64, N, 3, C.byref(d)))
        return np.array(d.pose[:]).reshape(4, 4), int(d.iterations), int(d.correspondences)

    ms = {"a": [], "b": [], "c": []}
    for k in range(WARMUP + CALLS):
        t0 = time.perf_counter()
        a = route_a()
        t1 = time.perf_counter()
        b = route_align(gpu, frame_dev.data_ptr(), L.ouster_hip_registration_align)
        t2 = time.perf_counter()
        if k >= WARMUP:
            ms["a"].append((t1 - t0) * 1e3)
            ms["b"].append((t2 - t1) * 1e3)
    for _ in range(HOST_CALLS):
        t0 = time.perf_counter()
        c = route_align(host, frame.ctypes.data, L.ouster_hip_registration_align_host)
        ms["c"].append((time.perf_counter() - t0) * 1e3)
    margin = max(8.0 * MEASURED_POSE_DIFFERENCE, 8.0 * 2.0 ** -52 * max(1.0, float(np.abs(b[0][:3, 3]).max())))
    want = R.matrix(R.se3_exp(MOTION))
    result = {"device": torch.cuda.get_device_name(0), "rows": N, "map": held, "max_distance": max_distance, "kernel_scale": kernel,
              "warmup": WARMUP, "calls": CALLS, "host_calls": HOST_CALLS,
              "passes": {"a": a[1], "b": b[1], "c": c[1]}, "correspondences": {"a": a[2], "b": b[2], "c": c[2]},
              "pose_margin": margin, "pose_a_minus_b": float(np.abs(a[0] - b[0]).max()), "pose_c_minus_b": float(np.abs(c[0] - b[0]).max()),
              "pose_b_minus_motion": float(np.abs(b[0] - want).max())}
    result["a_and_b_within_margin"] = bool(result["pose_a_minus_b"] <= margin)
    for r in ("a", "b", "c"):
        result[r] = {"ms_median": statistics.median(ms[r]), "ms_min": min(ms[r]), "ms_max": max(ms[r])}
    result["a_over_b"] = result["a"]["ms_median"] / result["b"]["ms_median"]
    result["c_over_b"] = result["c"]["ms_median"] / result["b"]["ms_median"]
    result["b_ms_per_pass"] = result["b"]["ms_median"] / max(1, b[1])
    L.ouster_hip_voxel_map_destroy(gpu)
    L.ouster_hip_voxel_map_destroy(host)
    out = os.path.join(ROOT, "profiles", "registration_bench")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "registration_bench.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
