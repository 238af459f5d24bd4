"""Times the resident voxel map: ouster_hip_voxel_map_update and ouster_hip_voxel_map_closest on rows resident in HBM beside the
same calls on a map made with OUSTER_HIP_VOXEL_MAP_HOST (csrc/host/voxel_map_util.cpp, one core of the same machine).  Both maps
get the same calls and their outputs are compared bitwise in the run.

Scenario: voxel 0.5, 20 points per voxel, max_distance 60; eight frames of 131 072 rows uniform in +-40 m make a map of about a
million points; then `update` of a further 131 072-row frame per call, the position moving 0.25 m each time (so every call evicts),
and `closest` of 131 072 queries with a bound of 1 m.  3 warm-up calls, median of 20 whole calls (each call is synchronous: it
ends with its read-back).  There are no phase times: ouster_hip_voxel_map_timing / _phase_ms are not built.

    python tools/ab/voxel_map_bench.py            # writes profiles/voxel_map_bench/voxel_map_bench.json
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

N, EXTENT, VOXEL, MAX_DISTANCE, MAX_POINTS, BOUND_SQ = 131072, 40.0, 0.5, 60.0, 20, 1.0
BUILD_FRAMES, WARMUP, CALLS = 8, 3, 20


def main():
    import torch
    from ouster_sdk_amd import _capi as capi
    L = capi.load_hip()
    ctx = capi.Context(0)
    rng = np.random.default_rng(42)

    def make(host):
        d = capi.VoxelMapDesc(VOXEL, MAX_DISTANCE, MAX_POINTS, 1, 0, capi.VOXEL_MAP_HOST if host else 0, 0)
        h = C.c_void_p()
        capi.check(L.ouster_hip_voxel_map_create(None if host else ctx.h, C.byref(d), C.byref(h)))
        return h

    def info(h):
        i = capi.VoxelMapInfo()
        capi.check(L.ouster_hip_voxel_map_info_read(h, C.byref(i)))
        return {n: int(getattr(i, n)) for n, _ in capi.VoxelMapInfo._fields_}

    gpu, host = make(False), make(True)
    capi.check(L.ouster_hip_voxel_map_reserve(gpu, 3 << 20))
    frames = [rng.uniform(-EXTENT, EXTENT, (N, 3)) for _ in range(BUILD_FRAMES + WARMUP + CALLS)]
    queries = rng.uniform(-EXTENT, EXTENT, (N, 3))
    pos = np.zeros(3)
    ms = {"update": {"gpu": [], "host": []}, "closest": {"gpu": [], "host": []}}
    q_dev = torch.from_numpy(queries).cuda()
    nn_dev, d2_dev = torch.empty((N, 3), dtype=torch.float64, device="cuda"), torch.empty(N, dtype=torch.float64, device="cuda")
    nn_host, d2_host = np.empty((N, 3)), np.empty(N)
    for k, rows in enumerate(frames):
        o = (C.c_double * 3)(*pos)
        dev = torch.from_numpy(rows).cuda()
        t0 = time.perf_counter()
        capi.check(L.ouster_hip_voxel_map_update(gpu, dev.data_ptr(), capi.F64, N, 3, o))
        t1 = time.perf_counter()
        capi.check(L.ouster_hip_voxel_map_update(host, rows.ctypes.data, capi.F64, N, 3, o))
        t2 = time.perf_counter()
        if k >= BUILD_FRAMES + WARMUP:
            ms["update"]["gpu"].append((t1 - t0) * 1e3)
            ms["update"]["host"].append((t2 - t1) * 1e3)
        if k >= BUILD_FRAMES:
            pos = pos + np.array([0.25, 0.0, 0.0])
    held = info(gpu)
    assert held["voxels"] == info(host)["voxels"] and held["points"] == info(host)["points"], (held, info(host))
    for k in range(WARMUP + CALLS):
        t0 = time.perf_counter()
        capi.check(L.ouster_hip_voxel_map_closest(gpu, q_dev.data_ptr(), capi.F64, N, 3, BOUND_SQ, nn_dev.data_ptr(), d2_dev.data_ptr()))
        t1 = time.perf_counter()
        if k >= WARMUP:
            ms["closest"]["gpu"].append((t1 - t0) * 1e3)
    for k in range(3):
        t0 = time.perf_counter()
        capi.check(L.ouster_hip_voxel_map_closest(host, queries.ctypes.data, capi.F64, N, 3, BOUND_SQ, nn_host.ctypes.data, d2_host.ctypes.data))
        ms["closest"]["host"].append((time.perf_counter() - t0) * 1e3)
    same = nn_dev.cpu().numpy().tobytes() == nn_host.tobytes() and d2_dev.cpu().numpy().tobytes() == d2_host.tobytes()
    cloud_dev = torch.empty((held["points"], 3), dtype=torch.float64, device="cuda")
    cloud_host = np.empty((held["points"], 3))
    n = C.c_uint64()
    capi.check(L.ouster_hip_voxel_map_pointcloud(gpu, cloud_dev.data_ptr(), held["points"], C.byref(n)))
    capi.check(L.ouster_hip_voxel_map_pointcloud(host, cloud_host.ctypes.data, held["points"], C.byref(n)))
    same = same and cloud_dev.cpu().numpy().tobytes() == cloud_host.tobytes()
    result = {"device": torch.cuda.get_device_name(0), "rows_per_call": N, "map": held, "hit_fraction": float((d2_host < BOUND_SQ).mean()),
              "outputs_bitwise_equal": bool(same), "warmup": WARMUP, "calls": CALLS, "host_closest_calls": 3, "phases": "not built"}
    for what in ("update", "closest"):
        g, h = statistics.median(ms[what]["gpu"]), statistics.median(ms[what]["host"])
        result[what] = {"gpu_ms_median": g, "gpu_ms_min": min(ms[what]["gpu"]), "gpu_ms_max": max(ms[what]["gpu"]),
                        "host_one_core_ms_median": h, "ratio": h / g}
    L.ouster_hip_voxel_map_destroy(gpu)
    L.ouster_hip_voxel_map_destroy(host)
    out = os.path.join(ROOT, "profiles", "voxel_map_bench")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "voxel_map_bench.json"), "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    assert same, "the GPU map and the host map differ"


if __name__ == "__main__":
    main()
