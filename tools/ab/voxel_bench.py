"""Times voxel down-sampling: ouster_hip_voxel_downsample on clouds resident in HBM beside ouster_hip_voxel_downsample_ref (the
plain C++ restatement, one core of the same machine), AVERAGE_POINT on f64 (N, 3) clouds.  Shapes: the four scenarios of the
reference's own perf test (tests/voxel_downsample_test.cpp:238-243: points uniform in +-range) and one batch-sized cloud
(32 frames of 128 x 2048 points, uniform in +-100 m at voxel 0.5).  3 warm-up calls, median of 20 whole calls (the call is
synchronous: it ends with its read-back); the host code is timed over 3 calls.  The phases (ouster_hip_voxel_timing: events around
each phase of a call) are taken in 20 further calls of their own, since the events cost the stream time; their medians do not
sum to the whole call, which also holds the launches' host side and the read-back.

    python tools/ab/voxel_bench.py            # writes profiles/voxel_bench/voxel_bench.json
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

SCENARIOS = [
    ("spread", 131072, 0.5, 50.0),
    ("lidar", 131072, 0.5, 7.5),
    ("cluster", 131072, 0.5, 2.5),
    ("big", 524288, 1.0, 250.0),
    ("batch", 32 * 128 * 2048, 0.5, 100.0),
]
WARMUP, CALLS, HOST_CALLS = 3, 20, 3


def main():
    import torch
    from ouster_sdk_amd import _capi as capi
    L = capi.load_hip()
    ctx = capi.Context(0)
    rows = []
    for label, n, voxel_size, extent in SCENARIOS:
        cloud = np.random.default_rng(42).uniform(-extent, extent, (n, 3))
        out_host = np.empty((n, 3))
        d = capi.VoxelDesc()
        d.n, d.cols, d.out_capacity, d.dtype = n, 3, n, capi.F64
        d.voxel_size, d.max_points_per_voxel, d.min_pts_threshold, d.strategy = voxel_size, 1, 1, capi.VOXEL_AVERAGE_POINT
        n_out = C.c_uint64()
        d.points, d.out = cloud.ctypes.data, out_host.ctypes.data
        host_ms = []
        for _ in range(HOST_CALLS):
            t0 = time.perf_counter()
            capi.check(L.ouster_hip_voxel_downsample_ref(C.byref(d), C.byref(n_out)))
            host_ms.append((time.perf_counter() - t0) * 1e3)
        host_rows = n_out.value
        pts, out = torch.from_numpy(cloud).cuda(), torch.empty((n, 3), dtype=torch.float64, device="cuda")
        d.points, d.out = pts.data_ptr(), out.data_ptr()
        gpu_ms = []
        for i in range(WARMUP + CALLS):
            t0 = time.perf_counter()
            capi.check(L.ouster_hip_voxel_downsample(ctx.h, C.byref(d), C.byref(n_out)))
            if i >= WARMUP:
                gpu_ms.append((time.perf_counter() - t0) * 1e3)
        capi.check(L.ouster_hip_voxel_timing(ctx.h, 1))
        phases = []
        for _ in range(CALLS):
            capi.check(L.ouster_hip_voxel_downsample(ctx.h, C.byref(d), C.byref(n_out)))
            ms = (C.c_float * len(capi.VOXEL_PHASES))()
            capi.check(L.ouster_hip_voxel_phase_ms(ctx.h, ms))
            phases.append(list(ms))
        capi.check(L.ouster_hip_voxel_timing(ctx.h, 0))
        phase_ms = {name: round(statistics.median(p[k] for p in phases), 4) for k, name in enumerate(capi.VOXEL_PHASES)}
        same = n_out.value == host_rows and np.array_equal(out[:host_rows].cpu().numpy().view(np.uint64), out_host[:host_rows].view(np.uint64))
        rows.append({"scenario": label, "points": n, "voxel_size": voxel_size, "extent_m": extent, "rows_out": int(host_rows),
                     "gpu_ms_median": round(statistics.median(gpu_ms), 4), "gpu_ms_min": round(min(gpu_ms), 4),
                     "phase_ms_median": phase_ms, "host_ref_ms_median": round(statistics.median(host_ms), 3), "gpu_equals_host_ref_bitwise": bool(same),
                     # input rows read by keys, gather and (first / last forms) write; output rows written
                     "bytes_in_out": n * 24 + int(host_rows) * 24})
        print(rows[-1], flush=True)
    ctx.close()
    out_dir = os.path.join(ROOT, "profiles", "voxel_bench")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "voxel_bench.json"), "w") as f:
        json.dump({"strategy": "AVERAGE_POINT", "dtype": "f64", "warmup": WARMUP, "calls": CALLS, "host_calls": HOST_CALLS,
                   "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
