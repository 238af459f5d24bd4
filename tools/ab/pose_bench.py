#!/usr/bin/env python3
"""Timing of interp_pose per column on the headline workload's shape: 256 frames x 2048 columns, timestamps
and status generated here and resident in HBM, a trajectory of 33 known poses spanning the batch.  A single run: 5 warm-up
launches, then 20 timed ones between HIP events on the context's stream (median; min and max beside it).
    interp_columns     ouster_hip_interp_pose_columns, what DeviceFrameBatch::interp_poses queues: the table upload (6.6 KB) and
                       one kernel that reads 12 B and writes 128 B + 48 B per valid column -- once in the default form (a
                       workgroup's rows staged in LDS, lane-linear stores) and once with the knob "pose_direct" (every lane
                       stores its own row).  moved_per_s counts bytes read + written; fraction_of_copy_rate divides it by
                       COPY_RATE, the 6.29 TB/s a float4 copy moves on this device.
    upload_route_emulated   NOT DeviceFrameBatch::upload_poses itself (the Python module does not expose the batch) but the copies
                       that method makes, issued through torch: per frame one synchronous copy of w x 16 doubles from pageable
                       memory, the conversion of rows 0..2 to float on the host, one copy of w x 12 floats; the poses are
                       computed BEFOREHAND.  A lower bound of the host route: the download of timestamps and status and the
                       host's own interpolation (an SE(3) exponential per column on one core) are not in it.
    host_wall          wall-clock of one interp_columns call including the host half (validation, log / inverse per segment).
Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
COPY_RATE = 6.29e12   # bytes moved per second by a float4 copy (read + write)
N, W, K, WARM, REPS = 256, 2048, 33, 5, 20


def main():
    import torch
    from ouster_sdk_amd import _capi as capi
    assert torch.cuda.is_available(), "pose_bench needs a GPU"
    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream=stream.cuda_stream)
    L = ctx.L
    t0 = 1_700_000_000_000_000_000
    ts = t0 + np.arange(N, dtype=np.int64)[:, None] * 100_000_000 + np.arange(W, dtype=np.int64)[None, :] * (100_000_000 // W)
    status = np.ones((N, W), np.int32)
    status[:, ::97] = 0   # a percent of the columns invalid: their rows are skipped
    d_ts, d_st = torch.from_numpy(ts).cuda(), torch.from_numpy(status).cuda()
    d_poses = torch.zeros((N, W, 16), dtype=torch.float64, device="cuda")
    d_rows = torch.zeros((N, W, 12), dtype=torch.float32, device="cuda")
    xk = t0 * 1e-9 - 0.05 + np.arange(K) * (N * 0.1 + 0.1) / (K - 1)
    rng = np.random.default_rng(5)
    poses, rot = [], np.eye(3)
    for i in range(K):
        a = rng.uniform(0.05, 0.4)
        c, s = np.cos(a), np.sin(a)
        rot = rot @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = rot, rng.uniform(-1e3, 1e3, 3)
        poses.append(m.reshape(16))
    poses = np.array(poses)

    def launch():
        capi.check(L.ouster_hip_interp_pose_columns(ctx.h, d_ts.data_ptr(), d_st.data_ptr(), N, W, xk.ctypes.data,
                                                    poses.ctypes.data, K, d_poses.data_ptr(), d_rows.data_ptr()))

    def timed(fn):
        with torch.cuda.stream(stream):
            for _ in range(WARM):
                fn()
            ms = []
            for _ in range(REPS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                fn()
                b.record(stream)
                b.synchronize()
                ms.append(a.elapsed_time(b))
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    n_valid = int(status.sum())
    written = n_valid * (128 + 48)
    moved = written + N * W * 4 + n_valid * 8   # every status word, the timestamps of the valid columns
    forms = {}
    for name, knob in (("lds_transposed", 0), ("direct", 1)):
        ctx.set_knob("pose_direct", knob)
        med, lo, hi = timed(launch)
        forms[name] = {"ms": {"median": med, "min": lo, "max": hi}, "written_per_s": written / (med * 1e-3),
                       "moved_per_s": moved / (med * 1e-3), "fraction_of_copy_rate": moved / (med * 1e-3) / COPY_RATE}
    ctx.set_knob("pose_direct", 0)
    walls = []
    for _ in range(REPS):
        ctx.sync()
        t = time.perf_counter()
        launch()
        ctx.sync()
        walls.append((time.perf_counter() - t) * 1e3)

    ctx.sync()
    host_poses = d_poses.cpu().numpy()   # "computed beforehand"

    def upload_route():
        for f in range(N):
            d_poses[f].copy_(torch.from_numpy(host_poses[f]))
            rows = host_poses[f][:, :12].astype(np.float32)
            d_rows[f].copy_(torch.from_numpy(rows))
    for _ in range(2):
        upload_route()
    ups = []
    for _ in range(5):
        torch.cuda.synchronize()
        t = time.perf_counter()
        upload_route()
        torch.cuda.synchronize()
        ups.append((time.perf_counter() - t) * 1e3)
    out = {"shape": [N, W], "known_poses": K, "valid_columns": n_valid,
           "interp_columns": forms, "bytes_written": written, "bytes_moved": moved, "copy_rate": COPY_RATE,
           "host_wall_ms": {"median": float(np.median(walls)), "min": float(min(walls))},
           "upload_route_emulated_ms": {"median": float(np.median(ups)), "min": float(min(ups)), "bytes": N * W * (128 + 48)}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
