#!/usr/bin/env python3
"""Timing of algorithm::normals on the headline workload's shape: 256 frames of 128 x 2048, dual return, clouds
and ranges resident in HBM (one synthetic frame -- a tilted plane and a sphere, a tenth of the pixels without range -- repeated),
staggered inputs with a shift table, pixel_search_range 1 and 3, f64 and f32 clouds.  A single run: 3 warm-up calls, then 20
timed ones between HIP events on the context's stream (median; min and max beside it).  A call is ouster_hip_normals as a whole:
the table upload, k_normals_subtent, the 16-byte-per-frame-and-return round trip with the host's acos / tan, the second upload
and k_normals.  bytes_moved counts the inputs once and the outputs once; fraction_of_copy_rate divides bytes_moved / time by
COPY_RATE, the 6.29 TB/s a float4 copy moves on this device.  Prints one JSON line and writes it to
profiles/normals_bench/normals_bench.json."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
COPY_RATE = 6.29e12   # bytes moved per second by a float4 copy (read + write)
N, H, W, WARM, REPS = 256, 128, 2048, 3, 20


def frame(seed=5):
    rng = np.random.default_rng(seed)
    az = 2.0 * np.pi * (np.arange(W) + 0.25) / W
    alt = np.deg2rad(np.linspace(22.0, -22.0, H))
    d = np.stack([np.cos(alt)[:, None] * np.cos(az)[None, :], np.cos(alt)[:, None] * np.sin(az)[None, :],
                  np.sin(alt)[:, None] * np.ones(W)[None, :]], axis=-1)
    n = np.array([0.8, 0.5, 0.33])
    n /= np.linalg.norm(n)
    t_plane = np.minimum(4.0 / np.maximum(np.abs(d @ n), 0.1), 40.0)
    c, r = np.array([2.0, 0.6, 0.1]), 0.9
    b = d @ c
    disc = b * b - (c @ c - r * r)
    t_sphere = np.where(disc > 0, b - np.sqrt(np.maximum(disc, 0)), np.inf)
    hit = (t_sphere > 0) & (t_sphere < t_plane)
    r1 = np.round(np.where(hit, t_sphere, t_plane) * 1000.0).astype(np.uint32)
    r2 = np.where(hit, np.round(t_plane * 1000.0), 0).astype(np.uint32)
    r1[rng.random((H, W)) < 0.1] = 0
    r2[rng.random((H, W)) < 0.1] = 0
    return (r1 * 0.001)[..., None] * d, r1, (r2 * 0.001)[..., None] * d, r2


def main():
    import torch
    from ouster_sdk_amd import _capi as capi
    assert torch.cuda.is_available(), "normals_bench needs a GPU"
    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream=stream.cuda_stream)
    xyz, r1, xyz2, r2 = frame()
    shifts = np.ascontiguousarray(np.round(np.linspace(-40, 40, H)), np.int32)
    d_r1 = torch.from_numpy(r1).cuda().unsqueeze(0).repeat(N, 1, 1).contiguous()
    d_r2 = torch.from_numpy(r2).cuda().unsqueeze(0).repeat(N, 1, 1).contiguous()
    d_out = torch.empty((2, N, H * W, 3), dtype=torch.float64, device="cuda")
    results = {}
    for name, dt, es in (("f64", torch.float64, 8), ("f32", torch.float32, 4)):
        d_x1 = torch.from_numpy(xyz).cuda().to(dt).reshape(1, H * W, 3).repeat(N, 1, 1).contiguous()
        d_x2 = torch.from_numpy(xyz2).cuda().to(dt).reshape(1, H * W, 3).repeat(N, 1, 1).contiguous()
        d = capi.NormalsDesc()
        d.xyz, d.range, d.xyz2, d.range2 = d_x1.data_ptr(), d_r1.data_ptr(), d_x2.data_ptr(), d_r2.data_ptr()
        d.normals, d.normals2 = d_out[0].data_ptr(), d_out[1].data_ptr()
        d.pixel_shift_by_row = shifts.ctypes.data
        d.xyz_rows = d.xyz2_rows = H * W
        d.n_frames, d.h, d.w, d.range2_h, d.range2_w = N, H, W, H, W
        d.xyz_dtype, d.staggered_output = capi.F64 if es == 8 else capi.F32, 1
        d.min_angle_of_incidence_rad, d.target_distance_m = np.pi / 180.0, 0.025
        moved = N * H * W * 2 * (3 * es + 4 + 24)
        for psr in (1, 3):
            d.pixel_search_range = psr
            ms = []
            with torch.cuda.stream(stream):
                for i in range(WARM + REPS):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    capi.check(ctx.L.ouster_hip_normals(ctx.h, C.byref(d)))
                    b.record(stream)
                    b.synchronize()
                    if i >= WARM:
                        ms.append(a.elapsed_time(b))
            med = float(np.median(ms))
            results["%s_psr%d" % (name, psr)] = {"ms": {"median": med, "min": float(min(ms)), "max": float(max(ms))},
                                                 "bytes_moved": moved, "moved_per_s": moved / (med * 1e-3),
                                                 "fraction_of_copy_rate": moved / (med * 1e-3) / COPY_RATE}
        del d_x1, d_x2
    ctx.close()
    out = {"shape": [N, H, W], "returns": 2, "staggered_inputs": True, "tile": [4, 64], "copy_rate": COPY_RATE, "calls": results}
    line = json.dumps(out)
    print(line)
    dest = os.path.join(ROOT, "profiles", "normals_bench")
    os.makedirs(dest, exist_ok=True)
    with open(os.path.join(dest, "normals_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
