#!/usr/bin/env python3
"""Timing of the RGB display-image path: LocalToneMapper on 128 x 2048 x 3 images, batches of 1, 16 and 64,
FLOAT16 -> float32 (what a colour sensor's RGB plane needs) and float32 in place.  A single run per batch size: 5 warm-up calls,
then 20 timed ones between HIP events on the context's stream (median; min and max beside it), inputs resident in HBM, log-normal
scenes generated here with torch.  Timed:
    lum_percentiles   ouster_hip_image_lum_percentiles: one workgroup per image, 4 digit passes (f32)
    tonemap           ouster_hip_image_tonemap as a whole: the histogram memset, k_tm_hist, k_tm_luts, k_tm_finish
    apply_rgb         ouster_hip_image_apply on the h x 3w view (k_img_apply), the RGB AutoExposure's streaming pass: the neighbour
    update_batch      LocalToneMapper.update_batch of the Python class as WALL time: upload, percentiles, host state machine,
                      the launch chain, download -- what a caller with host arrays waits for
    bands sweep       `tonemap` FLOAT16 again with k_tm_hist's bands per tile forced to 1, 2, 4, 8, 16 (0: the launch's choice)
Byte model per pixel (table reads come from L2 and are not counted):
    tonemap f16   6 (k_tm_hist reads) + 6 + 12 (k_tm_finish reads, writes) = 24 B     f32 in place   12 + 12 + 12 = 36 B
    apply_rgb     f16 6 + 12 = 18 B
    percentiles   every 4th pixel: 6 / 4 B x 4 passes (algorithmic)
The split of `tonemap` into its kernels comes from a kernel trace of this script (--images N restricts it to one batch size), not
from events: there is no per-kernel entry point.  Prints one JSON line; there is no pass / fail time."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PEAK = 8e12
H, W, WARM, REPS, PASSES = 128, 2048, 5, 20, 4


def timed(torch, capi, stream, call):
    for _ in range(WARM):
        capi.check(call())
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        capi.check(call())
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="*", default=[1, 16, 64])
    ap.add_argument("--no-wall", action="store_true", help="skip the update_batch wall time (kernel traces)")
    args = ap.parse_args()
    import torch
    from ouster_sdk_amd import _capi as capi
    from ouster_sdk_amd import core
    assert torch.cuda.is_available(), "tonemap_bench needs a GPU"
    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream=stream.cuda_stream)
    L = ctx.L
    px = H * W
    res = {}
    for n in args.images:
        g = torch.Generator(device="cuda").manual_seed(n)
        lum = torch.exp(1.3 * torch.randn((n, H, W, 1), device="cuda", generator=g)) * 0.3
        f32 = (lum * (0.4 + 1.2 * torch.rand((n, H, W, 3), device="cuda", generator=g))).contiguous()
        f16 = f32.to(torch.float16).contiguous()
        out = torch.empty_like(f32)
        work = f32.clone()
        n_pos = torch.empty(n, dtype=torch.int32, device="cuda")
        lo_hi = torch.empty((n, 2), dtype=torch.float32, device="cuda")
        recs = (capi.TonemapParams * n)()
        for r in recs:   # a dark scene: affine map, compression on, the colour ramp
            r.map.mode, r.map.sub, r.map.mul, r.map.add = capi.IMAGE_MAP_AFFINE, 0.001, 0.9, 0.0
            r.compress, r.color_correct, r.color_ramp = 1, 1, 0.6
        d_recs = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).cuda()
        d_maps = torch.from_numpy(np.frombuffer(b"".join(bytes(r.map) for r in recs), dtype=np.uint8).copy()).cuda()
        calls = {
            "lum_percentiles_f16": (lambda: L.ouster_hip_image_lum_percentiles(ctx.h, f16.data_ptr(), capi.F16, capi.F32, n, H, W, 0, 0.0, 0.2,
                                                                               n_pos.data_ptr(), lo_hi.data_ptr()), px // 4 * 6 * PASSES),
            "tonemap_f16": (lambda: L.ouster_hip_image_tonemap(ctx.h, f16.data_ptr(), capi.F16, out.data_ptr(), capi.F32, n, H, W, 0, 0,
                                                               d_recs.data_ptr()), px * 24),
            "tonemap_f32_in_place": (lambda: L.ouster_hip_image_tonemap(ctx.h, work.data_ptr(), capi.F32, work.data_ptr(), capi.F32, n, H, W, 0, 0,
                                                                        d_recs.data_ptr()), px * 36),
            "apply_rgb_f16": (lambda: L.ouster_hip_image_apply(ctx.h, f16.data_ptr(), capi.F16, out.data_ptr(), capi.F32, n, H, 3 * W, 0, 0, None,
                                                               d_maps.data_ptr()), px * 18),
        }
        torch.cuda.synchronize()
        row = {}
        with torch.cuda.stream(stream):
            for name, (call, model) in calls.items():
                t, lo, hi = timed(torch, capi, stream, call)
                row[name] = {"ms": round(t, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "model_bytes_per_image": model,
                             "frac_8TBps": round(model * n / (t * 1e-3) / PEAK, 4)}
        assert int(n_pos.min()) > 100 and float(out.max()) <= 1.0 and float(out.min()) >= 0.0
        if not args.no_wall:   # bands of rows per tile in k_tm_hist (knob "tonemap_bands"; 0 = the launch's own choice), whole call
            sweep = {}
            with torch.cuda.stream(stream):
                for bands in (0, 1, 2, 4, 8, 16):
                    ctx.set_knob("tonemap_bands", bands)
                    t, lo, hi = timed(torch, capi, stream, calls["tonemap_f16"][0])
                    sweep["bands_%d" % bands] = {"ms": round(t, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)}
            ctx.set_knob("tonemap_bands", 0)
            row["tonemap_f16_by_bands"] = sweep
        if not args.no_wall:
            host = f16.cpu().numpy()
            ltm = core.LocalToneMapper()
            for _ in range(3):
                ltm.update_batch(host)
            wall = []
            for _ in range(10):
                t0 = time.perf_counter()
                ltm.update_batch(host)
                wall.append((time.perf_counter() - t0) * 1e3)
            wall.sort()
            row["update_batch_wall_f16"] = {"ms": round(wall[len(wall) // 2], 3), "ms_min": round(wall[0], 3), "ms_max": round(wall[-1], 3)}
        res["images_%d" % n] = row
    print(json.dumps({"what": "LocalToneMapper, %d x %d x 3, median of %d after %d warm-ups" % (H, W, REPS, WARM),
                      "byte_model": "tonemap f16 24 B/px, f32 in place 36 B/px; apply_rgb f16 18 B/px; percentiles 6/4 B/px x %d passes" % PASSES,
                      **res}))


if __name__ == "__main__":
    main()
