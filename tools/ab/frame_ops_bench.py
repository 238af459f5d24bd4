#!/usr/bin/env python3
"""Timing of the frame_ops kernels on the headline workload's shape: 256 frames of 128 x 2048, planes
generated here with torch and resident in HBM.  A single run: 5 warm-up launches, then 20 timed ones per case between HIP
events on the context's stream (median; min and max beside it).  The clip and invalidate cases are idempotent (a second
launch finds the same pixels to replace), so every timed launch does the same work.  Printed per case: ms and the fraction of
8 TB/s under this byte model, per frame, with f = the fraction of pixels invalidated (measured on the data used):
    clip u32            h*w*4 B read + f' * h*w*4 B written   (f': 16-byte chunks holding a replaced value)
    filter_field        key h*w*4 B read + f * h*w*(4 + 2 + 1) B written to the u32 + u16 + u8 targets; targets never read
    filter_uv v         no pixel read at all: f * h*w*(4 + 2 + 1) B written
    mask                h*w*1 B read + f * h*w*(4 + 2 + 1) B written
    filter_xyz          one float of every 12-byte point is USED (h*w*4 B) but every line of the cloud is touched: h*w*12 B,
                        + f * h*w*(4 + 2 + 1) B written
    select_rows u32     2 * (h/2)*w*4 B
and, for context, the standalone destagger of the same u32 plane (same process, same shape; 2 * h*w*4 B): the yardstick.
Prints one JSON line."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PEAK = 8e12
N, H, W, WARM, REPS = 256, 128, 2048, 5, 20


def main():
    import torch
    from ouster_sdk_amd import _capi as capi
    assert torch.cuda.is_available(), "frame_ops_bench needs a GPU"
    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream=stream.cuda_stream)
    L = ctx.L
    g = torch.Generator(device="cuda").manual_seed(1)
    rng = torch.randint(0, 100000, (N, H, W), device="cuda", generator=g, dtype=torch.int32)   # u32 range, mm
    key = rng.clone()
    nir = torch.randint(0, 30000, (N, H, W), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
    refl = torch.randint(0, 255, (N, H, W), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
    masks = (torch.rand((2, H, W), device="cuda", generator=g) > 0.1).to(torch.uint8)
    xyz = torch.randn((N, H * W, 3), device="cuda", generator=g) * 20.0
    dst = torch.empty_like(rng)
    sel = torch.empty((N, H // 2, W), device="cuda", dtype=torch.int32)
    shifts = (C.c_int32 * H)(*[[24, 8, -8, -24][i % 4] for i in range(H)])
    targets = capi.fops_planes([rng.data_ptr(), nir.data_ptr(), refl.data_ptr()], [capi.U32, capi.U16, capi.U8], 0)
    clip_plane = capi.fops_planes([rng.data_ptr()], [capi.U32], 0)
    tbytes = 4 + 2 + 1
    px = H * W

    def pred(**kw):
        return capi.FopsPred(**kw)
    p_key = pred(kind=capi.FOPS_PRED_KEY, src_type=capi.U32, src=key.data_ptr(), lower=0.0, upper=10000.0)
    p_cols = pred(kind=capi.FOPS_PRED_COLS, lo=0, hi=W // 10, shifts=C.cast(shifts, C.c_void_p).value, n_shift_tables=1)
    p_mask = pred(kind=capi.FOPS_PRED_MASK, src=masks.data_ptr(), n_masks=2)
    p_xyz = pred(kind=capi.FOPS_PRED_XYZ, src_type=capi.F32, src=xyz.data_ptr(), axis=2, lower=-3.0, upper=3.0)
    f_key = float((key <= 10000).float().mean())
    f_cols = 0.1
    f_mask = float((masks == 0).float().mean())
    f_xyz = float(((xyz[:, :, 2] >= -3) & (xyz[:, :, 2] <= 3)).float().mean())
    f_clip = float(((rng < 1000) | (rng > 90000)).float().mean())
    idx = (C.c_uint32 * (H // 2))(*range(0, H, 2))
    vp = C.c_void_p * 1

    def inval(p):
        return lambda: L.ouster_hip_frame_ops_invalidate(ctx.h, C.byref(p), targets, 3, N, H, W)
    calls = {
        "clip_u32": lambda: L.ouster_hip_frame_ops_clip(ctx.h, clip_plane, 1, N, H, W, 1000.0, 90000.0),
        "filter_field": inval(p_key),
        "filter_uv_v": inval(p_cols),
        "mask": inval(p_mask),
        "filter_xyz": inval(p_xyz),
        "select_rows_u32": lambda: L.ouster_hip_frame_ops_select_rows(ctx.h, vp(key.data_ptr()), vp(sel.data_ptr()), (C.c_uint32 * 1)(4),
                                                                      1, N, H, W, idx, H // 2),
        "destagger_u32": lambda: L.ouster_hip_destagger(ctx.h, key.data_ptr(), dst.data_ptr(), H, W, 4, shifts, H, 0, N),
    }
    model = {   # clip: a chunk of four u32 is rewritten when any of the four is replaced
        "clip_u32": px * 4 + (1 - (1 - f_clip) ** 4) * px * 4,
        "filter_field": px * 4 + f_key * px * tbytes,
        "filter_uv_v": f_cols * px * tbytes,
        "mask": px + f_mask * px * tbytes,
        "filter_xyz": px * 12 + f_xyz * px * tbytes,
        "select_rows_u32": 2 * (H // 2) * W * 4,
        "destagger_u32": 2 * px * 4,
    }
    torch.cuda.synchronize()
    res = {}
    with torch.cuda.stream(stream):
        for name, call in calls.items():
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
            t = ms[len(ms) // 2]
            res[name] = {"ms": round(t, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
                         "model_bytes_per_frame": int(model[name]), "frac_8TBps": round(model[name] * N / (t * 1e-3) / PEAK, 4)}
    print(json.dumps({"what": "frame_ops, %d frames of %d x %d, targets u32 + u16 + u8, median of %d after %d warm-ups" % (N, H, W, REPS, WARM),
                      "invalidated_fraction": {"clip": round(f_clip, 4), "filter_field": round(f_key, 4), "filter_uv_v": f_cols,
                                               "mask": round(f_mask, 4), "filter_xyz": round(f_xyz, 4)}, **res}))


if __name__ == "__main__":
    main()
