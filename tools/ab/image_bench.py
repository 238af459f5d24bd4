#!/usr/bin/env python3
"""Timing of the display-image path on the headline workload's shape: NEAR_IR (u16 -> f32) of 256 frames of
128 x 2048, one sensor.  A single run: 5 warm-up launches, then 20 timed ones per kernel between HIP events on the context's
stream (median; min and max beside it), inputs resident in HBM.  The three C ABI calls are timed with the arguments
DeviceFrameBatch::render_images gives them (BeamUniformityCorrector in front of AutoExposure: dark counts applied on the
fly), on planes generated here with torch (NEAR_IR-like noise plus a per-row offset), NOT on the headline workload's
decoded packets.  render_images as a whole (three launches + two host round trips + the host state machine; synchronous) is
timed by tests/cpp/image_batch_tool in a child process as WALL time, not with events -- it is what a caller waits for -- on
256 frames decoded from four generated frames in rotation.  Printed per kernel: ms and the fraction of 8 TB/s under this byte model, per frame:
    apply        h*w*(2 + 4) B                               (read u16, write f32)
    dark rows    h*w*2 B + the separate mask pass h*w*2 B    (k_img_colmask + k_img_dark_rows, one call, timed together)
    percentiles  h*w/4*2 B x passes                          (4 digit passes for f32) -- the ALGORITHMIC bytes of the sample;
                 the sampled u16 lie 8 B apart, so every 64 B line of the plane is touched and the memory system moves
                 h*w*2 B x passes: "frac_lines" is computed against that
and, for context, the standalone destagger (u16, same process, same shape; 2 * h*w*2 B): the project's nearest neighbour.
Prints one JSON line."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PEAK = 8e12
N, H, W, WARM, REPS, PASSES = 256, 128, 2048, 5, 20, 4


sys.path.insert(0, os.path.join(ROOT, "tests"))
import cpp_tools  # noqa: E402  (tests/cpp_tools.py builds tests/cpp/image_batch_tool)


def main():
    import torch
    from ouster_sdk_amd import _capi as capi
    assert torch.cuda.is_available(), "image_bench needs a GPU"
    stream = torch.cuda.Stream()
    ctx = capi.Context(0, stream=stream.cuda_stream)
    L = ctx.L
    g = torch.Generator(device="cuda").manual_seed(1)
    planes = torch.randint(20, 220, (N, H, W), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
    planes += (torch.arange(H, device="cuda") % 7).to(torch.int16)[None, :, None]
    dst = torch.empty_like(planes)
    out = torch.empty((N, H, W), dtype=torch.float32, device="cuda")
    med = torch.empty((N, H - 1), dtype=torch.float32, device="cuda")
    ncols = torch.empty(N, dtype=torch.int32, device="cuda")
    dark = (torch.arange(H, device="cuda") % 7).float().repeat(N, 1).contiguous()
    n_pos = torch.empty(N, dtype=torch.int32, device="cuda")
    lo_hi = torch.empty((N, 2), dtype=torch.float32, device="cuda")
    maps_h = (capi.ImageMap * N)()
    for m in maps_h:
        m.mode, m.use_dark, m.sub, m.mul, m.add = capi.IMAGE_MAP_AFFINE, 1, 30.0, 0.8 / 160.0, 0.1
    maps = torch.from_numpy(np.frombuffer(maps_h, dtype=np.uint8).copy()).cuda()
    shifts = (C.c_int32 * H)(*[[24, 8, -8, -24][i % 4] for i in range(H)])
    p = planes.data_ptr()
    calls = {
        "dark_rows": lambda: L.ouster_hip_image_dark_rows(ctx.h, p, capi.U16, capi.F32, N, H, W, 0, med.data_ptr(), ncols.data_ptr()),
        "percentiles": lambda: L.ouster_hip_image_percentiles(ctx.h, p, capi.U16, capi.F32, N, H, W, 0, dark.data_ptr(), 0.1, 0.1,
                                                              n_pos.data_ptr(), lo_hi.data_ptr()),
        "apply": lambda: L.ouster_hip_image_apply(ctx.h, p, capi.U16, out.data_ptr(), capi.F32, N, H, W, 0, 0, dark.data_ptr(),
                                                  maps.data_ptr()),
        "destagger_u16": lambda: L.ouster_hip_destagger(ctx.h, p, dst.data_ptr(), H, W, 2, shifts, H, 0, N),
    }
    px = H * W
    model = {"dark_rows": px * 2 + px * 2, "percentiles": px // 4 * 2 * PASSES, "apply": px * (2 + 4), "destagger_u16": px * 2 * 2}
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
                         "model_bytes_per_frame": model[name], "frac_8TBps": round(model[name] * N / (t * 1e-3) / PEAK, 4)}
    res["percentiles"]["frac_lines"] = round(px * 2 * PASSES * N / (res["percentiles"]["ms"] * 1e-3) / PEAK, 4)
    assert int(n_pos.min()) > 100 and float(out.max()) <= 1.0 and float(out.min()) >= 0.0
    exe, env = cpp_tools.build("image_batch_tool")
    whole = subprocess.run([exe, "time", str(N), "20"], capture_output=True, text=True, env=env, timeout=600)
    res["render_images"] = json.loads(whole.stdout.strip().splitlines()[-1]) if whole.returncode == 0 else {"error": whole.stdout[-300:]}
    print(json.dumps({"what": "display images, NEAR_IR u16 -> f32, %d frames of %d x %d, median of %d after %d warm-ups" % (N, H, W, REPS, WARM),
                      "byte_model": "apply h*w*6; dark rows h*w*2 + mask pass h*w*2; percentiles h*w/4*2 x %d passes "
                                    "(frac_lines: h*w*2 x passes, the lines actually touched)" % PASSES, **res}))


if __name__ == "__main__":
    main()
