#!/usr/bin/env python3
"""Same-process A/A and A/B of two decode variants (a library build, a set of knobs, or both) on the SAME output tensors and the
same two rotated packet copies, as bench.py rotates its inputs: buffer placement differs from process to process by up to 20 %,
so a comparison across processes measures the placement, not the kernel.
usage: ring_ab.py <workload> <frames> A=<spec> B=<spec> [out.json]
  spec = [path/of/lib.so][@knob:value[,knob:value ...]]      (empty path: the product library)
  e.g. ring_ab.py single 256 A=@stream:128,stream_slots:2 B=@stream:128,stream_rows:16,stream_slots:5
Protocol: ALT alternations (default 6) of one block per variant, the order swapped every alternation; a block is one untimed
launch and 30 timed ones.  First A against a second context of A itself (the A/A spread), then A against B.  Outputs of B are
compared byte for byte with A's.  One JSON line on stdout, appended to out.json if given."""
import json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench
from ouster_sdk_amd import _capi
from ouster_sdk_amd.device import HotPath

wl, N = sys.argv[1], int(sys.argv[2])
specs = dict(a.split("=", 1) for a in sys.argv[3:5])
dest = sys.argv[5] if len(sys.argv) > 5 else None
ALT, LAUNCHES = int(os.environ.get("AB_ALT", "6")), 30
prof, bits, chan, dst, xyz = bench.WORKLOADS[wl][:5]
alt, az, shifts, b2l, l2s = bench.synth_calibration()
pool = torch.from_numpy(bench.synth_packets(16, bits=bits, chan=chan)).cuda()
pks = [pool.repeat(N // 16, 1, 1).contiguous() for _ in range(2)]


def make(spec):
    path, _, knobs = spec.partition("@")
    hp = HotPath(prof, bench.H, bench.W, 16, lib=_capi.load_hip(os.path.join(ROOT, path)) if path else None)
    hp.set_pixel_shift_by_row(shifts)
    hp.add_lut(b2l, l2s, az, alt)
    hp.ctx.set_knob("tune", 0)
    for kv in filter(None, knobs.split(",")):
        k, v = kv.split(":")
        hp.ctx.set_knob(k, int(v))
    return hp


hps = {"A": make(specs["A"]), "A2": make(specs["A"]), "B": make(specs["B"])}
out = hps["A"].alloc_outputs(N, destagger=dst, xyz=xyz)
snap = {}
for name, hp in hps.items():
    for t in out.values():
        t.view(torch.uint8).fill_(0x3C)
    for i in range(3):
        hp.decode(pks[i & 1], out)
    torch.cuda.synchronize()
    snap[name] = {k: v.clone() for k, v in out.items() if k != "frame_meta"}
    bad = [k for k, v in snap["A"].items() if not torch.equal(v.view(torch.uint8), snap[name][k].view(torch.uint8))]
    assert not bad, (name, bad)


def block(hp):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    hp.decode(pks[1], out)
    a.record()
    for i in range(LAUNCHES):
        hp.decode(pks[i & 1], out)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / LAUNCHES


def compare(x, y):
    t = {x: [], y: []}
    for r in range(ALT):
        for n in ((x, y) if r % 2 == 0 else (y, x)):
            t[n].append(block(hps[n]))
    mx, my = float(np.median(t[x])), float(np.median(t[y]))
    return {"ms": {x: [round(v, 4) for v in t[x]], y: [round(v, 4) for v in t[y]]}, "median_ms": {x: round(mx, 4), y: round(my, 4)},
            "second_faster_by": round((mx - my) / mx, 4)}


aa, ab = compare("A", "A2"), compare("A", "B")
res = {"workload": wl, "frames": N, "A": specs["A"], "B": specs["B"], "alternations": ALT, "launches_per_block": LAUNCHES,
       "kernels": {n: [h.ctx.last_decode_kernel()] + list(h.ctx.last_decode_tile()) for n, h in hps.items()},
       "A_vs_A": aa, "A_vs_B": ab, "aa_spread": abs(aa["second_faster_by"]), "improvement": ab["second_faster_by"],
       "counts_as_gain": ab["second_faster_by"] >= 2 * abs(aa["second_faster_by"]) and ab["second_faster_by"] > 0,
       "A_TBps": round(bench.algorithmic_bytes_per_frame(wl) * N / (ab["median_ms"]["A"] * 1e-3) / 1e12, 3)}
line = json.dumps(res)
print(line)
if dest:
    with open(dest, "a") as f:
        f.write(line + "\n")
