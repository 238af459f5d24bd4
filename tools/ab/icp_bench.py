"""Times ICP: ouster_hip_icp_align on clouds resident in HBM beside ouster_hip_icp_align_ref (the plain C++ restatement with
left-fold sums, one core of the same machine), both methods, on clouds the size of a down-sampled 128 x 1024 scan: the golden voxel
rows of tests/golden/icp_voxels.npz (3 482 rows at 1 m) and the same scene resampled to 20 000 rows, each against itself moved by
the small rigid transform of tests/icp_cases.py with 2 mm of noise; max_corr_dist 0.25.  3 warm-up calls, median of 20 whole calls
(a call is synchronous: every pass ends with its read-back and the solve on the host); the host code is timed over 3 calls.  The
phases (ouster_hip_icp_timing: the target grid once, then correspond / median / sums summed over the passes) are taken in 20
further calls of their own, since the events cost the stream time; they do not sum to the whole call, which also holds the launches'
host side, the read-backs and the solves.

    python tools/ab/icp_bench.py            # writes profiles/icp_bench/icp_bench.json
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

WARMUP, CALLS, HOST_CALLS = 3, 20, 3


def clouds():
    import icp_cases as K
    pts, nrm = K.golden_voxels()
    move = K.move_matrix()
    rng = np.random.default_rng(11)
    pick = rng.integers(0, len(pts), 20000)
    dense = pts[pick] + rng.uniform(-0.45, 0.45, (20000, 3))      # the same scene, more rows: jittered copies inside their voxels
    for label, p, n in (("golden_3482", pts, nrm), ("resampled_20000", dense, nrm[pick])):
        tgt = p @ move[:3, :3].T + move[:3, 3] + rng.normal(0.0, K.NOISE, p.shape)
        yield label, np.ascontiguousarray(p), np.ascontiguousarray(n), np.ascontiguousarray(tgt), np.ascontiguousarray(n @ move[:3, :3].T)


def main():
    import torch
    import icp_cases as K
    from ouster_sdk_amd import _capi as capi
    L = capi.load_hip()
    ctx = capi.Context(0)
    rows = []
    for label, src, src_n, tgt, tgt_n in clouds():
        for method in ("point", "plane"):
            normals = (src_n, tgt_n) if method == "plane" else (None, None)
            d, keep = K.make_desc(capi, src, tgt, normals[0], normals[1], None, K.REAL_DIST, 20.0)
            host_ms = []
            for _ in range(HOST_CALLS):
                t0 = time.perf_counter()
                capi.check(L.ouster_hip_icp_align_ref(C.byref(d)))
                host_ms.append((time.perf_counter() - t0) * 1e3)
            host_pose, host_stats = K.desc_pose(d), (d.iterations, d.correspondences)
            tensors = []

            def ptr(a):
                tensors.append(torch.from_numpy(np.array(a)).cuda())
                return tensors[-1].data_ptr()

            d, keep = K.make_desc(capi, src, tgt, normals[0], normals[1], None, K.REAL_DIST, 20.0, ptr=ptr)
            gpu_ms = []
            for i in range(WARMUP + CALLS):
                t0 = time.perf_counter()
                capi.check(L.ouster_hip_icp_align(ctx.h, C.byref(d)))
                if i >= WARMUP:
                    gpu_ms.append((time.perf_counter() - t0) * 1e3)
            capi.check(L.ouster_hip_icp_timing(ctx.h, 1))
            phases = []
            for _ in range(CALLS):
                capi.check(L.ouster_hip_icp_align(ctx.h, C.byref(d)))
                ms = (C.c_float * len(capi.ICP_PHASES))()
                capi.check(L.ouster_hip_icp_phase_ms(ctx.h, ms))
                phases.append(list(ms))
            capi.check(L.ouster_hip_icp_timing(ctx.h, 0))
            phase_ms = {name: round(statistics.median(p[k] for p in phases), 4) for k, name in enumerate(capi.ICP_PHASES)}
            rows.append({"cloud": label, "method": method, "rows": len(src), "passes": int(d.iterations),
                         "correspondences": int(d.correspondences), "same_passes_as_host_ref": (d.iterations, d.correspondences) == host_stats,
                         "max_abs_pose_diff_to_host_ref": float(np.abs(K.desc_pose(d) - host_pose).max()),
                         "gpu_ms_median": round(statistics.median(gpu_ms), 4), "gpu_ms_min": round(min(gpu_ms), 4),
                         "phase_ms_median": phase_ms, "host_ref_ms_median": round(statistics.median(host_ms), 3)})
            print(rows[-1], flush=True)
    ctx.close()
    out_dir = os.path.join(ROOT, "profiles", "icp_bench")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "icp_bench.json"), "w") as f:
        json.dump({"dtype": "f64", "max_corr_dist": K.REAL_DIST, "warmup": WARMUP, "calls": CALLS, "host_calls": HOST_CALLS,
                   "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
