"""Times the resident ICP target beside the single-call route: K sources against one target that does not change, by three routes
    (a) K calls of ouster_hip_icp_align on device arrays      -- the existing route, the baseline: K grid builds
    (b) one ouster_hip_icp_target_create, then K calls of ouster_hip_icp_target_align with one source each
    (c) one ouster_hip_icp_target_create, then one ouster_hip_icp_target_align of all K sources
on the clouds of tools/ab/icp_bench.py (the golden voxel rows, 3 482, and the same scene resampled to 20 000 rows), both methods,
K = 1, 8, 64 copies of the source, each moved by a small rigid transform of its own; max_corr_dist 0.25.  The create of (b) and (c)
is outside the timed window (it is what the route saves) and reported on its own.  A configuration (cloud, method) is one child
process under a time limit of its own; in it the routes are timed in alternation -- a, a', b, c, round after round, a' being route
(a) again: the A/A spread any difference has to exceed -- after WARMUP rounds, each sample a host clock around 32 / K runs of the route (every call ends in a stream synchronisation),
reported per run.  The results of the three routes are compared bit for bit before anything is timed.

    python tools/ab/icp_target_bench.py            # writes profiles/icp_target_bench/icp_target_bench.json
"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

WARMUP, ROUNDS = 3, 15
KS = (1, 8, 64)
CASE_TIMEOUT_S = 240


def moves(k):
    """K distinct small moves: rotation vectors up to 5 mrad, translations up to 3 cm"""
    rng = np.random.default_rng(7)
    return np.hstack([rng.uniform(-0.005, 0.005, (k, 3)), rng.uniform(-0.03, 0.03, (k, 3))])


def run_case(label, method):
    import torch
    import icp_bench
    import icp_cases as K
    import icp_target_cases as T
    import pose_model as P
    from ouster_sdk_amd import _capi as capi
    L = capi.load_hip()
    src, src_n, tgt, tgt_n = next(c[1:] for c in icp_bench.clouds() if c[0] == label)
    plane = method == "plane"
    ctx = capi.Context(0)
    tensors = []

    def ptr(a):
        tensors.append(torch.from_numpy(np.array(a)).cuda())
        return tensors[-1].data_ptr()

    t0 = time.perf_counter()
    rc, h = T.create(capi, ctx.h, tgt, tgt_n if plane else None, K.REAL_DIST, ptr=ptr, host=False)
    capi.check(rc)
    create_first_ms = (time.perf_counter() - t0) * 1e3
    uploaded = iter([t.data_ptr() for t in tensors] * 5)

    def resident(a):            # the target's arrays are in HBM already: a create is timed without its upload
        return next(uploaded)

    create_ms = []
    for _ in range(5):          # create + destroy of a second handle: what a changed target costs
        t0 = time.perf_counter()
        rc, h2 = T.create(capi, ctx.h, tgt, tgt_n if plane else None, K.REAL_DIST, ptr=resident, host=False)
        capi.check(rc)
        create_ms.append((time.perf_counter() - t0) * 1e3)
        L.ouster_hip_icp_target_destroy(h2)
    rows = []
    for k in KS:
        clouds, normals = [], []
        for mv in moves(k):
            m = np.array(P.pose_exp([float(v) for v in mv]), dtype=np.float64)
            clouds.append(np.ascontiguousarray((src - m[:3, 3]) @ m[:3, :3]))
            normals.append(np.ascontiguousarray(src_n @ m[:3, :3]))
        descs = [K.make_desc(capi, clouds[i], tgt, normals[i] if plane else None, tgt_n if plane else None, None, K.REAL_DIST, 20.0, ptr=ptr)
                 for i in range(k)]
        many, keep_many, tag = T.make_sources(capi, clouds, normals if plane else None, ptr=ptr)
        ones = [T.make_sources(capi, [clouds[i]], [normals[i]] if plane else None, ptr=ptr) for i in range(k)]

        def route_a():
            for d, _ in descs:
                capi.check(L.ouster_hip_icp_align(ctx.h, C.byref(d)))

        def route_b():
            for s, _, t in ones:
                capi.check(L.ouster_hip_icp_target_align(ctx.h, h, s, 1, t, 20.0))

        def route_c():
            capi.check(L.ouster_hip_icp_target_align(ctx.h, h, many, k, tag, 20.0))

        routes = (("a", route_a), ("a2", route_a), ("b", route_b), ("c", route_c))
        ms = {name: [] for name, _ in routes}
        reps = max(1, 32 // k)      # a sample is a window of some ten milliseconds at every K, reported per run of the route
        for i in range(WARMUP + ROUNDS):
            for name, fn in routes:
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                if i >= WARMUP:
                    ms[name].append((time.perf_counter() - t0) * 1e3 / reps)
            if i == 0:          # faster and different is not faster: the three routes give the same bits
                for j in range(k):
                    want = (bytes(descs[j][0].pose), descs[j][0].iterations, descs[j][0].solved, descs[j][0].correspondences)
                    for s in (many[j], ones[j][0][0]):
                        assert (bytes(s.pose), s.iterations, s.solved, s.correspondences) == want, (label, method, k, j)
        med = {name: statistics.median(v) for name, v in ms.items()}
        passes = [int(d.iterations) for d, _ in descs]
        rows.append({"cloud": label, "method": method, "rows": len(src), "k": k, "runs_per_sample": reps, "passes_max": max(passes), "passes_sum": sum(passes),
                     "a_ms_median": round(med["a"], 4), "a_ms_min": round(min(ms["a"]), 4),
                     "a2_ms_median": round(med["a2"], 4), "a2_ms_min": round(min(ms["a2"]), 4),
                     "aa_spread": round(abs(med["a"] - med["a2"]) / min(med["a"], med["a2"]), 4),
                     "b_ms_median": round(med["b"], 4), "b_ms_min": round(min(ms["b"]), 4),
                     "c_ms_median": round(med["c"], 4), "c_ms_min": round(min(ms["c"]), 4),
                     "b_over_a": round(med["b"] / med["a"], 4), "c_over_a": round(med["c"] / med["a"], 4),
                     "create_ms_first": round(create_first_ms, 4), "create_ms_median": round(statistics.median(create_ms), 4)})
        print(json.dumps(rows[-1]), flush=True)
    L.ouster_hip_icp_target_destroy(h)
    ctx.close()
    return {"device": torch.cuda.get_device_name(0), "rows": rows}


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--case":
        print("RESULT " + json.dumps(run_case(sys.argv[2], sys.argv[3])), flush=True)
        return 0
    rows, device = [], None
    for label in ("golden_3482", "resampled_20000"):
        for method in ("point", "plane"):
            # a child of its own under a time limit of its own; after a fault, an abort or a hang nothing more is started
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", label, method], capture_output=True, text=True,
                               timeout=CASE_TIMEOUT_S)
            sys.stdout.write(p.stdout)
            if p.returncode != 0:
                sys.stderr.write(p.stderr)
                return p.returncode
            res = json.loads(next(line for line in p.stdout.splitlines() if line.startswith("RESULT "))[7:])
            rows += res["rows"]
            device = res["device"]
    out_dir = os.path.join(ROOT, "profiles", "icp_target_bench")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "icp_target_bench.json"), "w") as f:
        json.dump({"dtype": "f64", "max_corr_dist": 0.25, "warmup": WARMUP, "rounds": ROUNDS, "device": device,
                   "routes": {"a": "K x ouster_hip_icp_align", "a2": "the same again (A/A)", "b": "K x ouster_hip_icp_target_align of one source",
                              "c": "one ouster_hip_icp_target_align of K sources"}, "rows": rows}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
