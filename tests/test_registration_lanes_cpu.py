"""The source of k_reg_pass's thread and of k_reg_fold (csrc/k_registration.hip) run on the CPU, one thread per lane
(tests/cpp/registration_lanes.cpp over tests/cpp/host_lanes), against tests/registration_model.py: moved rows, flags, neighbours,
squared distances and terms bit for bit; every thread's accumulators are the left fold of its rows base + t + 256 k, k = 0..3 (the
thread-to-row mapping); the sums within (ceil(N / 1024) + 40) * 2^-53 * sum |t| of math.fsum of the terms and the count exact.  The
inputs are those of tests/registration_cases.py.  No GPU."""
import math
import struct
import subprocess

import numpy as np
import pytest

import cpp_tools
import registration_cases as K
import registration_model as R


def run_lanes(tmp_path, rows, dtype, stride, estimate, P):
    model = K.step_model(P)
    n = len(rows)
    a = np.full((n, stride), 7.5, dtype=np.float32 if dtype == K.F32 else np.float64)
    with np.errstate(over="ignore"):
        a[:, :3] = rows
    case, result = tmp_path / "case.bin", tmp_path / "result.bin"
    with open(case, "wb") as f:
        f.write(struct.pack("<8I3d7d", n, P, int(estimate is not None), int(dtype == K.F32), stride, model.num_voxels(), 0, 0,
                            model.voxel_size, K.STEP_MAX_DISTANCE, K.STEP_KERNEL, *(estimate if estimate is not None else R.IDENTITY)))
        for cell, bucket in zip(model.cells, model.buckets):
            f.write(struct.pack("<3iI", *cell, len(bucket)))
        pts = np.zeros((model.num_voxels(), P, 3))
        for v, bucket in enumerate(model.buckets):
            pts[v, :len(bucket)] = bucket
        f.write(pts.tobytes())
        f.write(a.tobytes())
    p = subprocess.run([cpp_tools.build("registration_lanes")[0], str(case), str(result)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip() == "registration_lanes: done", (p.returncode, p.stdout, p.stderr)
    raw, at, out = open(result, "rb").read(), 0, {}
    threads = math.ceil(n / 1024) * 256
    for name, count, dt in (("moved", n * 3, np.float64), ("neighbours", n * 3, np.float64), ("dist_sq", n, np.float64),
                            ("terms", n * 16, np.float64), ("acc", threads * 16, np.float64), ("sums", 16, np.float64),
                            ("count", 1, np.uint64), ("thread_count", threads, np.uint32), ("flags", n, np.uint8)):
        out[name] = np.frombuffer(raw, dt, count, at)
        at += count * np.dtype(dt).itemsize
    assert at == len(raw)
    return out


@pytest.mark.parametrize("n, dtype, stride, estimate, P", [
    (1, K.F64, 3, False, 20), (255, K.F32, 4, True, 1), (257, K.F64, 7, True, 3), (1025, K.F32, 3, False, 20), (2049, K.F64, 4, True, 3)])
def test_the_pass_on_the_cpu_equals_the_model(tmp_path, n, dtype, stride, estimate, P):
    rows = K.step_rows(n)
    est = K.STEP_ESTIMATE if estimate else None
    moved, p = K.model_step(rows, dtype, est, P)
    got = run_lanes(tmp_path, rows, dtype, stride, est, P)
    K.same_bytes(got["moved"].reshape(-1, 3), moved, "moved rows", nan_rows=K.non_finite_rows(moved))
    assert got["flags"].tolist() == [int(f) for f in p["flags"]]
    K.same_bytes(got["neighbours"].reshape(-1, 3), np.array(p["neighbours"], dtype=np.float64).reshape(-1, 3), "neighbours")
    K.same_bytes(got["dist_sq"], np.array(p["dist_sq"], dtype=np.float64), "squared distances")
    terms = np.array(p["terms"], dtype=np.float64).reshape(-1, 16)
    K.same_bytes(got["terms"].reshape(-1, 16), terms, "terms")
    # thread t of chunk b folds rows 1024 b + t + 256 k, k = 0..3, in that order, from +0.0
    acc, counts = got["acc"].reshape(-1, 16), got["thread_count"]
    want = np.zeros_like(acc)
    want_counts = np.zeros(len(acc), dtype=np.uint32)
    for b in range(len(acc) // 256):
        for t in range(256):
            for k in range(4):
                i = 1024 * b + t + 256 * k
                if i < n:
                    want[256 * b + t] = want[256 * b + t] + terms[i]
                    want_counts[256 * b + t] += int(p["flags"][i])
    K.same_bytes(acc, want, "the threads' accumulators")
    assert counts.tolist() == want_counts.tolist()
    exact = np.array([math.fsum(terms[:, k]) for k in range(16)])
    err, bound = np.abs(got["sums"] - exact), K.sum_bound(n, p["terms"])
    assert (err <= bound).all(), (err, bound)
    assert int(got["count"][0]) == p["count"]
