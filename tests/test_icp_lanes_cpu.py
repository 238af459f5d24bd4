"""CPU-only: the source of the ICP grid kernels and of k_icp_correspond (csrc/k_icp.hip, over the cell table of csrc/k_voxel.hip)
compiled for the host, one thread per lane (tests/cpp/icp_lanes.cpp over tests/cpp/host_lanes/hip/hip_runtime.h), against
tests/icp_model.py bit for bit: the neighbour index and the residual of every row of the tie cases of tests/icp_cases.py, guard
elements behind both.  Keys, hash insert (real threads race for the slots), ids, segments, slots, gather and correspond are the
library's source; the scan and the stable sort, rocPRIM's on the device, are plain C++ here.  The sum kernels (k_icp_sums_point_a /
_b, k_icp_sums_plane), k_icp_median and k_icp_fold use cross-lane operations or device-only launches and are covered on the GPU only
(tests/test_gpu_icp.py)."""
import struct
import subprocess

import numpy as np
import pytest

import cpp_tools
import icp_cases as K
import icp_model as M


@pytest.fixture(scope="module")
def lanes():
    return cpp_tools.build("icp_lanes")[0]


def run(exe, tmp_path, arrays, pose, max_corr_dist, angle, table_log2=None):
    """-> (status, cells, nn with guard, r with guard)"""
    src, tgt, src_n, tgt_n = arrays["src"], arrays["tgt"], arrays["src_n"], arrays["tgt_n"]
    plane = src_n is not None
    n_src, n_tgt = len(src), len(tgt)
    if table_log2 is None:
        table_log2 = max(1, int(2 * n_tgt - 1).bit_length())
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("<10I", n_src, n_tgt, src.shape[1], tgt.shape[1], src_n.shape[1] if plane else 3, tgt_n.shape[1] if plane else 3,
                            int(src.dtype == np.float32), int(plane), table_log2, 0))
        f.write(struct.pack("<18d", max_corr_dist, M.cos_gate(angle) if plane else 0.0, *np.asarray(pose, dtype=np.float64).reshape(-1)))
        for a in (src, tgt) + ((src_n, tgt_n) if plane else ()):
            f.write(np.ascontiguousarray(a).tobytes())
    subprocess.check_call([exe, case, res], timeout=300)
    raw = open(res, "rb").read()
    status, cells = struct.unpack("<II", raw[:8])
    nn = np.frombuffer(raw[8:8 + 4 * (n_src + 16)], np.int32)
    r = np.frombuffer(raw[8 + 4 * (n_src + 16):], np.float64)
    return status, cells, nn, r


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
@pytest.mark.parametrize("n,variant", [(20, 0), (63, 0), (65, 1), (257, 0), (1041, 1)])
def test_correspondences_equal_the_model_bit_for_bit(lanes, tmp_path, n, plane, variant):
    arrays, pose = K.tie_case(n, plane, variant)
    want = K.tie_model(n, plane, variant)
    for log2 in (None, 9):      # the automatic table and 512 slots for 240 rows: long probe chains
        status, cells, nn, r = run(lanes, tmp_path, arrays, pose, K.CELL, K.tie_gate(n), log2)
        assert status == 0 and cells > 100
        assert (nn[n:] == -77).all() and (r[n:] == -7.25).all()
        assert np.array_equal(nn[:n], want["nn"]), np.flatnonzero(nn[:n] != want["nn"])[:10]
        assert K.same_bits(r[:n], want["r"])


def test_a_target_outside_the_grid_sets_the_status_and_nothing_else(lanes, tmp_path):
    src, tgt, _ = K.published_point()
    n = np.tile([0.0, 0.0, 1.0], (27, 1))
    far = tgt.copy()
    far[3, 1] = 3e9
    for normals in ((None, None), (n, n)):
        status, _, nn, r = run(lanes, tmp_path, dict(src=src, tgt=far, src_n=normals[0], tgt_n=normals[1]), np.eye(4), 0.25, 20.0)
        assert status == 1 and (nn == -77).all() and (r == -7.25).all()
    bad_n = n.copy()
    bad_n[3] = 0.0              # the row takes no part: no refusal, and its neighbours answer for it
    status, _, nn, _ = run(lanes, tmp_path, dict(src=src, tgt=far, src_n=n, tgt_n=bad_n), np.eye(4), 0.25, 20.0)
    grid = M.build_grid(far, bad_n, 0.25)
    want = M.correspond(np.eye(4), src, far, n, bad_n, grid, 0.25, 20.0)[0]
    assert status == 0 and np.array_equal(nn[:27], want) and nn[3] == -1
