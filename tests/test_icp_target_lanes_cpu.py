"""CPU-only: k_icp_correspond_many (csrc/k_icp.hip) compiled for the host, one thread per lane (tests/cpp/icp_target_lanes.cpp over
tests/cpp/host_lanes), against tests/icp_model.py bit for bit.  The two groups of tests/test_gpu_icp_target.py, one launch each:
group A is tie_target as float64 with the sources of 20, 65 and 1041 rows from the identity, group B the float32 strided target
with the sources of 257 and 1041 rows from POSE_B.  The neighbour index and the residual of every row of every source must equal
K.tie_model; the chunk table is the library's (csrc/host/icp_util.cpp).  Then each group again with one source marked inactive: its
rows keep their guard values, the others' results do not change.  A launch has one angle gate, and the 20-row tie case is built for
a wide-open one: on the plane route group A runs once per gate, each source compared with the model at the launch's gate.  The sum, median and fold kernels use cross-lane operations or
device-only launches and are covered on the GPU only."""
import struct
import subprocess

import numpy as np
import pytest

import cpp_tools
import icp_cases as K
import icp_model as M
import icp_target_cases as T


@pytest.fixture(scope="module")
def lanes():
    return cpp_tools.build("icp_target_lanes")[0]


def run(exe, tmp_path, group, plane, active, angle):
    """-> (status, chunks, nn with guard, r with guard) of the concatenated sources"""
    tgt, tgt_n = group["tgt"], group["tgt_n"]
    n_tgt = len(tgt)
    table_log2 = max(1, int(2 * n_tgt - 1).bit_length())
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("<8I", len(group["sources"]), n_tgt, tgt.shape[1], tgt_n.shape[1] if plane else 3, int(tgt.dtype == np.float32),
                            int(group["sources"][0]["src"].dtype == np.float32), int(plane), table_log2))
        f.write(struct.pack("<2d", K.CELL, M.cos_gate(angle) if plane else 0.0))
        for a in (tgt,) + ((tgt_n,) if plane else ()):
            f.write(np.ascontiguousarray(a).tobytes())
        for a, pose, on in zip(group["sources"], group["poses"], active):
            src, src_n = a["src"], a["src_n"]
            f.write(struct.pack("<4I", len(src), src.shape[1], src_n.shape[1] if plane else 3, int(on)))
            f.write(struct.pack("<16d", *np.asarray(pose, dtype=np.float64).reshape(-1)))
            for b in (src,) + ((src_n,) if plane else ()):
                f.write(np.ascontiguousarray(b).tobytes())
    subprocess.check_call([exe, case, res], timeout=300)
    raw = open(res, "rb").read()
    total = sum(group["sizes"])
    status, chunks = struct.unpack("<II", raw[:8])
    nn = np.frombuffer(raw[8:8 + 4 * (total + 16)], np.int32)
    r = np.frombuffer(raw[8 + 4 * (total + 16):], np.float64)
    return status, chunks, nn, r


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
@pytest.mark.parametrize("which", [0, 1], ids=["group_a", "group_b"])
def test_many_sources_in_one_launch_equal_the_model_bit_for_bit(lanes, tmp_path, plane, which):
    group = T.step_groups(plane)[which]
    sizes = group["sizes"]
    total = sum(sizes)
    # a launch has one gate: on the plane route the group runs once per gate of its tie cases (icp_target_cases.tie_model_at), so
    # that every source meets K.tie_model itself in a launch with all the others
    for angle in T.step_gates(group, plane):
        for off in (None, len(sizes) - 1, 0):
            active = [k != off for k in range(len(sizes))]
            status, chunks, nn, r = run(lanes, tmp_path, group, plane, active, angle)
            assert status == 0 and chunks == len(T.chunk_table(list(sizes)))
            assert (nn[total:] == K.GUARD_NN).all() and (r[total:] == K.GUARD_R).all()
            at = 0
            for n, on in zip(sizes, active):
                want = T.tie_model_at(n, plane, group["variant"], angle)
                got_nn, got_r = nn[at:at + n], r[at:at + n]
                if on:
                    assert np.array_equal(got_nn, want["nn"]), (n, angle, np.flatnonzero(got_nn != want["nn"])[:10])
                    assert K.same_bits(got_r, want["r"]), (n, angle)
                else:       # an inactive source: its chunks returned at once, the guard values are still there
                    assert (got_nn == K.GUARD_NN).all() and (got_r == K.GUARD_R).all(), (n, angle)
                at += n
