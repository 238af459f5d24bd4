"""CPU-only: the source of the normals kernels (csrc/k_normals.hip) compiled for the host, one thread per lane
(tests/cpp/normals_lanes.cpp over tests/cpp/host_lanes/hip/hip_runtime.h), against tests/normals_model.py bit for bit.  It checks
what can go wrong without a GPU in sight -- index arithmetic across frames, returns, tiles and staggered rows, the order of every
floating-point operation, the hand-over of the per-frame constants -- on the small scenes of tests/test_gpu_normals.py; the
device's own arithmetic and the C ABI around the kernels are that test's business."""
import struct
import subprocess

import numpy as np
import pytest

import cpp_tools
import normals_model as M
import test_gpu_normals as G


@pytest.fixture(scope="module")
def lanes():
    return cpp_tools.build("normals_lanes")[0]


def run(exe, tmp_path, xyz, r1, xyz2, r2, psr, f32=False, shifts=None, staggered_out=False, origins=None, poses=None, s2b=None):
    """arrays with a leading frame axis -> per return (n, h * w, 3)"""
    n, h, w = r1.shape
    ft = np.float32 if f32 else np.float64
    mode = 1 if origins is not None else 2 if poses is not None else 0
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("<9I", n, h, w, 1, int(f32), psr, int(shifts is not None), mode, int(staggered_out)))
        for a, t in ((xyz, ft), (r1, np.uint32), (xyz2, ft), (r2, np.uint32)):
            f.write(np.ascontiguousarray(a, t).tobytes())
        if shifts is not None:
            f.write((np.asarray(shifts, np.int64) % w).astype(np.uint32).tobytes())
        if mode == 1:
            f.write(np.ascontiguousarray(origins, np.float64).tobytes())
        if mode == 2:
            f.write(np.ascontiguousarray(poses, np.float64).tobytes() + np.ascontiguousarray(s2b, np.float64).tobytes())
    subprocess.check_call([exe, case, res], timeout=300)
    return np.fromfile(res, np.float64).reshape(2, n, h * w, 3)


def test_several_frames(lanes, tmp_path):
    h, w, psr, n, xyz, r1, xyz2, r2, poses, s2b = G.several_frames()
    got = run(lanes, tmp_path, xyz, r1, xyz2, r2, psr, poses=poses, s2b=s2b)
    for f in range(n):
        want = M.normals(xyz[f], r1[f], xyz2[f], r2[f], sensor_origins_xyz=M.sensor_origins(poses[f], s2b), pixel_search_range=psr)
        G.same_bits(got[0][f], want[0], "frame %d first" % f)
        G.same_bits(got[1][f], want[1], "frame %d second" % f)


@pytest.mark.parametrize("h,w,psr", [(1, 8, 1), (5, 7, 9), (7, 5, 9), (G.TILE_H + 1, G.TILE_W + 1, 3)])
def test_staggered_float_and_explicit_origins(lanes, tmp_path, h, w, psr):
    xyz, r1, xyz2, r2 = G.scene(h, w)
    shifts = np.random.default_rng(h * w).integers(-2 * w - 3, 2 * w + 3, h).astype(np.int32)
    sx, sr = G.stagger(xyz.reshape(h, w, 3), shifts)[None], G.stagger(r1, shifts)[None]
    sx2, sr2 = G.stagger(xyz2.reshape(h, w, 3), shifts)[None], G.stagger(r2, shifts)[None]
    want = G.model(h, w, True, False, psr, "null")
    got = run(lanes, tmp_path, sx, sr, sx2, sr2, psr, shifts=shifts)
    out = run(lanes, tmp_path, sx, sr, sx2, sr2, psr, shifts=shifts, staggered_out=True)
    for i in range(2):
        G.same_bits(got[i][0], want[i], "staggered in, return %d" % i)
        G.same_bits(out[i][0], G.stagger(want[i].reshape(h, w, 3), shifts), "staggered out, return %d" % i)
    want = G.model(h, w, True, True, psr, "explicit")
    got = run(lanes, tmp_path, xyz[None], r1[None], xyz2[None], r2[None], psr, f32=True, origins=G.origins_for(w, "explicit")[1])
    for i in range(2):
        G.same_bits(got[i][0], want[i], "f32, explicit origins, return %d" % i)
