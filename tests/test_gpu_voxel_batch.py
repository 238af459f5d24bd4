"""Voxel down-sampling on a resident hip::DeviceFrameBatch, through tests/cpp/voxel_batch_tool.cpp: 5 dual-return frames of the two
small sensors of the normals batch test, one packet of one frame left out, an f64 and a float batch with interpolated poses.
dewarp() then voxel_downsample at two voxel sizes must equal tests/voxel_model.py run on the batch's OWN download_dewarped points;
normals(staggered_output) then voxel_downsample_with_normals must equal the model on the batch's own downloaded cloud and normals
-- bit for bit, row order included -- and both again after filter_field on RANGE and a fresh dewarp().  The three precondition
errors (no dewarp() yet, no normals, normals in the destaggered layout) are std::invalid_argument, and a call that throws leaves no
result behind."""
import os
import subprocess

import numpy as np
import pytest

import voxel_cases as K
import voxel_model as M
from conftest import ROOT, has_gpu
from test_gpu_normals_batch import COL_NS, FRAME_NS, H, N, SKIP_FRAME, SKIP_PACKET, T0_NS, W, scene
from test_gpu_pose_batch import trajectory

pytestmark = pytest.mark.gpu

KNOWN = 9
FILTER_LO, FILTER_HI = 3000.0, 3600.0   # mm: filter_field invalidates the ranges INSIDE
VS_A, VS_B = 0.25, 1.0
TAGS = (("b64", np.float64), ("b32", np.float32))


def build_tool():
    rocm = os.environ.get("ROCM", "/opt/rocm")
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe, lib = os.path.join(out, "voxel_batch_tool"), os.path.join(ROOT, "ouster_sdk_amd", "lib")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "voxel_batch_tool.cpp"), "-L" + lib, "-louster_core_amd",
                           "-louster_hip", "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + lib,
                           "-Wl,-rpath," + os.path.join(rocm, "lib")])
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = lib + ":" + os.path.join(rocm, "lib") + ":" + env.get("LD_LIBRARY_PATH", "")
    return exe, env


@pytest.fixture(scope="module")
def run(oracle, tmp_path_factory):
    assert has_gpu()
    O = oracle
    tmp = tmp_path_factory.mktemp("voxel_batch")
    cal = O.synthetic_calib(h=H, w=W, profile="RNG15_RFL8_NIR8_DUAL")
    pf = cal.packet_format()
    packets = []
    for f in range(N):
        fr = O.Frame.for_profile(cal.profile, cal.h, cal.w, cal.cpp, with_window=cal.with_window)
        O.randomize_frame(fr, pf, 4000 + f, 0.1, frame_id=700 + f)
        r1, r2 = scene(f, fr.plane("RANGE") != 0)   # a tenth of the pixels stays without range
        fr.plane("RANGE")[:] = r1
        fr.plane("RANGE2")[:] = r2
        fr.timestamp[:] = T0_NS + f * FRAME_NS + np.arange(W, dtype=np.uint64) * np.uint64(COL_NS)
        pk, _ = O.frame_to_packets(fr, pf, cal.init_id & 0xFFFFFF, cal.prod_sn)
        packets.append(pk)
    np.ascontiguousarray(np.stack(packets)).tofile(tmp / "packets.bin")
    xk, poses = trajectory()
    with open(tmp / "known.bin", "wb") as fh:
        fh.write(xk.tobytes())
        fh.write(poses.tobytes())
    exe, env = build_tool()
    res = subprocess.run([exe, str(tmp / "packets.bin"), str(H), str(W), str(N), str(SKIP_FRAME), str(SKIP_PACKET), str(tmp / "known.bin"),
                          str(KNOWN), str(tmp / "o"), str(FILTER_LO), str(FILTER_HI), str(VS_A), str(VS_B)],
                         capture_output=True, text=True, env=env, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    out = {"stdout": res.stdout}
    for tag, ft in TAGS:
        b = {}
        for pre in ("", "f"):
            b[pre + "dw"] = np.fromfile(tmp / ("o.%s.%sdw" % (tag, pre)), ft).reshape(-1, 3)
            b[pre + "xyz0"] = np.fromfile(tmp / ("o.%s.%sxyz0" % (tag, pre)), ft).reshape(-1, 3)
            b[pre + "nrm0"] = np.fromfile(tmp / ("o.%s.%snrm0" % (tag, pre)), np.float64).reshape(-1, 3)
            for name in ("va", "wnp", "wnn") + (("vb", "vlast") if pre == "" else ()):
                b[pre + name] = np.fromfile(tmp / ("o.%s.%s%s" % (tag, pre, name)), np.float64).reshape(-1, 3)
        out[tag] = b
    return out


def test_preconditions_and_device_pointers(run):
    for line in ("pre_dewarp_throws 1", "pre_normals_throws 1", "destaggered_throws 1", "host_only_throws 1", "grid_throws 1",
                 "no_result_after_throw 1", "device_ptr b64 1",
                 "device_ptr b32 1"):
        assert run["stdout"].count(line) == (1 if line.startswith("device_ptr") else 2), (line, run["stdout"])


def test_the_clouds_are_what_the_test_needs(run):
    for tag, _ in TAGS:
        b = run[tag]
        pixels = N * H * W
        assert 0.7 * pixels < len(b["dw"]) < 0.97 * pixels and len(b["xyz0"]) == len(b["nrm0"]) == pixels
        assert 0.3 * len(b["dw"]) < len(b["fdw"]) < 0.95 * len(b["dw"])                 # filter_field took points out
        # several points per voxel at the larger size, and voxels that the threshold of 2 drops
        assert len(b["vb"]) <= len(b["vlast"]) < len(b["va"]) <= len(b["dw"])
        has = np.abs(b["nrm0"]).sum(axis=1) > 0
        assert 0.5 < has.mean() < 0.97 and np.isfinite(b["nrm0"]).all()
    assert not np.array_equal(run["b32"]["dw"].astype(np.float64), run["b64"]["dw"][:len(run["b32"]["dw"])])


@pytest.mark.parametrize("tag", ["b64", "b32"])
@pytest.mark.parametrize("pre", ["", "f"])
def test_voxels_of_the_dewarped_cloud_equal_the_model(run, tag, pre):
    b = run[tag]
    cloud = b[pre + "dw"].astype(np.float64)       # a float batch's points are widened: exact
    M.same_bits(b[pre + "va"], K.want(cloud, VS_A, strategy=M.AVERAGE_POINT), "%s %sva" % (tag, pre))
    if pre == "":
        M.same_bits(b["vb"], K.want(cloud, VS_B, 1, 2, M.AVERAGE_POINT), tag + " vb")
        M.same_bits(b["vlast"], K.want(cloud, VS_B, strategy=M.RANDOM), tag + " vlast")


@pytest.mark.parametrize("tag", ["b64", "b32"])
@pytest.mark.parametrize("pre", ["", "f"])
def test_voxels_with_normals_equal_the_model(run, tag, pre):
    b = run[tag]
    want_p, want_n = M.voxel_downsample_with_normals(b[pre + "xyz0"].astype(np.float64), b[pre + "nrm0"], VS_B)
    assert 10 < len(want_p) < len(b[pre + "xyz0"]) // 4
    M.same_bits(b[pre + "wnp"], want_p, "%s %swnp" % (tag, pre))
    M.same_bits(b[pre + "wnn"], want_n, "%s %swnn" % (tag, pre))
    if pre == "f":
        assert len(b["fwnp"]) != len(b["wnp"]) or not np.array_equal(b["fwnp"], b["wnp"])
