"""Voxel down-sampling on a resident hip::DeviceFrameBatch, through tests/cpp/voxel_batch_tool.cpp: 5 dual-return frames of the two
small sensors of the normals batch test, one packet of one frame left out, an f64 and a float batch with interpolated poses.
dewarp() then voxel_downsample at two voxel sizes must equal tests/voxel_model.py run on the batch's OWN download_dewarped points;
normals(staggered_output) then voxel_downsample_with_normals must equal the model on the batch's own downloaded cloud and normals
-- bit for bit, row order included -- and both again after filter_field on RANGE and a fresh dewarp().  The three precondition
errors (no dewarp() yet, no normals, normals in the destaggered layout) are std::invalid_argument, and a call that throws leaves no
result behind."""
import numpy as np
import pytest

import batch_cases as B
import cpp_tools
import voxel_cases as K
import voxel_model as M
from batch_cases import FILTER_HI, FILTER_LO, H, N, SKIP_FRAME, SKIP_PACKET, W
from conftest import has_gpu

pytestmark = pytest.mark.gpu

VS_A, VS_B = 0.25, 1.0
TAGS = (("b64", np.float64), ("b32", np.float32))


@pytest.fixture(scope="module")
def run(oracle, tmp_path_factory):
    assert has_gpu()
    tmp = tmp_path_factory.mktemp("voxel_batch")
    B.write_packets(oracle, tmp, B.scene)
    B.write_known(tmp)
    res = cpp_tools.run("voxel_batch_tool", [tmp / "packets.bin", H, W, N, SKIP_FRAME, SKIP_PACKET, tmp / "known.bin", B.K, tmp / "o",
                                             FILTER_LO, FILTER_HI, VS_A, VS_B])
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
