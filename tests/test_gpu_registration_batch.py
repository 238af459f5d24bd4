"""ICPRegistration on resident hip::DeviceFrameBatch es, through tests/cpp/registration_batch_tool.cpp: 5 dual-return frames of the
two small sensors of the normals batch test, dewarped and voxel_downsample d, go into a map with add_voxels_to; a second batch of
the same packets with its poses moved on by centimetres is aligned with align_voxels_to_map, its corrected rows go into the map,
and it is aligned again against the grown map.  Both poses must equal ouster_hip_registration_align on the batches' OWN
download_voxels rows bit for bit.  The refusals: before voxel_downsample (std::runtime_error), a map that lives on no device
(std::invalid_argument), a negative max_distance."""
import numpy as np
import pytest

import batch_cases as B
import cpp_tools
import registration_cases as K
import voxel_map_cases as VK
from batch_cases import H, N, W
from conftest import has_gpu

pytestmark = pytest.mark.gpu

VOXEL, MAP_VOXEL, MAX_DISTANCE, MAX_POINTS = 0.25, 1.0, 300.0, 3        # the scene spans several hundred metres
REG_DISTANCE, KERNEL, ITERATIONS = 1.0, 0.3, 30


@pytest.fixture(scope="module")
def run(oracle, tmp_path_factory):
    assert has_gpu()
    tmp = tmp_path_factory.mktemp("registration_batch")
    B.write_packets(oracle, tmp, B.scene)
    B.write_known(tmp)
    args = [tmp / "packets.bin", H, W, N, tmp / "known.bin", B.K, tmp / "o", VOXEL, MAP_VOXEL, MAX_DISTANCE, MAX_POINTS, REG_DISTANCE, KERNEL,
            ITERATIONS]
    p = cpp_tools.run("registration_batch_tool", args)
    out = {"stdout": p.stdout}
    for name in ("r0.vox", "r1.vox", "corrected"):
        out[name] = np.fromfile(tmp / ("o." + name), np.float64).reshape(-1, 3)
    for name in ("pose1", "pose2"):
        out[name] = np.fromfile(tmp / ("o." + name), np.float64).reshape(4, 4)
    return out


def test_refusals_and_the_device_overload(run):
    for line in ("pre_voxel_throws 1", "host_map_throws 1", "bad_parameter_throws 1", "device_overload 1"):
        assert run["stdout"].count(line) == 1, (line, run["stdout"])


def test_poses_equal_the_c_abi_on_the_batches_own_rows(run):
    import torch
    from ouster_sdk_amd import _capi as capi
    assert N == 5 and len(run["r0.vox"]) > 500 and len(run["r1.vox"]) > 500
    ctx = capi.Context(0)
    try:
        to_device = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
        with VK.CapiMap(capi, ctx.h, MAP_VOXEL, MAX_DISTANCE, MAX_POINTS, to_device=to_device, from_device=lambda t: t.cpu().numpy()) as m:
            m.add_points(run["r0.vox"])
            rows = to_device(run["r1.vox"])
            kw = dict(pointer=rows.data_ptr(), host=False, max_iterations=ITERATIONS, max_distance=REG_DISTANCE, kernel_scale=KERNEL)
            pose1, it1, count1, _ = K.align_capi(capi, m.h, run["r1.vox"], **kw)
            K.same_bytes(run["pose1"], pose1, "pose against the map of batch 0")
            # the case does what it was built for: passes were run on correspondences, and the pose moves the rows
            assert it1 >= 2 and count1 > 100 and not np.array_equal(pose1, np.eye(4))
            T = run["pose1"]
            assert np.allclose(run["corrected"], run["r1.vox"] @ T[:3, :3].T + T[:3, 3], rtol=0, atol=1e-9)
            m.add_points(run["corrected"])
            pose2, it2, count2, _ = K.align_capi(capi, m.h, run["r1.vox"], **kw)
            K.same_bytes(run["pose2"], pose2, "pose against the grown map")
            assert it2 >= 1 and count2 >= count1 and not np.array_equal(pose2, pose1)
    finally:
        ctx.close()
