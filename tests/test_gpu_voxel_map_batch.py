"""The resident voxel map fed from resident hip::DeviceFrameBatch es, through tests/cpp/voxel_map_batch_tool.cpp: three successive
batches of 5 dual-return frames of the two small sensors of the normals batch test, each with its poses moved on, dewarped,
voxel_downsample d and sent into one map with update_voxel_map at a moving position (each batch's first voxel row); then closest_in on the last batch.  The map's
cloud after every update and the neighbours must equal tests/voxel_map_model.py run on the batches' OWN download_voxels rows -- bit
for bit, row order included.  The throwing preconditions: before voxel_downsample (std::runtime_error), a map that lives in host
memory (std::invalid_argument), a position outside the grid."""
import numpy as np
import pytest

import batch_cases as B
import cpp_tools
import voxel_map_cases as K
import voxel_map_model as M
from batch_cases import H, N, W
from conftest import has_gpu

pytestmark = pytest.mark.gpu

VOXEL, MAP_VOXEL, MAX_DISTANCE, MAX_POINTS, BOUND_SQ = 0.25, 1.0, 300.0, 3, 0.01   # the scene spans several hundred metres
STEP = np.array([1.5, -0.75, 0.25])


@pytest.fixture(scope="module")
def run(oracle, tmp_path_factory):
    assert has_gpu()
    tmp = tmp_path_factory.mktemp("voxel_map_batch")
    B.write_packets(oracle, tmp, B.scene)
    B.write_known(tmp)
    args = [tmp / "packets.bin", H, W, N, tmp / "known.bin", B.K, tmp / "o", VOXEL, MAP_VOXEL, MAX_DISTANCE, MAX_POINTS, BOUND_SQ]
    p = cpp_tools.run("voxel_map_batch_tool", args)
    out = {"stdout": p.stdout}
    for r in range(3):
        for name in ("vox", "cloud", "pos"):
            out["r%d.%s" % (r, name)] = np.fromfile(tmp / ("o.r%d.%s" % (r, name)), np.float64).reshape(-1, 3)
    out["nn"] = np.fromfile(tmp / "o.nn", np.float64).reshape(-1, 3)
    out["d2"] = np.fromfile(tmp / "o.d2", np.float64)
    out["add.cloud"] = np.fromfile(tmp / "o.add.cloud", np.float64).reshape(-1, 3)
    return out


def test_preconditions_and_device_pointers(run):
    for line in ("pre_voxel_throws 1", "host_map_throws 1", "grid_throws 1", "device_ptr 1", "pre_closest 1"):
        assert run["stdout"].count(line) == 1, (line, run["stdout"])


def test_the_map_follows_the_batches(run):
    model = M.VoxelHashMap3d(MAP_VOXEL, MAX_DISTANCE, MAX_POINTS)
    sizes = []
    for r in range(3):
        rows = run["r%d.vox" % r]
        assert len(rows) > 500
        before = model.num_voxels()
        model.update(rows, tuple(run["r%d.pos" % r][0]))
        K.same_bytes(run["r%d.cloud" % r], model.pointcloud(), "cloud after update %d" % r)
        sizes.append((before, model.num_voxels(), model.num_points()))
    # the case does what it was built for: later batches meet held points, and the moving position evicts
    assert np.allclose(run["r2.vox"][-1] - run["r0.vox"][-1], 2 * STEP, atol=1e-6)      # the batches move on
    assert sizes[0][1] > 0 and sizes[1][0] > 0 and 0 < sizes[2][2] < sum(len(run["r%d.vox" % r]) for r in range(3))
    far = M.VoxelHashMap3d(MAP_VOXEL, 1e6, MAX_POINTS)
    for r in range(3):
        far.add_points(run["r%d.vox" % r])
    assert far.num_voxels() > model.num_voxels()                       # something was evicted on the way
    want = model.get_closest_neighbors(run["r2.vox"], BOUND_SQ)
    K.same_bytes(run["nn"], want[0], "neighbours")
    K.same_bytes(run["d2"], want[1], "distances")
    hit = run["d2"] < BOUND_SQ
    assert hit.any() and not hit.all() and (run["nn"][~hit] == 0.0).all()


def test_add_voxels_to(run):
    model = M.VoxelHashMap3d(MAP_VOXEL, MAX_DISTANCE, MAX_POINTS)
    model.add_points(run["r0.vox"])
    model.add_points(run["r2.vox"])
    K.same_bytes(run["add.cloud"], model.pointcloud(), "add_voxels_to")
