"""tests/voxel_map_model.py pinned by hand on the situations of the reference's tests/voxel_hashmap_test.cpp, against a brute-force
search within that test's 1e-12, and on the constructor's refusals."""
import math

import numpy as np
import pytest

import voxel_map_model as M


def brute_force(points, query):
    best, best_sq = (0.0, 0.0, 0.0), M.DBL_MAX
    for p in points:
        d = sum((float(p[k]) - float(query[k])) ** 2 for k in range(3))
        if d < best_sq:
            best, best_sq = tuple(p), d
    return best, best_sq


def test_empty_map_returns_max():
    m = M.VoxelHashMap3d(1.0)
    assert m.empty()
    assert m.get_closest_neighbor((0.5, 0.5, 0.5)) == ((0.0, 0.0, 0.0), M.DBL_MAX)
    assert m.get_closest_neighbor((0.5, 0.5, 0.5), 2.5) == ((0.0, 0.0, 0.0), 2.5)
    assert m.pointcloud().shape == (0, 3)


def test_exact_match():
    m = M.VoxelHashMap3d(1.0)
    m.add_points([(2.5, 3.5, 4.5)])
    assert not m.empty()
    assert m.get_closest_neighbor((2.5, 3.5, 4.5)) == ((2.5, 3.5, 4.5), 0.0)


def test_same_voxel_neighbor():
    m = M.VoxelHashMap3d(1.0)
    m.add_points([(0.3, 0.3, 0.3)])
    p, d = m.get_closest_neighbor((0.7, 0.7, 0.7))
    dx = 0.3 - 0.7
    assert p == (0.3, 0.3, 0.3) and d == (dx * dx + dx * dx) + dx * dx


def test_adjacent_voxel_across_a_face():
    m = M.VoxelHashMap3d(1.0)
    m.add_points([(0.2, 0.5, 0.5), (1.1, 0.5, 0.5)])
    assert m.cells == [(0, 0, 0), (1, 0, 0)]
    p, d = m.get_closest_neighbor((0.95, 0.5, 0.5))
    assert p == (1.1, 0.5, 0.5) and d == (1.1 - 0.95) * (1.1 - 0.95)


def test_a_bound_that_prunes_all_and_one_that_allows():
    m = M.VoxelHashMap3d(1.0)
    m.add_points([(5.0, 5.0, 5.0)])
    assert m.get_closest_neighbor((5.5, 5.5, 5.5), 0.001) == ((0.0, 0.0, 0.0), 0.001)
    p, d = m.get_closest_neighbor((5.1, 5.0, 5.0), 1.0)
    assert p == (5.0, 5.0, 5.0) and d == (5.0 - 5.1) * (5.0 - 5.1)
    # d^2 == max_distance_sq is no match: the best is replaced on strict <
    assert m.get_closest_neighbor((5.5, 5.0, 5.0), 0.25) == ((0.0, 0.0, 0.0), 0.25)
    assert m.get_closest_neighbor((5.5, 5.0, 5.0), 0.2500000001)[0] == (5.0, 5.0, 5.0)


def test_negative_coordinates():
    m = M.VoxelHashMap3d(1.0)
    m.add_points([(-2.3, -1.7, -0.5)])
    assert m.cells == [(-3, -2, -1)]
    p, d = m.get_closest_neighbor((-2.1, -1.9, -0.6))
    dx, dy, dz = -2.3 - -2.1, -1.7 - -1.9, -0.5 - -0.6
    assert p == (-2.3, -1.7, -0.5) and d == (dx * dx + dy * dy) + dz * dz


@pytest.mark.parametrize("seed, bound", [(42, None), (123, 2.0)])
def test_matches_brute_force(seed, bound):
    rng = np.random.default_rng(seed)
    m = M.VoxelHashMap3d(1.0, 100.0, 20)
    m.add_points(rng.uniform(-5.0, 5.0, (2000, 3)))
    held = m.pointcloud()
    assert 0 < len(held) <= 2000
    hits = 0
    for q in rng.uniform(-5.0, 5.0, (500, 3)):
        want = brute_force(held, q)[1]
        if bound is None:
            got = m.get_closest_neighbor(q)[1]
            assert abs(got - want) <= 1e-12
        else:
            got = m.get_closest_neighbor(q, bound * bound)[1]
            if want < bound * bound:
                assert abs(got - want) <= 1e-12
                hits += 1
            else:
                assert got >= bound * bound
    assert bound is None or hits > 0


def test_the_constructors_refusals_in_the_references_order():
    with pytest.raises(ValueError, match="^" + M.MSG_MAX_POINTS + "$"):
        M.VoxelHashMap3d(0.0, -1.0, 0, 1, 5)
    with pytest.raises(ValueError, match="^" + M.MSG_VOXEL_SIZE + "$"):
        M.VoxelHashMap3d(0.0, -1.0, 20, 1, 5)
    with pytest.raises(ValueError, match="^" + M.MSG_MAX_DISTANCE + "$"):
        M.VoxelHashMap3d(1.0, 0.0, 20, 1, 5)
    with pytest.raises(ValueError, match="^" + M.MSG_ATTRIBUTES + "$"):
        M.VoxelHashMap3d(1.0, 100.0, 20, 1, 5)
    for bad in (float("nan"), float("inf"), -float("inf")):   # ours: undefined in the reference
        with pytest.raises(ValueError, match=M.MSG_VOXEL_SIZE):
            M.VoxelHashMap3d(bad)
        with pytest.raises(ValueError, match=M.MSG_MAX_DISTANCE):
            M.VoxelHashMap3d(1.0, bad)
    with pytest.raises(ValueError, match="^" + M.MSG_RANGE + "$"):
        M.VoxelHashMap3d(1.0, float(2 ** 31 - 1))          # ceil + 1 == 2^31
    assert M.VoxelHashMap3d(1.0, float(2 ** 31 - 2)).max_voxel_dist == 2 ** 31 - 1
    m = M.VoxelHashMap3d(0.5, 10.0, 5, min_pts_threshold=99)     # accepted, no effect
    assert m.map_resolution_sq == 0.5 * 0.5 / 5.0 and m.inv == 2.0 and m.max_voxel_dist == 21
    m.add_points([(0.1, 0.1, 0.1)])
    assert m.num_points() == 1


def test_admission_is_first_n_point():
    m = M.VoxelHashMap3d(1.0, 100.0, 2)      # resolution_sq 0.5
    m.add_points([(0.1, 0.1, 0.1), (0.2, 0.1, 0.1), (0.9, 0.1, 0.1), (0.9, 0.9, 0.9), (1.5, 0.5, 0.5)])
    assert m.buckets == [[(0.1, 0.1, 0.1), (0.9, 0.1, 0.1)], [(1.5, 0.5, 0.5)]]
    m.add_points([(1.6, 0.5, 0.5), (0.5, 0.5, 0.5)])   # held points gate later calls; a full voxel takes nothing
    assert m.num_points() == 3
    before = m.pointcloud().tobytes()
    with pytest.raises(ValueError, match=M.MSG_GRID):     # refused as a whole
        m.add_points([(5.5, 5.5, 5.5), (float("nan"), 0.0, 0.0)])
    with pytest.raises(ValueError, match=M.MSG_GRID):
        m.add_points([(1e300, 0.0, 0.0)])
    assert m.pointcloud().tobytes() == before and m.num_voxels() == 2
    m.add_points(np.zeros((0, 3)))
    assert m.pointcloud().tobytes() == before


def test_removal_and_order():
    m = M.VoxelHashMap3d(1.0, 3.0)
    assert m.max_voxel_dist == 4
    m.add_points([(4.5, 0.5, 0.5), (3.5, 2.5, 1.5), (0.5, 0.5, 0.5), (-3.5, -2.5, -2.5), (3.9, 2.9, 1.9), (3.6, 2.6, 1.6)])
    got = m.extract_voxels_far_from_location((0.5, 0.5, 0.5))
    assert got.tolist() == [[4.5, 0.5, 0.5], [-3.5, -2.5, -2.5]]
    assert m.pointcloud().tolist() == [[3.5, 2.5, 1.5], [3.9, 2.9, 1.9], [0.5, 0.5, 0.5]]   # (3.6, 2.6, 1.6) was too close
    assert m.get_closest_neighbor((3.4, 2.4, 1.4))[0] == (3.5, 2.5, 1.5)
    with pytest.raises(ValueError, match=M.MSG_GRID):
        m.remove_voxels_far_from_location((float("inf"), 0.0, 0.0))
    with pytest.raises(ValueError, match=M.MSG_GRID):
        m.update([(0.0, 0.0, 0.0)], (math.nan, 0.0, 0.0))
    assert m.num_points() == 3
    m.update([(9.5, 0.5, 0.5)], (9.5, 0.5, 0.5))
    assert m.pointcloud().tolist() == [[9.5, 0.5, 0.5]]
    m.clear()
    assert m.empty() and m.num_points() == 0


def test_queries_outside_the_grid_and_at_its_edge():
    m = M.VoxelHashMap3d(1.0)
    top = float(2 ** 31 - 1)
    m.add_points([(top + 0.5, 0.5, 0.5), (top - 0.5, 0.5, 0.5)])
    assert m.cells == [(2 ** 31 - 1, 0, 0), (2 ** 31 - 2, 0, 0)]
    assert m.get_closest_neighbor((top + 0.25, 0.5, 0.5))[0] == (top + 0.5, 0.5, 0.5)      # the +1 shifts are skipped
    assert m.get_closest_neighbor((float("nan"), 0.5, 0.5), 7.0) == ((0.0, 0.0, 0.0), 7.0)
    assert m.get_closest_neighbor((top + 1.5, 0.5, 0.5)) == ((0.0, 0.0, 0.0), M.DBL_MAX)   # cell 2^31: outside


def test_hash_is_the_devices():
    assert M.voxel_hash((0, 0, 0)) == 0
    assert 0 <= M.voxel_hash((-1, 2, -3)) < 2 ** 32 and M.voxel_hash((-1, 2, -3)) != M.voxel_hash((1, 2, -3))
