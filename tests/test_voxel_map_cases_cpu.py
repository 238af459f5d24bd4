"""The inputs of tests/voxel_map_cases.py do what their names say, on tests/voxel_map_model.py alone: a test of the GPU that passes
must have passed for the reason it was written for."""
import numpy as np
import pytest

import voxel_map_cases as K
import voxel_map_model as M


@pytest.mark.parametrize("max_points", [1, 2, 20])
def test_the_admission_boundary_is_decided_by_distance_not_capacity(max_points):
    voxel, res_sq, held, at, nearer = K.admission_boundary(max_points)
    m = M.VoxelHashMap3d(voxel, 100.0, max_points)
    assert m.map_resolution_sq == res_sq
    m.add_points([held])
    assert M.point_to_voxel(at, m.inv) == M.point_to_voxel(nearer, m.inv) == M.point_to_voxel(held, m.inv) == (0, 0, 0)
    assert K.next_down(at[0]) == nearer[0]                       # one representable step apart
    if max_points > 1:
        assert M.dist_sq(held, nearer) < res_sq <= M.dist_sq(held, at)
    if max_points == 1:
        assert m.rejected_by(nearer) == m.rejected_by(at) == "capacity"   # a voxel of one point is full after the first
    else:
        assert m.rejected_by(nearer) == "distance" and m.rejected_by(at) is None


def test_three_times_p_distant_candidates_stop_at_p():
    pts = K.distant_in_one_voxel(60)
    m = M.VoxelHashMap3d(100.0, 1000.0, 20)
    assert all(M.dist_sq(a, b) >= m.map_resolution_sq for i, a in enumerate(pts) for b in pts[:i])
    m.add_points(pts[:20])
    assert m.num_voxels() == 1 and m.num_points() == 20
    assert all(m.rejected_by(p) == "capacity" for p in pts[20:])


def test_one_voxel_offered_many_candidates_rejects_by_distance_first():
    cand = K.one_voxel_candidates(5000, 3)
    m = M.VoxelHashMap3d(1.0, 100.0, 20)
    by_distance = 0
    for k, p in enumerate(cand):
        if m.num_points() == 20:
            break
        by_distance += k > 0 and m.rejected_by(p) == "distance"
        m.add_points([p])
    assert m.num_voxels() == 1 and m.num_points() == 20 and by_distance > 0 and k < 4000   # both rejections happen in the walk


def test_distinct_voxels_are_distinct():
    rows = K.distinct_voxels(1000)
    m = M.VoxelHashMap3d(1.0)
    m.add_points(rows)
    assert m.num_voxels() == 1000 == m.num_points()


def test_wrapping_chain_cells():
    cells = K.cells_starting_at(31, 31, 5)
    assert len(set(cells)) == 5 and all(M.voxel_hash(c) & 31 == 31 for c in cells)


def test_the_removal_boundary_sits_exactly_at_max_voxel_dist():
    voxel, max_distance, rows, origin, cells = K.removal_boundary()
    m = M.VoxelHashMap3d(voxel, max_distance)
    assert m.max_voxel_dist == 4
    m.add_points(rows)
    assert m.cells == cells and m.num_points() == 2 * len(cells)
    o = M.point_to_voxel(origin, m.inv)
    d2 = [sum((c[k] - o[k]) ** 2 for k in range(3)) for c in cells]
    assert d2 == [16, 14, 12, 16, 17, 0]
    assert [m.is_far(c, o) for c in cells] == [True, False, False, True, True, False]


def test_lattice_ties_are_ties():
    pts, queries = K.lattice_ties()
    m = M.VoxelHashMap3d(1.0, 100.0, 1)
    m.add_points(pts)
    assert m.num_points() == 8
    ties = []
    for q in queries:
        d = sorted(M.dist_sq(p, q) for p in pts)
        ties.append(sum(1 for x in d if x == d[0]))
        best = m.get_closest_neighbor(q)
        assert best[1] == d[0]
        # the winner is the first tied point in VOXEL_SHIFTS order
        voxel = M.point_to_voxel(q, m.inv)
        for shift in M.VOXEL_SHIFTS:
            cell = tuple(voxel[k] + shift[k] for k in range(3))
            if cell in m.index and M.dist_sq(m.buckets[m.index[cell]][0], q) == d[0]:
                assert best[0] == m.buckets[m.index[cell]][0]
                break
    assert ties == [8, 4, 2, 4, 2]


def test_face_queries_sit_on_cell_boundaries():
    q = K.face_edge_corner_queries()
    on = [sum(1 for c in row if (c * 2.0) == int(c * 2.0)) for row in q]
    assert {1, 2, 3} <= set(on)


def test_the_moving_script_evicts_and_keeps():
    m = M.VoxelHashMap3d(0.5, 4.0, 3)
    out = K.run_script(m, K.moving_script(5))
    counts = [o for name, o in out if name == "counts"]
    assert counts[0][0] > 0 and counts[-2].tolist() == [0, 0, 1] and counts[-1][0] > 0
    extracts = [o for name, o in out if name == "extract"]
    assert len(extracts) == 1 and len(extracts[0]) > 0           # the far origin evicts something
    clouds = [o for name, o in out if name == "cloud"]
    assert any(len(c) for c in clouds) and any(len(c) == 0 for c in clouds)
    d2 = [o for name, o in out if name == "closest distances"]
    assert any((d == 4.0).any() for d in d2) and any((d < 4.0).any() for d in d2)   # bounded queries with and without a neighbour
