"""The yardstick itself (tests/voxel_model.py), CPU only: the arrays the reference recorded, the properties its own C++ tests
assert, and the rules the model restates -- the floor at negative coordinates, the fold that starts at +0.0, the thresholds, the
special case of RANDOM that the GPU takes, every validation message and the order of the checks."""
import numpy as np
import pytest

import voxel_cases as K
import voxel_model as M


def voxels_of(rows, voxel_size):
    return [M.point_to_voxel(r, 1.0 / voxel_size) for r in np.asarray(rows)]


def test_recorded_arrays_of_the_reference():
    frame, recorded = K.recorded_case()
    for voxel_size, rows in recorded:
        got = M.voxel_downsample_xd(frame, voxel_size, 1, 1, M.AVERAGE_POINT)
        assert np.array_equal(M.sorted_rows(got), M.sorted_rows(rows)), (voxel_size, got)
    # first-seen order: the voxel of row 0 first
    assert M.voxel_downsample_xd(frame, 0.1, 1, 1, M.AVERAGE_POINT)[:, 1].tolist() == [1.0, 2.0]


@pytest.mark.parametrize("strategy", M.STRATEGIES)
def test_one_row_per_voxel_and_selected_rows_are_inputs(strategy):
    cloud = K.uniform_cloud(2000, cols=5, seed=3, extent=5.0)
    out = M.voxel_downsample_xd(cloud, 0.8, 1, 1, strategy)
    keys = voxels_of(out, 0.8)
    assert len(set(keys)) == len(keys) == len(set(voxels_of(cloud, 0.8)))
    if strategy != M.AVERAGE_POINT:
        rows = {r.tobytes() for r in cloud}
        assert all(r.tobytes() in rows for r in out)
    else:   # a mean lies in its voxel's cell (the box of its points)
        assert sorted(keys) == sorted(set(voxels_of(cloud, 0.8)))
    # several points per voxel: never more than asked for, all inputs, all in their voxel, voxels contiguous
    if strategy != M.AVERAGE_POINT:
        out = M.voxel_downsample_xd(cloud, 2.5, 3, 1, strategy)
        keys = voxels_of(out, 2.5)
        runs = [k for i, k in enumerate(keys) if i == 0 or keys[i - 1] != k]
        assert len(runs) == len(set(keys)) and max(keys.count(k) for k in set(keys)) <= 3
        rows = {r.tobytes() for r in cloud}
        assert all(r.tobytes() in rows for r in out)


def test_random_with_one_slot_is_last_point_wins():
    for seed in range(4):
        cloud = K.clustered_cloud(500, clusters=6, cols=4, seed=seed)
        M.same_bits(M.voxel_downsample_xd(cloud, 1.0, 1, 1, M.RANDOM), M.last_point_wins(cloud, 1.0), "seed %d" % seed)
    # with more slots the generator matters: the general form is what the model implements
    rand = M.Xorshift32()
    assert [rand() for _ in range(3)] == [11355432, 2836018348, 476557059]
    cloud = np.array([[0.1, 0.1, 0.1, float(i)] for i in range(6)])
    rand, slots = M.Xorshift32(), [0.0, 1.0]
    for i in range(2, 6):
        slots[(rand() * 2) >> 32] = float(i)
    assert M.voxel_downsample_xd(cloud, 1.0, 2, 1, M.RANDOM)[:, 3].tolist() == slots


def test_first_n_point_admission():
    cloud = np.array([[0.1, 0.1, 0.1], [0.15, 0.1, 0.1], [0.9, 0.9, 0.9], [0.5, 0.5, 0.5], [0.2, 0.8, 0.3], [0.1, 0.9, 0.1]])
    # resolution^2 = 1 / 4: the second point is 0.05 from the first and the fifth 0.22 (squared) from the fourth: refused
    out = M.voxel_downsample_3d(cloud, 1.0, 4, 1, M.FIRST_N_POINT)
    assert out.tolist() == [cloud[0].tolist(), cloud[2].tolist(), cloud[3].tolist(), cloud[5].tolist()]
    assert M.voxel_downsample_3d(cloud, 1.0, 2, 1, M.FIRST_N_POINT).tolist() == [cloud[0].tolist(), cloud[2].tolist()]   # full at two
    assert M.voxel_downsample_3d(cloud, 1.0, 1, 7, M.FIRST_N_POINT).tolist() == [cloud[0].tolist()]    # the threshold is not looked at


def test_negative_coordinates_floor_and_zero_signs():
    cloud = np.array([[-0.25, -1e-300, -0.0], [0.25, 1e-300, 0.0]])
    assert voxels_of(cloud, 0.5) == [(-1, -1, 0), (0, 0, 0)]
    assert voxels_of([[-0.5, -1.0, 0.5]], 0.5) == [(-1, -2, 1)]      # exactly on a face: the voxel above it
    lone = np.array([[-0.0, -0.0, -0.0, -0.0]])
    assert not np.signbit(M.voxel_downsample_xd(lone, 1.0, 1, 1, M.AVERAGE_POINT)).any()     # +0.0 + -0.0
    assert np.signbit(M.voxel_downsample_xd(lone, 1.0, 1, 1, M.RANDOM)).all()
    assert np.signbit(M.voxel_downsample_xd(lone, 1.0, 1, 1, M.FIRST_N_POINT)).all()


def test_average_is_a_left_fold_in_input_order():
    col = np.array([1e16, 1.0, -1e16, 1.0])
    cloud = np.zeros((4, 4))
    cloud[:, :3], cloud[:, 3] = 0.5, col
    assert M.voxel_downsample_xd(cloud, 1.0, 1, 1, M.AVERAGE_POINT)[0, 3] == (((0.0 + 1e16) + 1.0) - 1e16 + 1.0) / 4.0 == 0.25
    assert M.voxel_downsample_xd(cloud[::-1], 1.0, 1, 1, M.AVERAGE_POINT)[0, 3] == 0.0


def test_threshold_rules():
    cloud = np.array([[0.5, 0.5, 0.5]] * 3 + [[1.5, 0.5, 0.5]] * 2 + [[2.5, 0.5, 0.5]])
    for min_pts, kept in ((0, 3), (1, 3), (2, 2), (3, 1), (4, 0)):
        assert len(M.voxel_downsample_3d(cloud, 1.0, 1, min_pts, M.AVERAGE_POINT)) == kept
        assert len(M.voxel_downsample_3d(cloud, 1.0, 1, min_pts, M.RANDOM)) == 3
    assert M.voxel_downsample_3d(cloud, 1.0, 1, 4, M.AVERAGE_POINT).shape == (0, 3)


def test_with_normals_rules():
    pts, nrm = K.normals_cloud()
    out_p, out_n = M.voxel_downsample_with_normals(pts, nrm, 1.0)
    assert len(out_p) == len(out_n) > 0 and np.isfinite(out_p).all() and np.isfinite(out_n).all()
    assert np.abs(np.sqrt((out_n * out_n).sum(1)) - 1.0).max() < 1e-12
    keys = voxels_of(out_p, 1.0)
    assert (10, 10, 10) not in keys and (20, 10, 10) in keys      # n and -n: dropped; nearly cancelling: kept
    # scaling a normal changes nothing but rounding; a zero normal takes its point out
    a = M.voxel_downsample_with_normals([[0.1, 0.1, 0.1], [0.9, 0.9, 0.9]], [[0.0, 0.0, 4.0], [0.0, 0.0, 0.0]], 1.0)
    assert a[0].tolist() == [[0.1, 0.1, 0.1]] and a[1].tolist() == [[0.0, 0.0, 1.0]]
    empty = M.voxel_downsample_with_normals(np.zeros((0, 3)), np.zeros((0, 3)), 1.0)
    assert empty[0].shape == empty[1].shape == (0, 3)


def test_validation_messages_and_their_order():
    good = np.zeros((2, 3))
    for fn, msg, bad in ((M.voxel_downsample_3d, M.MSG_3D, np.zeros((2, 4))), (M.voxel_downsample_3d, M.MSG_3D, np.zeros(3)),
                         (M.voxel_downsample_xd, M.MSG_XD, np.zeros((2, 2))), (M.voxel_downsample_xd, M.MSG_XD, np.zeros((0, 2)))):
        with pytest.raises(ValueError) as e:
            fn(bad, 1.0)
        assert str(e.value) == msg
    for fn in (M.voxel_downsample_3d, M.voxel_downsample_xd):
        assert fn(np.zeros((0, 3)), -1.0, 0).shape == (0, 3)                 # empty: before any other check
        with pytest.raises(ValueError, match=M.MSG_MAX_POINTS):
            fn(good, -1.0, 0)                                                # max_points before voxel_size
        for size in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=M.MSG_VOXEL_SIZE):
                fn(good, size)
        for bad in (float("nan"), float("inf"), 1e13):
            c = good.copy()
            c[1, 2] = bad
            with pytest.raises(ValueError, match=M.MSG_GRID):
                fn(c, 0.5, 1, 1, M.AVERAGE_POINT)
    assert M.voxel_downsample_xd(np.array([[0.0, 0.0, 0.0, float("nan")]]), 1.0).shape == (1, 4)   # attributes are not looked at
    assert M.voxel_downsample_3d(np.array([[-2.0 ** 30, 0.0, 2.0 ** 30 - 0.5]]), 0.5).shape == (1, 3)      # the grid's two ends
    with pytest.raises(ValueError, match=M.MSG_GRID):
        M.voxel_downsample_3d(np.array([[2.0 ** 30, 0.0, 0.0]]), 0.5)
    wn = M.voxel_downsample_with_normals
    for args, msg in (((np.zeros((2, 4)), np.zeros((2, 3)), 1.0), M.MSG_WN_SHAPE), ((good, np.zeros((2, 2)), 1.0), M.MSG_WN_SHAPE),
                      ((good, np.zeros((3, 3)), 1.0), M.MSG_WN_ROWS), ((good, good, 0.0), M.MSG_WN_SIZE),
                      ((good, good, float("nan")), M.MSG_WN_SIZE), ((np.zeros((2, 4)), np.zeros((3, 3)), 0.0), M.MSG_WN_SHAPE),
                      ((good, np.zeros((3, 3)), 0.0), M.MSG_WN_ROWS)):
        with pytest.raises(ValueError) as e:
            wn(*args)
        assert str(e.value) == msg
    far = np.array([[1e13, 0.0, 0.0]])
    assert wn(far, np.zeros((1, 3)), 0.5)[0].shape == (0, 3)                 # a skipped row is not held to the grid
    with pytest.raises(ValueError, match=M.MSG_GRID):
        wn(far, np.array([[0.0, 0.0, 1.0]]), 0.5)
