"""What the registration tests rely on (tests/registration_cases.py), asserted on the model alone.  CPU only."""
import math

import numpy as np
import pytest

import registration_cases as K
import registration_model as R
import voxel_map_model as M


@pytest.mark.parametrize("max_points", [1, 3, 20])
def test_step_map_is_a_few_hundred_voxels_and_holds_the_special_groups(max_points):
    m = K.step_model(max_points)
    assert 200 <= m.num_voxels() <= 600
    cloud = {tuple(p) for p in m.pointcloud()}
    for p in (K.AT_BOUND_POINT,) + K.TWO_POINTS + K.FOUR_POINTS:      # each alone in its voxel: held whatever P is
        assert p in cloud


@pytest.mark.parametrize("max_points", [1, 3, 20])
def test_special_rows_are_what_their_names_say(max_points):
    m = K.step_model(max_points)
    rows = dict(K.SPECIAL_ROWS)
    bound = K.STEP_MAX_DISTANCE * K.STEP_MAX_DISTANCE
    assert M.dist_sq(K.AT_BOUND_POINT, rows["at_bound"]) == bound      # exactly at the bound
    got = dict(zip(rows, R.associate(list(rows.values()), m, K.STEP_MAX_DISTANCE)))
    assert [got[k][0] for k in rows] == [False, True, True, True, False, False]
    assert got["at_bound"][2] == bound and got["nan"][1] == (0.0, 0.0, 0.0) and got["off_grid"][2] == bound
    # ties: every candidate is equally far, and the first in VOXEL_SHIFTS order keeps it
    assert {M.dist_sq(p, rows["tie_two"]) for p in K.TWO_POINTS} == {0.0625}
    assert {M.dist_sq(p, rows["tie_four"]) for p in K.FOUR_POINTS} == {0.125}
    assert got["tie_two"][1] == K.TWO_POINTS[1]       # the row's own voxel (shift (0, 0, 0)) holds the second point
    assert got["tie_four"][1] == K.FOUR_POINTS[3]


@pytest.mark.parametrize("n", K.ROW_COUNTS)
def test_step_rows_mix_rows_with_and_without_a_correspondence(n):
    rows = K.step_rows(n)
    assert rows.shape == (n, 3)
    if n < 16:
        return
    _, p = K.model_step(rows, K.F64, None, 3)
    assert 0.3 * n < p["count"] < 0.95 * n
    assert [p["flags"][K.special_index(n, k)] for k, _ in K.SPECIAL_ROWS] == [False, True, True, True, False, False]
    assert all(t == R.ZERO_TERMS for t, f in zip(p["terms"], p["flags"]) if not f)
    assert all(math.isfinite(s) for s in p["sums"])                    # the NaN row adds +0.0, not NaN
    # with and without an estimate, as f32 and f64, none but the nan and off_grid rows are moved to something not finite
    special = sorted(K.special_index(n, k) for k in ("nan", "off_grid"))
    for dtype in (K.F32, K.F64):
        for est in (None, K.STEP_ESTIMATE):
            moved, _ = K.model_step(rows, dtype, est, 3)
            bad = np.flatnonzero(K.non_finite_rows(moved)).tolist()      # (1e300 is finite as f64, an infinity as f32)
            assert K.special_index(n, "nan") in bad and set(bad) <= set(special)


def test_the_estimate_moves_rows_by_centimetres():
    rows = K.step_rows(257)
    moved, _ = K.model_step(rows, K.F64, K.STEP_ESTIMATE, 3)
    d = np.linalg.norm(moved[:200] - rows[:200], axis=1)
    assert 0.005 < d.min() and d.max() < 0.2
    angle = 2.0 * math.acos(K.STEP_ESTIMATE[3])
    assert 0.0 < math.degrees(angle) < 1.0


def test_scene_of_seed_1_meets_the_preconditions_of_the_gpu_test():
    left, exact = K.scene_run(1, False), K.scene_run(1, True)
    assert left[1] == exact[1] == 23 and left[2] == exact[2] == 2380 and left[3] and exact[3]
    for a, b in zip(left[4], exact[4]):                                # identical correspondences in every pass
        assert a["flags"] == b["flags"] and a["neighbours"] == b["neighbours"]
    # no rounding can change the pass count: the last dx . dx is a factor 4 below the criterion, every earlier one a factor 4 above
    c2 = K.SCENE_CONVERGENCE * K.SCENE_CONVERGENCE
    for run in (left, exact):
        norms = [R.squared_norm6(p["dx"]) for p in run[4]]
        assert norms[-1] < c2 / 4.0 and min(norms[:-1]) > 4.0 * c2
    d = K.pose_difference(left[0], exact[0])
    print("seed 1: passes %d, correspondences %d, |left fold - fsum| = %.3e" % (left[1], left[2], d))
    assert d <= K.MEASURED_POSE_DIFFERENCE
    # a realistic pair: the motion is found to the noise, most rows take part
    T, want = R.matrix(exact[0]), R.matrix(R.se3_exp(K.SCENE_MOTION))
    assert np.abs(T - want).max() < 0.02 and left[2] > 0.95 * K.SCENE_ROWS
    max_distance, kernel_scale = K.scene_parameters()
    assert (max_distance, kernel_scale) == (6.0, 2.0 / 3.0)
