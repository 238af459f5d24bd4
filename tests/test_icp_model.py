"""tests/icp_model.py checked against what the reference publishes about point_to_point_align / point_to_plane_align: its two test
cases (python/tests/test_align_clouds.py, restated in tests/icp_cases.py, with the reference's own tolerances), its early returns, its
skip rules, its gate and its errors; and the model's solvers against numpy's."""
import math

import numpy as np
import pytest

import icp_cases as K
import icp_model as M


def test_published_point_to_point_case():
    src, tgt, shift = K.published_point()
    pose = M.point_to_point_align(src, tgt, max_corr_dist=0.5)
    np.testing.assert_allclose(pose[:3, :3], np.eye(3), atol=1e-10)
    np.testing.assert_allclose(pose[:3, 3], shift, atol=1e-10)
    exact = M.point_to_point_align(src, tgt, max_corr_dist=0.5, exact=True)
    np.testing.assert_allclose(exact, pose, atol=1e-14)


def test_published_point_to_plane_case():
    src, tgt, src_n, tgt_n = K.published_plane()
    pose = M.point_to_plane_align(src, tgt, src_n, tgt_n, max_corr_dist=0.5)
    np.testing.assert_allclose(pose[:3, :3], np.eye(3), atol=1e-10)
    np.testing.assert_allclose(pose[:3, 3], [0.0, 0.0, 0.2], atol=1e-9)


def test_nineteen_rows_on_either_side_return_the_guess():
    src, tgt, _ = K.published_point()
    guess = np.array(K.POSE_B)
    for a, b in ((src[:19], tgt), (src, tgt[:19])):
        pose, iterations, count, solved = M.align(M.POINT, a, b, None, None, guess, 0.5)
        assert np.array_equal(pose, guess) and (iterations, count, solved) == (0, 0, False)
    n = np.tile([0.0, 0.0, 1.0], (27, 1))
    pose, iterations, _, solved = M.align(M.PLANE, src[:19], tgt, n[:19], n, guess, 0.5)
    assert np.array_equal(pose, guess) and iterations == 0 and not solved
    assert M.align(M.POINT, src[:20], tgt, None, None, None, 0.5)[3]


def test_fewer_than_twenty_correspondences_return_the_guess():
    src, tgt, _ = K.published_point()
    far = tgt.copy()
    far[8:] += 100.0                      # 8 rows still match
    guess = np.eye(4)
    guess[0, 3] = 0.01
    pose, iterations, count, solved = M.align(M.POINT, src, far, None, None, guess, 0.5)
    assert np.array_equal(pose, guess) and (iterations, count, solved) == (1, 8, False)


def test_rows_that_take_no_part_are_ignored():
    src, tgt, shift = K.published_point()
    junk = np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [-np.inf, 0.0, 0.0]])
    want = M.point_to_point_align(src, tgt, max_corr_dist=0.5)
    got = M.point_to_point_align(np.vstack([junk, src]), np.vstack([tgt[:5], junk, tgt[5:]]), max_corr_dist=0.5)
    np.testing.assert_allclose(got, want, atol=1e-12)
    p, t, pn, tn = K.published_plane()
    want = M.point_to_plane_align(p, t, pn, tn, max_corr_dist=0.5)
    # a zero, a tiny and a NaN normal on either side: the row is as good as absent (its point is fine)
    extra = np.array([[0.5, 0.5, 0.0]] * 3)
    bad_n = np.array([[0.0, 0.0, 0.0], [0.0, 1e-13, 0.0], [np.nan, 0.0, 1.0]])
    got = M.point_to_plane_align(np.vstack([p, extra]), np.vstack([t, extra + [0.0, 0.0, 0.01]]), np.vstack([pn, bad_n]),
                                 np.vstack([tn, bad_n]), max_corr_dist=0.5)
    np.testing.assert_allclose(got, want, atol=1e-12)
    trace = []
    M.align(M.PLANE, np.vstack([p, extra]), np.vstack([t, extra + [0.0, 0.0, 0.01]]), np.vstack([pn, bad_n]), np.vstack([tn, bad_n]),
            None, 0.5, trace=trace)
    assert (trace[0]["nn"][25:] == -1).all() and not (trace[0]["nn"][:25] >= 25).any()


def test_gate_of_0_and_of_180_degrees():
    p, t, pn, tn = K.published_plane()
    tilted = pn + [0.05, 0.0, 0.0]          # 2.9 degrees off
    guess = np.eye(4)
    # 0 degrees: cos = 1, only exactly parallel unit normals pass; the tilted ones leave no correspondence
    pose, _, count, solved = M.align(M.PLANE, p, t, tilted, tn, guess, 0.5, 0.0)
    assert count == 0 and not solved and np.array_equal(pose, guess)
    assert M.align(M.PLANE, p, t, pn, tn, guess, 0.5, 0.0)[2] == 25
    # 180 degrees: cos = -1, |dot| >= -1 always: even normals at a right angle pass
    side = np.tile([1.0, 0.0, 0.0], (25, 1))
    assert M.align(M.PLANE, p, t, side, tn, guess, 0.5, 180.0)[2] == 25
    assert M.align(M.PLANE, p, t, side, tn, guess, 0.5, 20.0)[2] == 0


def test_every_error():
    src, tgt, _ = K.published_point()
    n = np.tile([0.0, 0.0, 1.0], (27, 1))
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="max_corr_dist must be finite and greater than zero"):
            M.point_to_point_align(src, tgt, max_corr_dist=bad)
        with pytest.raises(ValueError, match="max_corr_dist must be finite and greater than zero"):
            M.point_to_plane_align(src, tgt, n, n, max_corr_dist=bad, max_normal_angle_deg=-1.0)   # the first check wins
    for bad in (-0.5, 180.5, math.nan, math.inf):
        with pytest.raises(ValueError, match=r"max_normal_angle_deg must be finite and in \[0, 180\]"):
            M.point_to_plane_align(src, tgt, n[:5], n, max_normal_angle_deg=bad)
    with pytest.raises(ValueError, match="source_points and source_normals must have the same number of rows"):
        M.point_to_plane_align(src, tgt, n[:5], n[:6])
    with pytest.raises(ValueError, match="target_points and target_normals must have the same number of rows"):
        M.point_to_plane_align(src, tgt, n, n[:6])
    out = tgt.copy()
    out[3, 1] = 3e9                          # cell 1.2e10 at max_corr_dist 0.25
    with pytest.raises(ValueError, match="point_to_point_align: target point outside the int32 cell grid"):
        M.point_to_point_align(src, out)
    with pytest.raises(ValueError, match="point_to_plane_align: target point outside the int32 cell grid"):
        M.point_to_plane_align(src, out, n, n)
    bad_n = n.copy()
    bad_n[3] = 0.0                           # ... unless the row takes no part
    M.point_to_plane_align(src, out, n, bad_n)


def test_nearest_tie_and_distance_rules():
    tgt, _ = K.tie_target(False)
    grid = M.build_grid(tgt, None, K.CELL)
    d2 = K.CELL * K.CELL
    ax = [-1.0, -0.5, 0.0, 0.5, 1.0, 1.5]
    index = {(x, y, z): i for i, (x, y, z) in enumerate((x, y, z) for x in ax for y in ax for z in ax)}
    # two at 0.25 across a cell face: the cell visited first (dx = -1) holds (0, 0, 0)... which is the query's own cell here, since
    # floor(0.25 / 0.5) = 0: visiting order is by cell, (-1, ..) cells first, and the first row found keeps the tie
    assert M.nearest(grid, tgt, [0.25, 0.0, 0.0], d2) == index[(0.0, 0.0, 0.0)]
    assert M.nearest(grid, tgt, [0.25, 0.25, 0.25], d2) == index[(0.0, 0.0, 0.0)]
    assert M.nearest(grid, tgt, [-0.75, -0.75, -0.75], d2) == index[(-1.0, -1.0, -1.0)]
    # a duplicated row: the lower index wins
    assert M.nearest(grid, tgt, [-1.0, -1.0, -1.0], d2) == 0
    # exactly max_corr_dist away is no match; half of it is
    assert M.nearest(grid, tgt, [10.5, 10.0, 10.0], d2) == -1
    assert M.nearest(grid, tgt, [10.25, 10.0, 10.0], d2) == 216
    assert M.nearest(grid, tgt, [math.nan, 0.0, 0.0], d2) == -1 and M.nearest(grid, tgt, [1e12, 0.0, 0.0], d2) == -1


def test_median_and_huber():
    assert M.median_abs([3.0, -1.0, 2.0]) == 2.0
    assert M.median_abs([3.0, -1.0, 2.0, -8.0]) == 0.5 * (2.0 + 3.0)
    assert M.median_abs([]) == 0.0
    assert M.huber_delta(0.0, 0.5) == 1.5 * 0.125 and M.huber_delta(0.0, 0.001) == 1.5 * 1e-3
    assert M.huber_delta(math.nan, 0.5) == 1.5 * 0.125 and M.huber_delta(0.01, 0.5) == 1.5 * (1.4826 * 0.01)
    assert M.weight(0.1, 0.2) == 1.0 and M.weight(-0.4, 0.2) == 0.2 / 0.4 and M.weight(5.0, 0.0) == 1.0


def test_solvers_agree_with_numpy():
    rng = np.random.default_rng(3)
    for k in range(20):
        a = rng.normal(size=(3, 3)) * 10.0 ** rng.integers(-3, 4)
        if k % 5 == 0:
            a[:, 2] = a[:, 0] * 0.5 - a[:, 1]         # rank 2: the third left vector is the cross product of the other two
        u, s, v = M.svd3(a.tolist())
        np.testing.assert_allclose(np.array(u) @ np.diag(s) @ np.array(v).T, a, atol=1e-12 * np.abs(a).max())
        np.testing.assert_allclose(s, np.linalg.svd(a, compute_uv=False), atol=1e-12 * np.abs(a).max())
        np.testing.assert_allclose(np.array(u).T @ np.array(u), np.eye(3), atol=1e-12)
        h = rng.normal(size=(6, 6))
        h = h @ h.T + np.eye(6) * 1e-3
        b = rng.normal(size=6)
        np.testing.assert_allclose(M.ldlt6(h.tolist(), b.tolist()), np.linalg.solve(h, b), rtol=1e-8)
    assert M.svd3([[1.0, 0.0, 0.0], [2.0, 0.0, 0.0], [3.0, 0.0, 0.0]]) is None        # rank 1: no rotation is determined
    assert M.ldlt6((-np.eye(6)).tolist(), [1.0] * 6) is None


def test_realistic_pair_recovers_the_move():
    src, src_n, tgt, tgt_n, move = K.realistic_pair(1)
    for method in (M.POINT, M.PLANE):
        pose, iterations, count, solved = M.align(method, src, tgt, src_n if method else None, tgt_n if method else None, None,
                                                  K.REAL_DIST)
        assert solved and count > len(src) // 2 and 1 < iterations <= M.MAX_ITERATIONS
        assert np.abs(pose - move).max() < 5e-3
