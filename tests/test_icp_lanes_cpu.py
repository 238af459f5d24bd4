"""CPU-only: the source of the ICP grid kernels and of k_icp_correspond (csrc/k_icp.hip, over the cell table of csrc/k_voxel.hip)
compiled for the host, one thread per lane (tests/cpp/icp_lanes.cpp over tests/cpp/host_lanes/hip/hip_runtime.h), against
tests/icp_model.py bit for bit: the neighbour index and the residual of every row of the tie cases of tests/icp_cases.py, guard
elements behind both.  The grid is built by the library's own icp_grid_run: keys, hash insert (real threads race for the slots),
ids, segments, slots and gather are the library's source, and so are the resets, the order of the steps and the number of bits the
sort is given; only the two rocPRIM calls themselves are stand-ins (a scan, and a stable sort that looks at the key bits it is given
and no others).  The program fills the read-back, the table and every other array with junk before the run, so every case passes
only if the run resets what it must.  The sum kernels (k_icp_sums_point_a /
_b, k_icp_sums_plane), k_icp_median and k_icp_fold use cross-lane operations or device-only launches and are covered on the GPU only
(tests/test_gpu_icp.py)."""
import struct
import subprocess

import numpy as np
import pytest

import cpp_tools
import icp_cases as K
import icp_model as M


@pytest.fixture(scope="module")
def lanes():
    return cpp_tools.build("icp_lanes")[0]


def run(exe, tmp_path, arrays, pose, max_corr_dist, angle, table_log2=None):
    """-> (status, cells, nn with guard, r with guard)"""
    src, tgt, src_n, tgt_n = arrays["src"], arrays["tgt"], arrays["src_n"], arrays["tgt_n"]
    plane = src_n is not None
    n_src, n_tgt = len(src), len(tgt)
    if table_log2 is None:
        table_log2 = max(1, int(2 * n_tgt - 1).bit_length())
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("<10I", n_src, n_tgt, src.shape[1], tgt.shape[1], src_n.shape[1] if plane else 3, tgt_n.shape[1] if plane else 3,
                            int(src.dtype == np.float32), int(plane), table_log2, 0))
        f.write(struct.pack("<18d", max_corr_dist, M.cos_gate(angle) if plane else 0.0, *np.asarray(pose, dtype=np.float64).reshape(-1)))
        for a in (src, tgt) + ((src_n, tgt_n) if plane else ()):
            f.write(np.ascontiguousarray(a).tobytes())
    subprocess.check_call([exe, case, res], timeout=300)
    raw = open(res, "rb").read()
    status, cells = struct.unpack("<II", raw[:8])
    nn = np.frombuffer(raw[8:8 + 4 * (n_src + 16)], np.int32)
    r = np.frombuffer(raw[8 + 4 * (n_src + 16):], np.float64)
    return status, cells, nn, r


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
@pytest.mark.parametrize("n,variant", [(20, 0), (63, 0), (65, 1), (257, 0), (1041, 1)])
def test_correspondences_equal_the_model_bit_for_bit(lanes, tmp_path, n, plane, variant):
    arrays, pose = K.tie_case(n, plane, variant)
    want = K.tie_model(n, plane, variant)
    for log2 in (None, 9):      # the automatic table and 512 slots for 240 rows: long probe chains
        status, cells, nn, r = run(lanes, tmp_path, arrays, pose, K.CELL, K.tie_gate(n), log2)
        assert status == 0 and cells > 100
        assert (nn[n:] == -77).all() and (r[n:] == -7.25).all()
        assert np.array_equal(nn[:n], want["nn"]), np.flatnonzero(nn[:n] != want["nn"])[:10]
        assert K.same_bits(r[:n], want["r"])


def test_a_target_outside_the_grid_sets_the_status_and_nothing_else(lanes, tmp_path):
    src, tgt, _ = K.published_point()
    n = np.tile([0.0, 0.0, 1.0], (27, 1))
    far = tgt.copy()
    far[3, 1] = 3e9
    for normals in ((None, None), (n, n)):
        status, _, nn, r = run(lanes, tmp_path, dict(src=src, tgt=far, src_n=normals[0], tgt_n=normals[1]), np.eye(4), 0.25, 20.0)
        assert status == 1 and (nn == -77).all() and (r == -7.25).all()
    bad_n = n.copy()
    bad_n[3] = 0.0              # the row takes no part: no refusal, and its neighbours answer for it
    status, _, nn, _ = run(lanes, tmp_path, dict(src=src, tgt=far, src_n=n, tgt_n=bad_n), np.eye(4), 0.25, 20.0)
    grid = M.build_grid(far, bad_n, 0.25)
    want = M.correspond(np.eye(4), src, far, n, bad_n, grid, 0.25, 20.0)[0]
    assert status == 0 and np.array_equal(nn[:27], want) and nn[3] == -1


# ---- the width of the grid's sort: voxel_sort_bits(n_tgt) bits hold the cell ids 0 .. n_tgt (tests/test_voxel_lanes_cpu.py has the
# same three cases on the voxel route)
def own_cells(n):
    """n target rows, row i alone in cell (i, 0, 0) of a K.CELL grid: cell ids 0 .. n - 1 in row order"""
    c = np.random.default_rng(n).uniform(0.05, 0.45, (n, 3))
    c[:, 0] += K.CELL * np.arange(n)
    return c


def other_row_of(rows):
    """a second row for each cell of `rows`: mirrored within the cell in y and z"""
    out = rows.copy()
    out[:, 1:] = K.CELL - out[:, 1:]
    return out


def check_against_the_model(lanes, tmp_path, tgt, cells):
    """a source row 1 mm beside every target row (beside the cell's middle where the target row is not finite)"""
    src = np.where(np.isfinite(tgt), tgt, 0.25) + 0.001
    grid = M.build_grid(tgt, None, K.CELL)
    want_nn, want_r, _, _ = M.correspond(np.eye(4), src, tgt, None, None, grid, K.CELL)
    status, got_cells, nn, r = run(lanes, tmp_path, dict(src=src, tgt=tgt, src_n=None, tgt_n=None), np.eye(4), K.CELL, 20.0)
    n = len(src)
    assert status == 0 and got_cells == cells
    assert (nn[n:] == -77).all() and (r[n:] == -7.25).all()
    assert np.array_equal(nn[:n], want_nn), np.flatnonzero(nn[:n] != want_nn)[:10]
    assert K.same_bits(r[:n], np.asarray(want_r))
    return nn[:n]


@pytest.mark.parametrize("n", [255, 256, 257])
def test_sort_width_every_target_row_a_cell_of_its_own(lanes, tmp_path, n):
    """ids up to n - 1: with 255 rows they use the top bit of the 8-bit key.  A cell of one row is one segment wherever the sort
    puts it, so the two tests below bring rows that a narrower sort tears apart"""
    nn = check_against_the_model(lanes, tmp_path, own_cells(n), n)
    assert np.array_equal(nn, np.arange(n))


def test_sort_width_cells_that_differ_in_the_top_bit_only(lanes, tmp_path):
    """255 target rows, an 8-bit key: rows 0 .. 199 open cells 0 .. 199, then cells 0, 128, 1, 129, ... get a second row each.  A
    sort blind to bit 7 leaves the rows of cells k and 128 + k interleaved, and a query finds half a cell"""
    first = own_cells(200)
    tgt = np.vstack([first, other_row_of(first[[k // 2 + 128 * (k % 2) for k in range(55)]])])
    nn = check_against_the_model(lanes, tmp_path, tgt, 200)
    assert np.array_equal(nn, np.arange(255))


@pytest.mark.parametrize("n", [256, 257])
def test_sort_width_a_row_that_takes_no_part_has_the_largest_key(lanes, tmp_path, n):
    """With 256 and 257 rows the key has 9 bits, and beside cells of two rows bit 8 is set in one id only: n itself, that of a row
    that takes no part.  Rows: cell 0, cell 1, a row that is not finite, cell 0 again, cell 1 again, then a cell per row.  A sort
    blind to bit 8 reads 256 as 0 and 257 as 1 and puts that row between the two rows of the cell"""
    first = own_cells(n - 3)
    tgt = np.vstack([first[:2], [[np.nan, 0.1, 0.1]], other_row_of(first[:2]), first[2:]])
    assert len(tgt) == n
    nn = check_against_the_model(lanes, tmp_path, tgt, n - 3)
    assert np.array_equal(np.delete(nn, 2), np.delete(np.arange(n), 2))
