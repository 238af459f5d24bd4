"""CPU-only: the source of the voxel kernels (csrc/k_voxel.hip) compiled for the host, one thread per lane (tests/cpp/voxel_lanes.cpp
over tests/cpp/host_lanes), against tests/voxel_model.py bit for bit, row order included.  The program calls the library's own
voxel_run: keys, hash insert (real threads race for the slots), ids, segments, gather, reduce and write are the library's source,
and so are the resets, the order of the steps and the number of bits the sort is given; only the two rocPRIM calls themselves are
stand-ins (a scan, and a stable sort that looks at the key bits it is given and no others).  It checks what can go wrong without a
GPU in sight -- the validity rules, the floor at negative coordinates, the order of every sum, strides, the compaction, what a
refusal leaves behind, the width of the sort; the device's own arithmetic and the C ABI around the kernels are
tests/test_gpu_voxel.py's business.
A stale workspace needs no test of its own: the program fills the header, the hash table (every slot held by row 0) and every other
array with junk before each run, so every case here of more than one voxel passes only if voxel_run resets what it must."""
import struct
import subprocess

import numpy as np
import pytest

import cpp_tools
import voxel_cases as K
import voxel_model as M

FORM_AVERAGE, FORM_FIRST, FORM_LAST, FORM_NORMALS = 0, 1, 2, 3


@pytest.fixture(scope="module")
def lanes():
    return cpp_tools.build("voxel_lanes")[0]


def run(exe, tmp_path, frame, voxel_size, form, min_pts=1, normals=None, dtype=np.float64, stride=None, table_log2=None, capacity=None):
    """-> (status, n_vox, n_out, out (capacity, cols), out_normals (capacity, 3))"""
    frame = np.asarray(frame)
    n, cols = frame.shape
    stride = stride or cols
    cap = n if capacity is None else capacity
    if table_log2 is None:
        table_log2 = max(1, int(2 * n - 1).bit_length())
    src = np.full((n, stride), 123.5, dtype)
    src[:, :cols] = frame
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("<6IdQQ", n, cols, stride, int(dtype == np.float32), form, table_log2, voxel_size, min_pts, cap))
        f.write(src.tobytes())
        if normals is not None:
            f.write(np.ascontiguousarray(normals, np.float64).tobytes())
    subprocess.check_call([exe, case, res], timeout=300)
    raw = open(res, "rb").read()
    status, n_vox, n_out = struct.unpack("<IIQ", raw[:16])
    body = np.frombuffer(raw[16:], np.float64)
    return status, n_vox, n_out, body[:cap * cols].reshape(cap, cols), body[cap * cols:].reshape(cap, 3)


def same(got, want, cols, what):
    status, _, n_out, out, out_n = got
    want_p, want_n = want if isinstance(want, tuple) else (want, None)
    assert status == 0 and n_out == len(want_p), (what, status, n_out, len(want_p))
    M.same_bits(out[:n_out], want_p.reshape(n_out, cols), what)
    assert (out[n_out:] == K.GUARD).all(), what
    if want_n is not None:
        M.same_bits(out_n[:n_out], want_n, what + " normals")
        assert (out_n[n_out:] == K.GUARD).all(), what
    else:
        assert (out_n == K.GUARD).all(), what


@pytest.mark.parametrize("cols", [3, 5, 9])
def test_average_with_threshold_and_attributes(lanes, tmp_path, cols):
    cloud = K.clustered_cloud(700, clusters=9, cols=cols, seed=cols)
    cloud[-3:, :3] += 100.0   # three voxels of one point each: below a threshold of 2
    for min_pts in (1, 2, 90):
        got = run(lanes, tmp_path, cloud, 1.0, FORM_AVERAGE, min_pts=min_pts)
        same(got, K.want(cloud, 1.0, 1, min_pts, M.AVERAGE_POINT), cols, "min_pts %d" % min_pts)
        assert got[1] == 12


def test_first_and_last_point_copies(lanes, tmp_path):
    cloud = K.clustered_cloud(600, clusters=5, cols=4, seed=11)
    same(run(lanes, tmp_path, cloud, 1.0, FORM_FIRST, min_pts=50), K.want(cloud, 1.0, 1, 50, M.FIRST_N_POINT), 4, "first")
    same(run(lanes, tmp_path, cloud, 1.0, FORM_LAST, min_pts=50), K.want(cloud, 1.0, 1, 50, M.RANDOM), 4, "last")
    M.same_bits(K.want(cloud, 1.0, 1, 1, M.RANDOM), M.last_point_wins(cloud, 1.0), "model: RANDOM with one slot")


def test_faces_negative_coordinates_and_zeros(lanes, tmp_path):
    cloud = K.face_cloud()
    for form, strategy in ((FORM_AVERAGE, M.AVERAGE_POINT), (FORM_FIRST, M.FIRST_N_POINT)):
        same(run(lanes, tmp_path, cloud, 0.5, form), K.want(cloud, 0.5, strategy=strategy), 3, "faces, form %d" % form)
    lone = np.array([[-0.0, -0.0, -0.0]])
    got = run(lanes, tmp_path, lone, 1.0, FORM_AVERAGE)
    same(got, K.want(lone, 1.0, strategy=M.AVERAGE_POINT), 3, "a lone -0.0")
    assert not np.signbit(got[3][0]).any()          # 0.0 + -0.0 is +0.0
    assert np.signbit(run(lanes, tmp_path, lone, 1.0, FORM_LAST)[3][0]).all()   # a copy keeps the sign


def test_float_input_strides_and_table_sizes(lanes, tmp_path):
    cloud = K.uniform_cloud(500, cols=4, seed=3, extent=4.0).astype(np.float32)
    expect = K.want(cloud, 0.7, strategy=M.AVERAGE_POINT)
    for log2 in (9, 10, 14):      # 512 slots for 500 points: nearly full
        same(run(lanes, tmp_path, cloud, 0.7, FORM_AVERAGE, dtype=np.float32, stride=7, table_log2=log2), expect, 4, "table 2^%d" % log2)
    line = K.line_cloud(300, diagonal=True)
    same(run(lanes, tmp_path, line, 1.0, FORM_LAST, table_log2=9), K.want(line, 1.0), 3, "diagonal")
    one = np.tile(np.array([[0.3, 0.4, 0.5, 1e16]]), (1000, 1))
    rng = np.random.default_rng(0)
    one[:, 3] = rng.uniform(-1.0, 1.0, 1000) * 10.0 ** rng.integers(-8, 9, 1000)   # a sum whose bits depend on its order
    same(run(lanes, tmp_path, one, 1.0, FORM_AVERAGE), K.want(one, 1.0, strategy=M.AVERAGE_POINT), 4, "one voxel")


def test_with_normals(lanes, tmp_path):
    pts, nrm = K.normals_cloud()
    expect = K.want(pts, 1.0, normals=nrm)
    same(run(lanes, tmp_path, pts, 1.0, FORM_NORMALS, normals=nrm), expect, 3, "with normals")
    same(run(lanes, tmp_path, pts.astype(np.float32), 1.0, FORM_NORMALS, normals=nrm, dtype=np.float32),
         K.want(pts.astype(np.float32), 1.0, normals=nrm), 3, "with normals, float points")
    # a skipped row may lie outside the grid; a row that takes part may not
    far = pts.copy()
    far[0] = 1e13
    keep = nrm.copy()
    keep[0] = 0.0
    same(run(lanes, tmp_path, far, 1.0, FORM_NORMALS, normals=keep), K.want(far, 1.0, normals=keep), 3, "skipped row outside the grid")
    keep[0] = [0.0, 0.0, 1.0]
    status, _, _, out, out_n = run(lanes, tmp_path, far, 1.0, FORM_NORMALS, normals=keep)
    assert status == 1 and (out == K.GUARD).all() and (out_n == K.GUARD).all()


def test_refusals_write_nothing(lanes, tmp_path):
    cloud = K.clustered_cloud(200, clusters=4, seed=21)
    for bad in (1e13, np.nan, -np.inf):
        c = cloud.copy()
        c[77, 1] = bad
        for form in (FORM_AVERAGE, FORM_FIRST):
            status, _, _, out, _ = run(lanes, tmp_path, c, 0.5, form)
            assert status == 1 and (out == K.GUARD).all(), (bad, form)
    c = cloud.copy()
    c[5, 0] = -2.0 ** 31 * 0.5          # floor(p / 0.5) == -2^31: the last voxel of the grid
    same(run(lanes, tmp_path, c, 0.5, FORM_AVERAGE), K.want(c, 0.5, strategy=M.AVERAGE_POINT), 3, "grid edge")
    c[5, 0] = 2.0 ** 31 * 0.5           # 2^31: one past it
    assert run(lanes, tmp_path, c, 0.5, FORM_AVERAGE)[0] == 1
    # an output one row short: the count, no row
    for form, strategy in ((FORM_AVERAGE, M.AVERAGE_POINT), (FORM_LAST, M.RANDOM)):
        status, _, n_out, out, _ = run(lanes, tmp_path, cloud, 1.0, form, capacity=3)
        assert status == 0 and n_out == 4 == len(K.want(cloud, 1.0, strategy=strategy)) and (out == K.GUARD).all()
        same(run(lanes, tmp_path, cloud, 1.0, form, capacity=4), K.want(cloud, 1.0, strategy=strategy), 3, "capacity 4")


# ---- the width of the sort: voxel_sort_bits(n) bits hold the ids 0 .. n; 255, 256 and 257 rows lie around the step from 8 to 9
def own_voxels(n, cols=4):
    """n rows, row i alone in voxel (i, 0, 0) of a voxel-1.0 grid: voxel ids 0 .. n - 1 in row order"""
    c = np.random.default_rng(n).uniform(0.05, 0.95, (n, cols))
    c[:, 0] += np.arange(n)
    return c


@pytest.mark.parametrize("n", [255, 256, 257])
def test_sort_width_every_row_a_voxel_of_its_own(lanes, tmp_path, n):
    """ids up to n - 1: with 255 rows they use the top bit of the 8-bit key.  On its own this order of ids cannot go wrong -- a
    voxel of one row is one segment wherever the sort puts it -- so the two tests below bring rows that a narrower sort tears apart"""
    cloud = own_voxels(n)
    for form, strategy in ((FORM_FIRST, M.FIRST_N_POINT), (FORM_AVERAGE, M.AVERAGE_POINT)):
        got = run(lanes, tmp_path, cloud, 1.0, form)
        same(got, K.want(cloud, 1.0, strategy=strategy), 4, "%d voxels of one row, form %d" % (n, form))
        assert got[1] == n


def test_sort_width_voxels_that_differ_in_the_top_bit_only(lanes, tmp_path):
    """255 rows, an 8-bit key: rows 0 .. 199 open voxels 0 .. 199, then voxels 0, 128, 1, 129, ... get a second row each.  A sort
    blind to bit 7 takes ids k and 128 + k for one and leaves their rows interleaved: k, 128 + k, k, 128 + k"""
    first = own_voxels(200)
    again = first[[k // 2 + 128 * (k % 2) for k in range(55)]] * [1.0, 0.5, 0.5, -3.0]     # the same cells, other rows
    cloud = np.vstack([first, again])
    assert len(cloud) == 255
    for form, strategy in ((FORM_FIRST, M.FIRST_N_POINT), (FORM_LAST, M.RANDOM), (FORM_AVERAGE, M.AVERAGE_POINT)):
        got = run(lanes, tmp_path, cloud, 1.0, form)
        same(got, K.want(cloud, 1.0, strategy=strategy), 4, "aliased ids, form %d" % form)
        assert got[1] == 200


@pytest.mark.parametrize("n", [256, 257])
def test_sort_width_a_skipped_row_has_the_largest_key(lanes, tmp_path, n):
    """With 256 and 257 rows the key has 9 bits, and bit 8 is set in one id only that these rows can produce together with a
    second row per voxel: n itself, the id of a row that takes no part.  Rows: voxel 0, voxel 1, a row with a zero normal, voxel 0
    again, voxel 1 again, then a voxel per row.  A sort blind to bit 8 reads 256 as 0 and 257 as 1, and puts the skipped row
    between the two rows of that voxel"""
    pts = own_voxels(n - 3, 3)
    pts = np.vstack([pts[:2], [[0.5, 0.5, 0.5]], pts[:2] * [1.0, 0.5, 0.5], pts[2:]])
    nrm = np.random.default_rng(n).normal(size=(n, 3))
    nrm[2] = 0.0
    assert len(pts) == n
    got = run(lanes, tmp_path, pts, 1.0, FORM_NORMALS, normals=nrm)
    same(got, K.want(pts, 1.0, normals=nrm), 3, "%d rows, one skipped" % n)
    assert got[1] == n - 3
