"""What the voxel tests share: the ctypes call of the C ABI on numpy arrays with guard rows behind every output, the model's
answer for the same desc, and the clouds.  No test in here."""
import ctypes as C

import numpy as np

import voxel_model as M
from ouster_sdk_amd import _capi as capi

GUARD_ROWS = 3
GUARD = -7.25   # what every output element holds before a call


def recorded_case():
    """python/tests/test_core.py:486-507 of the reference: 4 points with 2 attributes -> (frame, [(voxel_size, rows)])"""
    pts = np.array([[0.0, 1.0, 0.0], [0.0, 1.0, 0.0], [0.0, 2.0, 0.0], [0.0, 2.0, 0.0]])
    attrs = np.array([[10.0, 100.0], [12.0, 102.0], [20.0, 200.0], [22.0, 202.0]])
    frame = np.hstack([pts, attrs])
    return frame, [(0.1, np.array([[0, 2, 0, 21, 201], [0, 1, 0, 11, 101]], np.float64)),
                   (4.0, np.array([[0, 1.5, 0, 16, 151]], np.float64))]


def uniform_cloud(n, cols=3, seed=1, extent=50.0):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-extent, extent, (n, cols))
    return a


def clustered_cloud(n=4096, clusters=7, cols=3, seed=2):
    """n points in `clusters` voxels of size 1.0, interleaved so that every voxel's points arrive all through the input"""
    rng = np.random.default_rng(seed)
    centre = rng.integers(-20, 20, (clusters, 3)).astype(np.float64)
    which = rng.integers(0, clusters, n)
    which[:clusters] = np.arange(clusters)
    a = np.empty((n, cols))
    a[:, :3] = centre[which] + rng.uniform(0.05, 0.95, (n, 3))
    a[:, 3:] = rng.uniform(-1000.0, 1000.0, (n, cols - 3))
    return a


def line_cloud(n=4096, diagonal=False):
    """n distinct voxels of size 1.0 along the x axis or the main diagonal"""
    k = np.arange(n, dtype=np.float64) - n // 2
    a = np.zeros((n, 3))
    a[:, 0] = k + 0.5
    if diagonal:
        a[:, 1] = k + 0.25
        a[:, 2] = k + 0.75
    return a


def face_cloud():
    """points exactly on voxel faces at voxel size 0.5, negative coordinates and both zeros"""
    v = np.array([-1.0, -0.5, -0.25, -0.0, 0.0, 0.25, 0.5, 1.0, -1e-300, 1e-300])
    g = np.stack(np.meshgrid(v, v[::-1], v, indexing="ij"), -1).reshape(-1, 3)
    return np.ascontiguousarray(g)


def normals_cloud(n=600, seed=5):
    """points in a few dozen voxels of size 1.0 with normals of every awkward kind -> (points, normals)"""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-3.0, 3.0, (n, 3))
    nrm = rng.normal(size=(n, 3)) * rng.uniform(0.1, 10.0, (n, 1))      # non-unit
    nrm[::7] = 0.0                                                         # zero normals
    nrm[3::31] = 1e-13                                                     # shorter than 1e-12
    pts[5::41, 1] = np.nan
    pts[6::43, 2] = np.inf
    nrm[8::37, 0] = np.nan
    nrm[9::39, 2] = -np.inf
    # a voxel that holds n and -n only: dropped
    pts = np.vstack([pts, [[10.2, 10.2, 10.2], [10.7, 10.7, 10.7]]])
    nrm = np.vstack([nrm, [[0.6, 0.0, 0.8], [-0.6, 0.0, -0.8]]])
    # a voxel whose normals nearly cancel: kept, with a tiny sum
    pts = np.vstack([pts, [[20.2, 10.2, 10.2], [20.7, 10.7, 10.7]]])
    nrm = np.vstack([nrm, [[0.6, 0.0, 0.8], [-0.6, 1e-9, -0.8]]])
    return np.ascontiguousarray(pts), np.ascontiguousarray(nrm)


def want(frame, voxel_size, max_points=1, min_pts=1, strategy=M.RANDOM, normals=None):
    """the model's rows for a desc -> out, or (out, out_normals)"""
    frame = np.asarray(frame, np.float64)
    if normals is not None:
        return M.voxel_downsample_with_normals(frame, normals, voxel_size)
    return M.voxel_downsample_xd(frame, voxel_size, max_points, min_pts, strategy)


def call(fn, ctx, frame, voxel_size, max_points=1, min_pts=1, strategy=M.RANDOM, normals=None, dtype=np.float64, row_stride=0,
         table_log2=0, capacity=None, to_device=None, from_device=None):
    """One C ABI call on `frame` (n, cols).  fn: ouster_hip_voxel_downsample_ref (ctx None and not passed), _host or the device form
    (to_device / from_device move arrays).  Outputs are filled with GUARD and carry GUARD_ROWS rows past `capacity`.
    -> (rc, n_out, out, out_normals): the whole output arrays, guard rows included."""
    frame = np.asarray(frame)
    n, cols = frame.shape
    stride = row_stride or cols
    src = np.full((max(n, 1), stride), 123.5, dtype)
    src[:n, :cols] = frame
    cap = n if capacity is None else capacity
    out = np.full((cap + GUARD_ROWS, cols), GUARD)
    out_n = np.full((cap + GUARD_ROWS, 3), GUARD)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float64)
    d = capi.VoxelDesc()
    d.n, d.cols, d.row_stride, d.out_capacity = n, cols, row_stride, cap
    d.dtype = capi.F32 if dtype == np.float32 else capi.F64
    d.voxel_size, d.max_points_per_voxel, d.min_pts_threshold, d.strategy = voxel_size, max_points, min_pts, strategy
    d.table_log2 = table_log2
    held = [src, out, out_n, nrm]
    if to_device is None:
        d.points, d.out, d.out_normals = src.ctypes.data, out.ctypes.data, out_n.ctypes.data
        if nrm is not None:
            d.normals = nrm.ctypes.data if nrm.size else out_n.ctypes.data
    else:
        dev = [to_device(a) if a is not None else None for a in held]
        d.points, d.out, d.out_normals = dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr()
        if nrm is not None:
            d.normals = dev[3].data_ptr()
    n_out = C.c_uint64(12345)
    rc = fn(C.byref(d), C.byref(n_out)) if ctx is False else fn(ctx, C.byref(d), C.byref(n_out))
    if to_device is not None:
        out, out_n = from_device(dev[1]), from_device(dev[2])
    return rc, int(n_out.value), out, out_n


def check_rows(res, expect, cols, what=""):
    """res of call(); expect: the model's rows (or pair).  Bit for bit, row order included, everything past the rows untouched."""
    rc, n_out, out, out_n = res
    assert rc == capi.OK, (what, rc, capi.load_hip().ouster_hip_last_error())
    exp_p, exp_n = expect if isinstance(expect, tuple) else (expect, None)
    assert n_out == len(exp_p), (what, n_out, len(exp_p))
    M.same_bits(out[:n_out], exp_p.reshape(n_out, cols), what)
    assert (out[n_out:] == GUARD).all(), what + ": rows past the result were written"
    if exp_n is not None:
        M.same_bits(out_n[:n_out], exp_n, what + " (normals)")
        assert (out_n[n_out:] == GUARD).all(), what + ": normal rows past the result were written"
    else:
        assert (out_n == GUARD).all(), what


def check_untouched(res, rc_want, what=""):
    rc, n_out, out, out_n = res
    assert rc == rc_want, (what, rc)
    assert (out == GUARD).all() and (out_n == GUARD).all(), what + ": a refused call wrote output"
    return n_out
