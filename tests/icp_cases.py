"""Inputs and call helpers the ICP tests share (tests/test_icp_model.py, test_icp_api_cpu.py, test_gpu_icp.py): the reference's two
published cases, clouds built so that the tie rules decide, the realistic pair from tests/golden/icp_voxels.npz, and the C ABI
through ctypes."""
import ctypes as C
import functools
import math
import os

import numpy as np

import icp_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
CELL = 0.5          # max_corr_dist of the built cases: the lattice below has this spacing
GUARD = 16          # elements behind every per-row output
GUARD_NN, GUARD_R = -77, -7.25

# the realistic pair: the golden voxel rows moved by MOVE (a rotation vector and a translation, both well inside max_corr_dist)
# with gaussian noise of NOISE m on the target
MOVE = (0.004, -0.003, 0.006, 0.03, -0.02, 0.015)
NOISE = 0.002
REAL_DIST = 0.25


def published_point():
    """the 3x3x3 lattice on {-1, 0, 1}^3 against itself shifted by (0.1, -0.05, 0.025); max_corr_dist 0.5"""
    g = np.array([[x, y, z] for x in (-1.0, 0.0, 1.0) for y in (-1.0, 0.0, 1.0) for z in (-1.0, 0.0, 1.0)])
    shift = np.array([0.1, -0.05, 0.025])
    return g, g + shift, shift


def published_plane():
    """the 5x5 integer plane z = 0 against z = 0.2, +z normals; max_corr_dist 0.5"""
    p = np.array([[float(x), float(y), 0.0] for x in range(5) for y in range(5)])
    n = np.tile([0.0, 0.0, 1.0], (25, 1))
    return p, p + np.array([0.0, 0.0, 0.2]), n, n.copy()


def tie_target(plane):
    """A lattice of spacing CELL on [-1, 1.5]^3 -- every coordinate an exact multiple of the cell size, negative ones included --
    with its first rows duplicated at the end, one far row, and rows that take no part (NaN, inf; with normals: zero, NaN)."""
    ax = [-1.0, -0.5, 0.0, 0.5, 1.0, 1.5]
    lat = np.array([[x, y, z] for x in ax for y in ax for z in ax])
    far = np.array([[10.0, 10.0, 10.0]])
    bad = np.array([[np.nan, 0.0, 0.0], [0.25, np.inf, 0.25], [0.1, 0.1, -np.inf]])
    pts = np.vstack([lat, far, bad, lat[:12], lat[100:104]])
    if not plane:
        return pts, None
    rng = np.random.default_rng(5)
    nrm = np.tile([0.0, 0.0, 1.0], (len(pts), 1)) * rng.uniform(0.3, 3.0, (len(pts), 1))   # non-unit
    nrm[::7] = nrm[::7] + rng.uniform(-0.4, 0.4, (len(nrm[::7]), 3))                           # tilted: some past the gate
    nrm[5] = 0.0                       # a lattice row that takes no part: its neighbours win instead
    nrm[17] = [np.nan, 0.0, 1.0]
    nrm[40] = [1e-13, 0.0, 0.0]
    nrm[41] = [0.0, -2.0, 0.0]         # at a right angle to every source normal: found, then gated out
    return pts, nrm


def tie_source(n, plane, seed):
    """n query rows: equidistant from 2, 4 and 8 lattice rows (across a face, an edge, a corner of the cells), on lattice rows, next to
    the duplicated rows, exactly CELL from the far row (no match) and half of that (a match), then uniform ones; from 63 rows on
    also rows that take no part."""
    special = [[0.25, 0.0, 0.0], [-0.75, 0.5, -1.0], [0.25, 0.25, 0.0], [-0.25, -0.25, 0.5], [0.25, 0.25, 0.25], [-0.75, -0.75, -0.75],
               [0.0, 0.0, 0.0], [-1.0, -1.0, -1.0], [-1.0, -1.0, -0.75], [1.5, 1.5, 1.5], [10.5, 10.0, 10.0], [10.0, 10.0, 9.5],
               [10.25, 10.0, 10.0], [0.5, 0.25, 1.0], [1.25, -0.5, 0.25], [-0.5, 0.0, 0.75]]
    if n < 63:
        special = special[:10] + special[12:]      # the smallest case keeps every row matched: a count of exactly 20
    rng = np.random.default_rng(seed)
    rows = np.vstack([np.array(special), rng.uniform(-1.2, 1.7, (max(n - len(special), 0), 3))])[:n]
    order = rng.permutation(n)
    rows = rows[order]
    nrm = None
    if plane:
        nrm = np.tile([0.0, 0.0, 1.0], (n, 1)) * rng.uniform(0.2, 5.0, (n, 1)) + rng.uniform(-0.15, 0.15, (n, 3))
    if n >= 63:
        rows[11] = [np.nan, 0.0, 0.0]
        rows[29] = [0.0, np.inf, 0.0]
        rows[47] = [1e12, 0.0, 0.0]        # its cell no int32 holds: no neighbour
        if plane:
            nrm[13] = 0.0
            nrm[31] = [0.0, np.nan, 1.0]
            nrm[33] = [0.0, 0.0, 1e-13]
    return rows, nrm


def tie_gate(n):
    """max_normal_angle_deg of a tie case: the reference's default; wide open for the smallest, so that its 20 rows all count"""
    return 180.0 if n == 20 else 20.0


POSE_B = [[math.cos(0.3), -math.sin(0.3), 0.0, 0.04], [math.sin(0.3), math.cos(0.3), 0.0, -0.03], [0.0, 0.0, 1.0, 0.02],
          [0.0, 0.0, 0.0, 1.0]]


def unpose(pose, rows):
    """rows moved by the inverse of `pose`, so that the queries land near where tie_source put them"""
    p = np.array(pose)
    with np.errstate(invalid="ignore"):        # the rows that take no part stay NaN / inf
        return (rows - p[:3, 3]) @ p[:3, :3]


@functools.lru_cache(maxsize=None)
def tie_case(n, plane, variant):
    """variant 0: identity pose, float64, dense.  1: POSE_B, float32 rows with a stride of 5 (normals 4)."""
    tgt, tgt_n = tie_target(plane)
    src, src_n = tie_source(n, plane, 100 + n)
    pose = np.eye(4)
    if variant == 1:
        pose = np.array(POSE_B)
        src = unpose(pose, src)
        if plane:
            src_n = src_n @ pose[:3, :3]
    dtype, strides = (np.float32, (5, 4)) if variant == 1 else (np.float64, (3, 3))

    def lay(a, stride):
        if a is None:
            return None
        out = np.full((len(a), stride), 123.0, dtype)
        out[:, :3] = a.astype(dtype)
        return out

    arrays = dict(src=lay(src, strides[0]), tgt=lay(tgt, strides[0]), src_n=lay(src_n, strides[1]), tgt_n=lay(tgt_n, strides[1]))
    for a in arrays.values():
        if a is not None:
            a.setflags(write=False)
    return arrays, pose


@functools.lru_cache(maxsize=None)
def tie_model(n, plane, variant):
    """the model's pass for tie_case"""
    a, pose = tie_case(n, plane, variant)
    src, tgt = M.widen(a["src"]), M.widen(a["tgt"])
    src_n = M.widen(a["src_n"]) if plane else None
    tgt_n = M.widen(a["tgt_n"]) if plane else None
    grid = M.build_grid(tgt, tgt_n, CELL)
    return M.step(M.PLANE if plane else M.POINT, pose, src, tgt, src_n, tgt_n, grid, CELL, tie_gate(n))


@functools.lru_cache(maxsize=None)
def golden_voxels():
    z = np.load(os.path.join(HERE, "golden", "icp_voxels.npz"))
    return np.ascontiguousarray(z["points"]), np.ascontiguousarray(z["normals"])


def move_matrix():
    import pose_model as P
    return np.array(P.pose_exp([float(v) for v in MOVE]), dtype=np.float64)


@functools.lru_cache(maxsize=None)
def realistic_pair(seed):
    """(source points, source normals, target points, target normals, the move)"""
    pts, nrm = golden_voxels()
    move = move_matrix()
    rng = np.random.default_rng(seed)
    tgt = pts @ move[:3, :3].T + move[:3, 3] + rng.normal(0.0, NOISE, pts.shape)
    tgt_n = nrm @ move[:3, :3].T
    return pts, nrm, tgt, tgt_n, move


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def make_desc(capi, src, tgt, src_n=None, tgt_n=None, guess=None, max_corr_dist=0.25, max_normal_angle_deg=20.0, ptr=None, rows=None):
    """-> (IcpDesc, what must stay alive).  ptr: array -> address (host arrays by default).  rows: overrides of the four counts."""
    ptr = ptr or (lambda a: a.ctypes.data)
    d = capi.IcpDesc()
    keep = []

    def put(a):
        if a is None:
            return None, 0, 0
        a = np.asarray(a)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        a = np.ascontiguousarray(a)
        keep.append(a)
        return (ptr(a) if len(a) else ptr(np.zeros((1, 3), a.dtype))), len(a), (a.shape[1] if a.ndim == 2 else 3)

    d.source_points, d.n_source, d.source_stride = put(src)
    d.target_points, d.n_target, d.target_stride = put(tgt)
    d.source_normals, d.n_source_normals, d.source_normal_stride = put(src_n)
    d.target_normals, d.n_target_normals, d.target_normal_stride = put(tgt_n)
    for k, v in (rows or {}).items():
        setattr(d, k, v)
    d.dtype = capi.F32 if keep and keep[0].dtype == np.float32 else capi.F64
    g = np.eye(4) if guess is None else np.asarray(guess, dtype=np.float64).reshape(4, 4)
    d.initial_guess[:] = g.reshape(-1).tolist()
    d.max_corr_dist, d.max_normal_angle_deg = max_corr_dist, max_normal_angle_deg
    d.pose[:] = [GUARD_R] * 16
    d.iterations, d.solved, d.correspondences = 777, 777, 777
    return d, keep


def desc_untouched(d):
    return list(d.pose) == [GUARD_R] * 16 and (d.iterations, d.solved, d.correspondences) == (777, 777, 777)


def desc_pose(d):
    return np.array(list(d.pose)).reshape(4, 4)


def step_ref(capi, d, pose):
    """ouster_hip_icp_step_ref -> (rc, IcpStepOut, nn, r)"""
    n = d.n_source
    nn = np.full(n + GUARD, GUARD_NN, np.int32)
    r = np.full(n + GUARD, GUARD_R, np.float64)
    out = capi.IcpStepOut()
    out.nn, out.r = nn.ctypes.data, r.ctypes.data
    p = (C.c_double * 16)(*np.asarray(pose, dtype=np.float64).reshape(-1).tolist())
    rc = capi.load_hip().ouster_hip_icp_step_ref(C.byref(d), p, C.byref(out))
    return rc, out, nn, r


def same_bits(a, b):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes() == np.ascontiguousarray(b, dtype=np.float64).tobytes()


def pose_margin(measured, truth_t):
    """what a pose may differ from the exact-sum model by: 8 x the measured left-fold / exact difference, with the floor of the issue"""
    return max(8.0 * measured, 8.0 * 2.0 ** -52 * max(1.0, float(np.abs(truth_t).max())))
