"""algorithm::normals on the GPU, bit for bit against tests/normals_model.py: the kernel has only IEEE add / multiply / divide / sqrt
in f64 with contraction off, and its three transcendental constants come from the host's libm, like the model's.  Results are
compared as 64-bit patterns (so -0.0 is not 0.0).  Device outputs lie between guard bytes of 0xCD that must stay.

The synthetic scene: a tilted plane and a sphere in front of it seen from the origin, ranges in mm, the plane behind the sphere
as second return; 10 % of the pixels, whole rows and whole columns (column W / 2 among them: the subtent search has to walk
outward) without range; a one-pixel-wide pole 600 mm in front of the plane (thin foreground); at (64, 256) also a pixel whose
upper and lower neighbour lie at exactly the same distance (the tie goes to the first visited) and pixels at the origin itself
(no beam: they fall through every case)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import normals_model as M
from conftest import ROOT, has_gpu

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "ouster_sdk_amd", "compat"))
GUARD = 256
TILE_H, TILE_W = 4, 64   # NORMALS_TILE_H / NORMALS_TILE_W of csrc/k_normals.h; the kernel stages no halo (halo 0)


@pytest.fixture(scope="module")
def gpu():
    import torch
    from ouster_sdk_amd import _capi as capi
    assert has_gpu()
    ctx = capi.Context(0)
    yield capi, ctx, torch
    ctx.close()


@functools.lru_cache(maxsize=None)
def scene(h, w, seed=5, zero=False):
    """-> xyz (h*w,3) f64, range (h,w) u32, xyz2, range2: destaggered, read-only"""
    rng = np.random.default_rng(seed)
    az = 2.0 * np.pi * (np.arange(w) + 0.25) / w
    alt = np.deg2rad(np.linspace(22.0, -22.0, h)) if h > 1 else np.array([0.05])
    d = np.stack([np.cos(alt)[:, None] * np.cos(az)[None, :], np.cos(alt)[:, None] * np.sin(az)[None, :],
                  np.sin(alt)[:, None] * np.ones(w)[None, :]], axis=-1)
    # the plane n . p = 4 seen from inside a room: |n . d| keeps every beam on a wall 4 m / cos away at most 40 m
    n = np.array([0.8, 0.5, 0.33])
    n /= np.linalg.norm(n)
    t_plane = np.minimum(4.0 / np.maximum(np.abs(d @ n), 0.1), 40.0)
    c, r = np.array([2.0, 0.6, 0.1]), 0.9
    b = d @ c
    disc = b * b - (c @ c - r * r)
    t_sphere = np.where(disc > 0, b - np.sqrt(np.maximum(disc, 0)), np.inf)
    hit = (t_sphere > 0) & (t_sphere < t_plane)
    r1 = np.round(np.where(hit, t_sphere, t_plane) * 1000.0).astype(np.uint32)
    r2 = np.where(hit, np.round(t_plane * 1000.0), 0).astype(np.uint32)
    if w >= 8:                                   # the pole: one column, 600 mm in front of the wall
        cp = (3 * w) // 4
        r2[:, cp] = np.where(hit[:, cp], r2[:, cp], r1[:, cp])
        r1[:, cp] = np.where(hit[:, cp], r1[:, cp], r1[:, cp] - 600)
    r1[rng.random((h, w)) < 0.1] = 0
    r2[rng.random((h, w)) < 0.1] = 0
    if w >= 4:
        r1[:, w // 2] = 0
        r1[:, 1] = 0
    if h >= 4:
        r1[h // 3, :] = 0
        r2[h - 2, :] = 0
    if zero:
        r1[:], r2[:] = 0, 0
    xyz = (r1.astype(np.float64) * 0.001)[..., None] * d
    xyz2 = (r2.astype(np.float64) * 0.001)[..., None] * d
    if h >= 16 and w >= 16 and not zero:
        u, v = h // 2, w // 8                    # the tie: up (0, 0, 5) and down (3, 0, -4) from the centre, both 25 m^2 away
        r1[u - 1:u + 2, v - 1:v + 2] = 0
        r2[u - 1:u + 2, v - 1:v + 2] = 0
        xyz[u - 1:u + 2, v - 1:v + 2] = 0
        for (du, dv, p) in ((0, 0, (20.0, 0.0, 0.0)), (-1, 0, (20.0, 0.0, 5.0)), (1, 0, (23.0, 0.0, -4.0)), (0, 1, (20.0, 2.0, 0.0))):
            r1[u + du, v + dv] = 20000
            xyz[u + du, v + dv] = p
        for (u, v) in ((h // 4, w // 3), (h - 3, 5)):   # range without a beam
            r1[u, v] = 1000
            xyz[u, v] = 0.0
    out = (xyz.reshape(h * w, 3), r1, xyz2.reshape(h * w, 3), r2)
    for a in out:
        a.setflags(write=False)
    return out


def origins_for(w, mode, seed=11):
    """-> (origins (w,3) the model uses, origins array or None, poses (w,16) or None, sensor_to_body (16,) or None)"""
    rng = np.random.default_rng(seed)
    if mode == "null":
        return np.zeros((w, 3)), None, None, None
    if mode == "explicit":
        o = rng.normal(scale=0.05, size=(w, 3))
        return o, o, None, None
    poses = np.tile(np.eye(4), (w, 1, 1))
    poses[:, :3, :3] += rng.normal(scale=0.01, size=(w, 3, 3))
    poses[:, :3, 3] = rng.normal(scale=0.05, size=(w, 3))
    s2b = np.eye(4)
    s2b[:3, :] += rng.normal(scale=0.02, size=(3, 4))
    poses, s2b = np.ascontiguousarray(poses.reshape(w, 16)), np.ascontiguousarray(s2b.reshape(16))
    return M.sensor_origins(poses, s2b), None, poses, s2b


@functools.lru_cache(maxsize=None)
def model(h, w, dual, f32, psr, mode, zero=False, classify=False):
    xyz, r1, xyz2, r2 = scene(h, w, zero=zero)
    if f32:
        xyz, xyz2 = xyz.astype(np.float32).astype(np.float64), xyz2.astype(np.float32).astype(np.float64)
    org = origins_for(w, mode)[0]
    if dual:
        return M.normals(xyz, r1, xyz2, r2, sensor_origins_xyz=org, pixel_search_range=psr, classify=classify)
    res = M.normals(xyz, r1, sensor_origins_xyz=org, pixel_search_range=psr, classify=classify)
    return res if classify else (res,)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float64).reshape(-1, 3), np.ascontiguousarray(want, np.float64).reshape(-1, 3)
    bad = np.nonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))[0]
    print("%s: %d of %d normals differ%s" % (what, len(bad), len(want), "" if not len(bad) else
                                              "; first at %d: got %r want %r" % (bad[0], got[bad[0]], want[bad[0]])))
    assert len(bad) == 0, what


def stagger(a, shifts):
    """the staggered form of a destaggered (h, w, ...) array: pixel (u, v) goes to column (v - shift[u]) mod w"""
    return np.stack([np.roll(a[u], -int(shifts[u]), axis=0) for u in range(a.shape[0])])


def run_device(gpu, xyz, r1, xyz2=None, r2=None, *, f32=False, psr=1, shifts=None, staggered_out=False, origins=None, poses=None,
               s2b=None, min_angle=M.DEFAULT_MIN_ANGLE_INCIDENCE_RAD, target=M.DEFAULT_TARGET_DISTANCE_METER, host=None):
    """one frame through ouster_hip_normals (device memory between guard bytes), or through ouster_hip_normals_host with
    host = "foreign" (numpy memory) / "pool" (the library's pool).  -> list of (h*w, 3) per return"""
    capi, ctx, torch = gpu
    h, w = r1.shape
    dual = xyz2 is not None
    ft = np.float32 if f32 else np.float64
    ins = [np.ascontiguousarray(xyz, ft).reshape(h * w, 3), np.ascontiguousarray(r1, np.uint32)]
    if dual:
        ins += [np.ascontiguousarray(xyz2, ft).reshape(h * w, 3), np.ascontiguousarray(r2, np.uint32)]
    extra = [None if a is None else np.ascontiguousarray(a, np.float64) for a in (origins, poses)]
    d = capi.NormalsDesc()
    keep, pool = [], []
    nbytes = h * w * 24

    def place(a):
        if host == "foreign":
            keep.append(a)
            return a.ctypes.data
        if host == "pool":
            p = ctx.L.ouster_hip_host_alloc(max(a.nbytes, 1), 0)
            pool.append((p, max(a.nbytes, 1)))
            C.memmove(p, a.ctypes.data, a.nbytes)
            return p
        t = torch.from_numpy(a).cuda()
        keep.append(t)
        return t.data_ptr()

    ptrs = [place(a) for a in ins]
    d.xyz, d.range = ptrs[0], ptrs[1]
    if dual:
        d.xyz2, d.range2 = ptrs[2], ptrs[3]
        d.xyz2_rows, d.range2_h, d.range2_w = h * w, h, w
    if extra[0] is not None:
        d.sensor_origins, d.n_origins = place(extra[0]), len(extra[0])
    if extra[1] is not None:
        d.poses = place(extra[1])
        s2b = np.ascontiguousarray(s2b, np.float64)
        d.sensor_to_body = s2b.ctypes.data
    outs = []
    for _ in range(2 if dual else 1):
        if host == "foreign":
            outs.append(np.full(GUARD + nbytes + GUARD, 0xCD, np.uint8))
            outs_ptr = outs[-1].ctypes.data
        elif host == "pool":
            p = ctx.L.ouster_hip_host_alloc(GUARD + nbytes + GUARD, 0)
            pool.append((p, GUARD + nbytes + GUARD))
            C.memset(p, 0xCD, GUARD + nbytes + GUARD)
            outs.append(p)
            outs_ptr = p
        else:
            outs.append(torch.full((GUARD + nbytes + GUARD,), 0xCD, dtype=torch.uint8, device="cuda"))
            outs_ptr = outs[-1].data_ptr()
        if len(outs) == 1:
            d.normals = outs_ptr + GUARD
        else:
            d.normals2 = outs_ptr + GUARD
    if shifts is not None:
        sh = np.ascontiguousarray(shifts, np.int32)
        d.pixel_shift_by_row = sh.ctypes.data
    d.xyz_rows, d.n_frames, d.h, d.w = h * w, 1, h, w
    d.pixel_search_range, d.xyz_dtype, d.staggered_output = psr, capi.F32 if f32 else capi.F64, int(staggered_out)
    d.min_angle_of_incidence_rad, d.target_distance_m = min_angle, target
    capi.check((ctx.L.ouster_hip_normals_host if host else ctx.L.ouster_hip_normals)(ctx.h, C.byref(d)))
    ctx.sync()
    res = []
    for o in outs:
        if host == "foreign":
            raw = o
        elif host == "pool":
            raw = np.ctypeslib.as_array((C.c_uint8 * (GUARD + nbytes + GUARD)).from_address(o)).copy()
        else:
            raw = o.cpu().numpy()
        assert np.all(raw[:GUARD] == 0xCD) and np.all(raw[GUARD + nbytes:] == 0xCD), "guard bytes"
        res.append(raw[GUARD:GUARD + nbytes].view(np.float64).reshape(h * w, 3).copy())
    for p, n in pool:
        ctx.L.ouster_hip_host_free(p, n)
    return res


# (7, 5, 9): h > w and a range past both, the other branch of the cut-off at max(h, w)
SHAPES = [(1, 1, 1), (1, 8, 1), (2, 2, 1), (5, 7, 1), (5, 7, 3), (5, 7, 9), (7, 5, 9), (TILE_H + 1, TILE_W + 1, 3), (64, 256, 1)]


@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("h,w,psr", SHAPES)
def test_scene_equals_the_model(gpu, h, w, psr, dual):
    xyz, r1, xyz2, r2 = scene(h, w)
    want = model(h, w, dual, False, psr, "null")
    got = run_device(gpu, xyz, r1, *((xyz2, r2) if dual else ()), psr=psr)
    for i, (g, m) in enumerate(zip(got, want)):
        same_bits(g, m, "%dx%d psr %d %s return %d" % (h, w, psr, "dual" if dual else "single", i))


def test_the_scene_takes_every_branch():
    """a condition on the model's output, not a measurement: the (64, 256) scene reaches every case of the reference's loop"""
    _, _, c1, c2 = model(64, 256, True, False, 1, "null", classify=True)
    seen = set(np.unique(c1)) | set(np.unique(c2))
    for case in (M.ZERO_RANGE, M.CASE_A, M.CASE_B_VERTICAL, M.CASE_B_HORIZONTAL, M.CASE_C, M.CASE_C_FLIP, M.FELL_THROUGH):
        assert case in seen, case
    xyz, r1, _, _ = scene(64, 256)
    u, v = 32, 32                                                 # the tie: the upper neighbour is visited first and kept
    assert c1[u * 256 + v] in (M.CASE_C, M.CASE_C_FLIP)
    n = model(64, 256, True, False, 1, "null")[0][u * 256 + v]
    up, right = xyz[(u - 1) * 256 + v] - xyz[u * 256 + v], xyz[u * 256 + v + 1] - xyz[u * 256 + v]
    assert np.array_equal(up, [0.0, 0.0, 5.0]) and abs(abs(n @ np.cross(up, right)) / np.linalg.norm(np.cross(up, right)) - 1.0) < 1e-12


def test_reference_tiny_cases(gpu):
    x = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0], [1.0, 1.0, 0.0]]])
    r = np.array([[0, 1], [1, 1]], np.uint32)
    x2 = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]])
    rr2 = np.array([[0, 1], [0, 0]], np.uint32)
    org = np.zeros((2, 3))
    for a, b in ((x, r), (x2, rr2)):
        want = M.normals(a, b, sensor_origins_xyz=org, pixel_search_range=1, min_angle_of_incidence_rad=0.1, target_distance_m=100)
        got = run_device(gpu, a, b, origins=org, min_angle=0.1, target=100.0)
        same_bits(got[0], want, "2x2 single")
        want = M.normals(a, b, a, b, sensor_origins_xyz=org, pixel_search_range=1, min_angle_of_incidence_rad=0.1, target_distance_m=100)
        got = run_device(gpu, a, b, a, b, origins=org, min_angle=0.1, target=100.0)
        same_bits(got[0], want[0], "2x2 dual first")
        same_bits(got[1], want[1], "2x2 dual second")


@pytest.mark.parametrize("h,w", [(5, 7), (64, 256)])
def test_all_zero_image(gpu, h, w):
    xyz, r1, xyz2, r2 = scene(h, w, zero=True)
    got = run_device(gpu, xyz, r1, xyz2, r2)
    for g in got:
        assert not g.view(np.uint64).any()
    same_bits(got[0], model(h, w, True, False, 1, "null", zero=True)[0], "all zero")


@pytest.mark.parametrize("h,w,psr", [(5, 7, 3), (TILE_H + 1, TILE_W + 1, 3), (64, 256, 1)])
def test_float_clouds(gpu, h, w, psr):
    xyz, r1, xyz2, r2 = scene(h, w)
    want = model(h, w, True, True, psr, "null")
    got = run_device(gpu, xyz, r1, xyz2, r2, f32=True, psr=psr)
    same_bits(got[0], want[0], "f32 first")
    same_bits(got[1], want[1], "f32 second")


@pytest.mark.parametrize("h,w,psr", [(1, 8, 1), (5, 7, 3), (5, 7, 9), (TILE_H + 1, TILE_W + 1, 3), (64, 256, 1)])
def test_staggered_input_and_output(gpu, h, w, psr):
    """shifts of both signs, larger than w on the small widths; the staggered output is the destaggered one moved with the points"""
    xyz, r1, xyz2, r2 = scene(h, w)
    shifts = np.random.default_rng(h * w).integers(-2 * w - 3, 2 * w + 3, h).astype(np.int32)
    if h > 1:
        shifts[0], shifts[1] = -(w + 2), w + 1
    sx, sr = stagger(xyz.reshape(h, w, 3), shifts), stagger(r1, shifts)
    sx2, sr2 = stagger(xyz2.reshape(h, w, 3), shifts), stagger(r2, shifts)
    want = model(h, w, True, False, psr, "null")
    got = run_device(gpu, sx, sr, sx2, sr2, psr=psr, shifts=shifts)
    same_bits(got[0], want[0], "staggered in, first")
    same_bits(got[1], want[1], "staggered in, second")
    got = run_device(gpu, sx, sr, sx2, sr2, psr=psr, shifts=shifts, staggered_out=True)
    for i in range(2):
        same_bits(got[i], stagger(want[i].reshape(h, w, 3), shifts), "staggered out, return %d" % i)
    single = run_device(gpu, sx, sr, psr=psr, shifts=shifts, staggered_out=True)
    same_bits(single[0], stagger(model(h, w, False, False, psr, "null")[0].reshape(h, w, 3), shifts), "staggered out, single")


@pytest.mark.parametrize("mode", ["explicit", "poses"])
@pytest.mark.parametrize("h,w,psr", [(5, 7, 3), (64, 256, 1)])
def test_origins(gpu, h, w, psr, mode):
    xyz, r1, xyz2, r2 = scene(h, w)
    _, org, poses, s2b = origins_for(w, mode)
    want = model(h, w, True, False, psr, mode)
    got = run_device(gpu, xyz, r1, xyz2, r2, psr=psr, origins=org, poses=poses, s2b=s2b)
    same_bits(got[0], want[0], mode + " first")
    same_bits(got[1], want[1], mode + " second")


@pytest.mark.parametrize("host", ["foreign", "pool"])
def test_host_forms(gpu, host):
    h, w, psr = 64, 256, 1
    xyz, r1, xyz2, r2 = scene(h, w)
    want = model(h, w, True, False, psr, "null")
    got = run_device(gpu, xyz, r1, xyz2, r2, psr=psr, host=host)
    same_bits(got[0], want[0], host + " first")
    same_bits(got[1], want[1], host + " second")
    _, org, poses, s2b = origins_for(7, "poses")
    xyz, r1, xyz2, r2 = scene(5, 7)
    got = run_device(gpu, xyz, r1, psr=3, poses=poses, s2b=s2b, host=host)
    same_bits(got[0], M.normals(xyz, r1, sensor_origins_xyz=origins_for(7, "poses")[0], pixel_search_range=3), host + " poses")


def frames_for_batch(h, w):
    """five frames of different content -> xyz (n, h*w, 3), r1 (n, h, w), xyz2, r2:
    0, 3: two scenes;  1: all zero (the fallback subtent, between frames that have a pair);  2: a first return with range in one
    row only (no column has two rows: no pair) over a second return that has pairs;  4: the first return's winning column holds
    two rows on the same beam (dot 1, subtent 0: the dual form's override is not taken and the second return's own pair serves)"""
    fr = []
    for seed in (5, 6, 7, 8, 9):
        fr.append([np.array(a) for a in scene(h, w, seed=seed)])
    for a in fr[1]:
        a[...] = 0
    keep = fr[2][1][h // 2].copy()
    fr[2][1][...] = 0
    fr[2][1][h // 2] = keep
    x, r = fr[4][0].reshape(h, w, 3), fr[4][1]
    r[:, w // 2] = 0
    r[0, w // 2] = r[h - 1, w // 2] = 2000
    x[0, w // 2] = x[h - 1, w // 2] = (2.0, 0.0, 0.0)
    return [np.stack([f[i] for f in fr]) for i in range(4)]


def several_frames():
    """-> h, w, psr, n, clouds and ranges of frames_for_batch, per-frame poses (n, w, 16), sensor_to_body (16,); checks on the model
    that the frames are what frames_for_batch says"""
    h, w, psr, n = 6, TILE_W + 6, 2, 5
    xyz, r1, xyz2, r2 = frames_for_batch(h, w)
    rng = np.random.default_rng(21)
    poses = np.tile(np.eye(4), (n, w, 1, 1))
    poses[..., :3, 3] = rng.normal(scale=0.05, size=(n, w, 3))
    poses[..., :3, :3] += rng.normal(scale=0.01, size=(n, w, 3, 3))
    poses = np.ascontiguousarray(poses.reshape(n, w, 16))
    s2b = np.eye(4)
    s2b[:3, :] += rng.normal(scale=0.02, size=(3, 4))
    s2b = np.ascontiguousarray(s2b.reshape(16))
    org = [M.sensor_origins(poses[f], s2b) for f in range(n)]
    o = org[4][w // 2]                               # frame 4: both points 2 m along x from their column's origin
    for u in (0, h - 1):
        xyz[4].reshape(h, w, 3)[u, w // 2] = (o[0] + 2.0, o[1], o[2])
    pairs = [M.subtent_pair(xyz[f].tolist(), r1[f].reshape(-1).tolist(), org[f].tolist(), h, w) for f in range(n)]
    assert pairs[0] is not None and pairs[1] is None and pairs[2] is None and pairs[3] is not None
    assert pairs[4] is not None and M.vertical_subtent(h, pairs[4]) == 0.0
    for f in (2, 4):
        assert M.subtent_pair(xyz2[f].tolist(), r2[f].reshape(-1).tolist(), org[f].tolist(), h, w) is not None
    return h, w, psr, n, xyz, r1, xyz2, r2, poses, s2b


def test_several_frames_in_one_call(gpu):
    """n_frames > 1 through ouster_hip_normals: per-frame constants, pairs, poses and plane offsets; each frame equals the model
    run on that frame alone"""
    capi, ctx, torch = gpu
    h, w, psr, n, xyz, r1, xyz2, r2, poses, s2b = several_frames()
    nbytes = n * h * w * 24
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (xyz, r1, xyz2, r2, poses)]
    outs = [torch.full((GUARD + nbytes + GUARD,), 0xCD, dtype=torch.uint8, device="cuda") for _ in range(2)]
    d = capi.NormalsDesc()
    d.xyz, d.range, d.xyz2, d.range2, d.poses = (x.data_ptr() for x in t)
    d.sensor_to_body = s2b.ctypes.data
    d.normals, d.normals2 = outs[0].data_ptr() + GUARD, outs[1].data_ptr() + GUARD
    d.xyz_rows = d.xyz2_rows = h * w
    d.n_frames, d.h, d.w, d.range2_h, d.range2_w = n, h, w, h, w
    d.pixel_search_range, d.xyz_dtype = psr, capi.F64
    d.min_angle_of_incidence_rad, d.target_distance_m = M.DEFAULT_MIN_ANGLE_INCIDENCE_RAD, M.DEFAULT_TARGET_DISTANCE_METER
    capi.check(ctx.L.ouster_hip_normals(ctx.h, C.byref(d)))
    ctx.sync()
    got = []
    for o in outs:
        raw = o.cpu().numpy()
        assert np.all(raw[:GUARD] == 0xCD) and np.all(raw[GUARD + nbytes:] == 0xCD), "guard bytes"
        got.append(raw[GUARD:GUARD + nbytes].view(np.float64).reshape(n, h * w, 3))
    for f in range(n):
        want = M.normals(xyz[f], r1[f], xyz2[f], r2[f], sensor_origins_xyz=M.sensor_origins(poses[f], s2b), pixel_search_range=psr)
        same_bits(got[0][f], want[0], "frame %d first" % f)
        same_bits(got[1][f], want[1], "frame %d second" % f)
    assert not got[0][1].view(np.uint64).any() and got[0][0].any() and got[1][2].any() and got[1][4].any()


def test_python_face(gpu):
    import ouster.sdk.algorithm as algorithm
    h, w = 64, 256
    xyz, r1, xyz2, r2 = scene(h, w)
    org = np.zeros((w, 3))
    single = algorithm.normals(xyz.reshape(h, w, 3), r1, sensor_origins_xyz=org)
    assert single.shape == (h, w, 3) and single.dtype == np.float64
    same_bits(single, model(h, w, False, False, 1, "null")[0], "python single")
    first, second = algorithm.normals(xyz, r1, xyz2, r2, org, 1)
    assert first.shape == second.shape == (h, w, 3)
    want = model(h, w, True, False, 1, "null")
    same_bits(first, want[0], "python first")
    same_bits(second, want[1], "python second")
    xyz, r1, _, _ = scene(5, 7)
    got = algorithm.normals(xyz, r1, np.zeros((7, 3)), pixel_search_range=9)
    same_bits(got, model(5, 7, False, False, 9, "null")[0], "python psr 9")


def test_car_scan_at_full_size(gpu):
    """single_scan_016.osf, 128 x 1024, dual: equal to the model on every pixel"""
    import test_normals_model as T
    h, w, _, d = T.osf_inputs(T.CAR)
    (xyz, rng), (xyz2, rng2) = d["RANGE"], d["RANGE2"]
    _, first, second = T.car_model()
    got = run_device(gpu, xyz, rng, xyz2, rng2, origins=np.zeros((w, 3)))
    same_bits(got[0], first, "car first")
    same_bits(got[1], second, "car second")
