"""Inputs and call helpers the IcpTarget tests share (test_icp_target_api_cpu.py, test_icp_target_lanes_cpu.py,
test_gpu_icp_target.py), all over tests/icp_cases.py: the two step groups, the seven sources of the align case and the model's run of
each, and the ouster_hip_icp_target_* calls through ctypes."""
import ctypes as C
import functools

import numpy as np

import icp_cases as K
import icp_model as M

CHUNK = 1024


# ---- step: two groups, each one call.  (target case, [(n, variant)], the pose every source starts from) -----------------------------
def step_groups(plane):
    """-> [(target points, target normals, [source arrays dict], [pose], [model pass])]; group A: tie_target as f64 dense and the
    variant-0 sources from the identity; group B: the f32 strided target of variant 1 and its sources from POSE_B"""
    groups = []
    for sizes, variant in (((20, 65, 1041), 0), ((257, 1041), 1)):
        first, _ = K.tie_case(sizes[0] if variant == 0 else 257, plane, variant)
        cases = [K.tie_case(n, plane, variant) for n in sizes]
        for a, _ in cases:      # every case of a variant shares one target
            assert a["tgt"].tobytes() == first["tgt"].tobytes()
        groups.append(dict(tgt=first["tgt"], tgt_n=first["tgt_n"], sources=[a for a, _ in cases], poses=[p for _, p in cases],
                           models=[K.tie_model(n, plane, variant) for n in sizes], sizes=sizes, variant=variant))
    return groups


@functools.lru_cache(maxsize=None)
def tie_model_at(n, plane, variant, angle):
    """K.tie_model with the gate of the call.  A call has one max_normal_angle_deg for all its sources, while tie_case(20) is built
    for a wide-open gate (K.tie_gate): on the plane route every group is therefore run once per gate of its sources, and a source
    whose own gate is another one is compared with the model at the call's gate."""
    if not plane or angle == K.tie_gate(n):
        return K.tie_model(n, plane, variant)
    a, pose = K.tie_case(n, plane, variant)
    src, tgt, src_n, tgt_n = M.widen(a["src"]), M.widen(a["tgt"]), M.widen(a["src_n"]), M.widen(a["tgt_n"])
    return M.step(M.PLANE, pose, src, tgt, src_n, tgt_n, M.build_grid(tgt, tgt_n, K.CELL), K.CELL, angle)


def step_gates(group, plane):
    """the gates a group is run with: those of its sources' tie cases"""
    return sorted({K.tie_gate(n) for n in group["sizes"]}) if plane else [20.0]


STEP_COUNTS ={False: [20, 60, 1036, 253, 1037], True: [20, 55, 965, 235, 966]}     # the model's, in the order of the groups

# ---- align: seven sources in one call -----------------------------------------------------------------------------------------
ALIGN_FIRST = (0, 37, 74, 111, 148, 500, 900)
ALIGN_SIZE = (600, 1024, 1025, 1233, 2049, 19, 20)
ALIGN_MOVES = ((0, 0, 0, 0, 0, 0), K.MOVE, (0.02, 0.01, -0.03, 0.10, -0.08, 0.05), (0, 0, 0.05, 0.15, 0.1, -0.1), (0, 0, 0, 5, 5, 5),
               (0, 0, 0, 0, 0, 0), (0, 0, 0, 0.01, 0, 0))
ALIGN_PASSES = {M.POINT: [2, 3, 4, 8, 7, 0, 2], M.PLANE: [2, 3, 3, 4, 1, 0, 2]}


@functools.lru_cache(maxsize=None)
def align_sources():
    """-> (target points, target normals, [(source points, source normals)]): rows [first, first + size) of the realistic pair's
    source cloud, each moved by the inverse of pose_exp of its move, normals rotated likewise"""
    import pose_model as P
    src, src_n, tgt, tgt_n, _ = K.realistic_pair(1)
    out = []
    for first, size, move in zip(ALIGN_FIRST, ALIGN_SIZE, ALIGN_MOVES):
        m = np.array(P.pose_exp([float(v) for v in move]), dtype=np.float64)
        rows, normals = src[first:first + size], src_n[first:first + size]
        p = np.ascontiguousarray((rows - m[:3, 3]) @ m[:3, :3])          # R^T (x - t)
        n = np.ascontiguousarray(normals @ m[:3, :3])
        p.setflags(write=False), n.setflags(write=False)
        out.append((p, n))
    return tgt, tgt_n, out


@functools.lru_cache(maxsize=None)
def align_model(method):
    """the model's run of every source alone -> [(pose, iterations, count, solved)]"""
    tgt, tgt_n, sources = align_sources()
    out = []
    for p, n in sources:
        normals = (n, tgt_n) if method == M.PLANE else (None, None)
        out.append(M.align(method, p, tgt, normals[0], normals[1], None, K.REAL_DIST, 20.0))
    return out


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def target_desc(capi, cloud, normals=None, max_corr_dist=0.25, ptr=None, **over):
    """-> (IcpTargetDesc, what must stay alive)"""
    ptr = ptr or (lambda a: a.ctypes.data)
    d = capi.IcpTargetDesc()
    keep = []

    def put(a):
        if a is None:
            return None, 0, 0
        a = np.asarray(a)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        a = np.ascontiguousarray(a)
        keep.append(a)
        return (ptr(a) if len(a) else ptr(np.zeros((1, 3), a.dtype))), len(a), a.shape[1]

    d.points, d.n, d.stride = put(cloud)
    d.normals, d.n_normals, d.normal_stride = put(normals)
    d.dtype = capi.F32 if keep and keep[0].dtype == np.float32 else capi.F64
    d.max_corr_dist = max_corr_dist
    for k, v in over.items():
        setattr(d, k, v)
    return d, keep


def create(capi, ctx, cloud, normals=None, max_corr_dist=0.25, ptr=None, host=True, **over):
    """-> (rc, handle as c_void_p; .value is None after a failure)"""
    L = capi.load_hip()
    d, keep = target_desc(capi, cloud, normals, max_corr_dist, ptr, **over)
    h = C.c_void_p(0xdead)      # must be overwritten, with NULL on failure
    fn = L.ouster_hip_icp_target_create_host if host else L.ouster_hip_icp_target_create
    rc = fn(ctx, C.byref(d), C.byref(h))
    return rc, h


def make_sources(capi, clouds, normals=None, guesses=None, ptr=None, rows=None):
    """-> (IcpSource array, what must stay alive, dtype tag); outputs filled with guard values like icp_cases.make_desc"""
    ptr = ptr or (lambda a: a.ctypes.data)
    n = len(clouds)
    s = (capi.IcpSource * max(n, 1))()
    keep = []
    dtype = capi.F64

    def put(a):
        a = np.asarray(a)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        a = np.ascontiguousarray(a)
        keep.append(a)
        return (ptr(a) if len(a) else ptr(np.zeros((1, 3), a.dtype))), len(a), a.shape[1], a.dtype

    for k in range(n):
        s[k].points, s[k].n, s[k].stride, dt = put(clouds[k])
        dtype = capi.F32 if dt == np.float32 else capi.F64
        if normals is not None and normals[k] is not None:
            s[k].normals, s[k].n_normals, s[k].normal_stride, _ = put(normals[k])
        g = np.eye(4) if guesses is None or guesses[k] is None else np.asarray(guesses[k], dtype=np.float64).reshape(4, 4)
        s[k].initial_guess[:] = g.reshape(-1).tolist()
        s[k].pose[:] = [K.GUARD_R] * 16
        s[k].iterations, s[k].solved, s[k].correspondences = 777, 777, 777
    for (k, name), v in (rows or {}).items():
        setattr(s[k], name, v)
    return s, keep, dtype


def sources_untouched(s, n):
    return all(list(s[k].pose) == [K.GUARD_R] * 16 and (s[k].iterations, s[k].solved, s[k].correspondences) == (777, 777, 777)
               for k in range(n))


def source_result(s):
    return np.array(list(s.pose)).reshape(4, 4), s.iterations, s.correspondences, s.solved


def chunk_table(rows):
    """the chunk table in a few lines of Python: every source cut into runs of CHUNK rows from its own row 0"""
    return [(k, first, min(CHUNK, n - first)) for k, n in enumerate(rows) for first in range(0, n, CHUNK)]
