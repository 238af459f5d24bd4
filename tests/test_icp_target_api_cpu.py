"""The public surface of IcpTarget (ouster_hip_icp_target_*, algorithm::IcpTarget, ouster_sdk_amd.core.IcpTarget), checked without a
GPU: symbols and struct layout; every refusal through the C ABI with the outputs untouched, through Python and through C++
(tests/cpp/icp_target_snippet.cpp); the chunk-table builder against a few lines of Python; the small-target route, which needs no
GPU; the loud failure of the GPU entry points without one; the plain C++ helpers under ASan / UBSan in a program of their own
(tests/cpp/icp_target_ref_main.cpp); and the preconditions of the GPU file's align case, from tests/icp_model.py alone."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cpp_tools
import icp_cases as K
import icp_model as M
import icp_target_cases as T
from conftest import ROOT, has_gpu
from ouster_sdk_amd import _capi as capi

sys.path.insert(0, os.path.join(ROOT, "ouster_sdk_amd", "compat"))

SYMBOLS = ["ouster_hip_icp_target_create", "ouster_hip_icp_target_create_host", "ouster_hip_icp_target_info_read",
           "ouster_hip_icp_target_align", "ouster_hip_icp_target_align_host", "ouster_hip_icp_target_step"]
MSG_OTHER_CTX = "icp_target: made by another context"
MSG_ROWS = "icp: more than 2^30 rows"
OTHER_CTX = C.c_void_p(0x1000)      # compared, never followed: the refusal comes before anything reads the context


def last_error():
    return capi.load_hip().ouster_hip_last_error().decode()


def test_symbols_are_declared_and_exported():
    L = capi.load_hip()
    header = open(os.path.join(ROOT, "include", "ouster_hip.h")).read()
    for name in SYMBOLS:
        assert name in capi.ABI_SYMBOLS and hasattr(L, name) and ("int " + name + "(") in header, name
    assert "void ouster_hip_icp_target_destroy(ouster_hip_icp_target* target);" in header and hasattr(L, "ouster_hip_icp_target_destroy")
    assert "uint64_t ouster_hip_icp_chunk_table(" in header and "ouster_hip_icp_chunk_table" in capi.ABI_SYMBOLS
    assert C.sizeof(capi.IcpTargetDesc) == 2 * 8 + 4 * 8 + 2 * 4 + 8
    assert C.sizeof(capi.IcpTargetInfo) == 4 * 8 + 2 * 4 + 8
    assert C.sizeof(capi.IcpSource) == 2 * 8 + 4 * 8 + 16 * 8 + 16 * 8 + 2 * 4 + 8
    assert capi.IcpSource.pose.offset == 48 + 128 and capi.IcpTargetDesc.max_corr_dist.offset == 56
    assert L.ouster_hip_icp_chunk_rows() == T.CHUNK
    L.ouster_hip_icp_target_destroy(None)       # a no-op
    assert L.ouster_hip_icp_target_info_read(None, C.byref(capi.IcpTargetInfo())) == capi.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("rows", [[20], [1023], [1024], [1025], [2049], [20, 1023, 1024, 1025, 2049], [2049, 0, 20, 0, 1025], [], [0, 0]])
def test_chunk_table_equals_its_definition(rows):
    L = capi.load_hip()
    want = T.chunk_table(rows)
    r = (C.c_uint64 * max(len(rows), 1))(*rows)
    assert L.ouster_hip_icp_chunk_table(r, len(rows), None, 0) == len(want)         # counting only
    cap = len(want) + 2
    out = (C.c_uint32 * (3 * cap))(*([0xabcdef] * (3 * cap)))
    assert L.ouster_hip_icp_chunk_table(r, len(rows), out, cap) == len(want)
    got = [tuple(out[3 * k:3 * k + 3]) for k in range(cap)]
    assert got[:len(want)] == want and got[len(want):] == [(0xabcdef,) * 3] * 2
    # every source's runs are those of the single call: ceil(n / chunk) of them, all full but the last
    for k, n in enumerate(rows):
        mine = [c for c in want if c[0] == k]
        assert len(mine) == -(-n // T.CHUNK) and sum(c[2] for c in mine) == n and all(c[2] == T.CHUNK for c in mine[:-1])
    if len(want) > 1:                           # a table that is too small is filled as far as it goes
        small = (C.c_uint32 * (3 * len(want)))(*([7] * (3 * len(want))))
        assert L.ouster_hip_icp_chunk_table(r, len(rows), small, 1) == len(want)
        assert tuple(small[:3]) == want[0] and set(small[3:]) == {7}


def create_error_cases():
    tgt = K.published_point()[1]
    n = np.tile([0.0, 0.0, 1.0], (27, 1))
    nan, inf = float("nan"), float("inf")
    cases = [(M.MSG_DIST, dict(max_corr_dist=bad)) for bad in (0.0, -1.0, nan, inf)]
    cases += [(M.MSG_DIST, dict(normals=n[:5], max_corr_dist=0.0, dtype=99, flags=1))]            # the first in order wins
    cases += [(M.MSG_TGT_ROWS, dict(normals=n[:26])), (M.MSG_TGT_ROWS, dict(normals=n[:26], dtype=99))]
    cases += [("dtype must be F32 or F64", dict(dtype=99, flags=1)), ("flags must be 0", dict(flags=1)), ("flags must be 0", dict(normals=n, flags=0x80000000))]
    cases += [("a row stride is smaller than 3", dict(stride=2)), ("a row stride is smaller than 3", dict(normals=n, normal_stride=1))]
    cases += [("NULL pointer", dict(points=None))]
    return tgt, n, cases


def test_create_validation_comes_before_the_gpu():
    """ctx is NULL: a validation error must win over it, which shows that nothing touched the GPU; *out is NULL afterwards"""
    L = capi.load_hip()
    tgt, n, cases = create_error_cases()
    for message, kw in cases:
        over = {k: v for k, v in kw.items() if k not in ("normals", "max_corr_dist")}
        for host in (True, False):
            rc, h = T.create(capi, None, tgt, kw.get("normals"), kw.get("max_corr_dist", 0.25), host=host, **over)
            assert rc == capi.ERR_INVALID_ARGUMENT and last_error() == message and h.value is None, (message, last_error())
    for host in (True, False):
        rc, h = T.create(capi, None, tgt, host=host, n=(1 << 30) + 1)
        assert rc == capi.ERR_UNSUPPORTED and last_error() == MSG_ROWS and h.value is None
        rc, h = T.create(capi, None, tgt, normals=n, host=host, n=(1 << 30) + 1)        # the rows of the normals come first
        assert rc == capi.ERR_INVALID_ARGUMENT and last_error() == M.MSG_TGT_ROWS and h.value is None
    d, keep = T.target_desc(capi, tgt)
    h = C.c_void_p(5)
    assert L.ouster_hip_icp_target_create(None, None, C.byref(h)) == capi.ERR_INVALID_ARGUMENT and last_error() == "NULL argument" and h.value is None
    assert L.ouster_hip_icp_target_create(None, C.byref(d), None) == capi.ERR_INVALID_ARGUMENT and last_error() == "NULL argument"


@pytest.fixture(scope="module")
def small_targets():
    """targets of 19 rows, made without a context: point and plane"""
    L = capi.load_hip()
    tgt = K.published_point()[1][:19]
    n = np.tile([0.0, 0.0, 2.0], (19, 1))
    made = []
    for normals in (None, n):
        rc, h = T.create(capi, None, tgt, normals, 0.5, host=normals is None)
        assert rc == capi.OK and h.value, last_error()
        made.append(h)
    yield made
    for h in made:
        L.ouster_hip_icp_target_destroy(h)


def test_small_target_info_and_the_guess(small_targets):
    L = capi.load_hip()
    src = K.published_point()[0]
    n = np.tile([0.0, 0.0, 1.0], (27, 1))
    for h, plane in zip(small_targets, (False, True)):
        info = capi.IcpTargetInfo()
        assert L.ouster_hip_icp_target_info_read(h, C.byref(info)) == capi.OK
        assert (info.rows, info.rows_used, info.cells, info.device_bytes, info.has_normals, info.max_corr_dist) == (19, 0, 0, 0, int(plane), 0.5)
        guesses = [np.array(K.POSE_B), None, np.eye(4) * 3.0]
        clouds = [src, src[:5], np.zeros((0, 3))]
        for fn in (L.ouster_hip_icp_target_align, L.ouster_hip_icp_target_align_host):
            s, keep, dtype = T.make_sources(capi, clouds, [n, n[:5], n[:0]] if plane else None, guesses)
            assert fn(None, h, s, 3, dtype, 20.0) == capi.OK, last_error()
            for k in range(3):
                pose, it, count, solved = T.source_result(s[k])
                assert np.array_equal(pose, np.eye(4) if guesses[k] is None else guesses[k]) and (it, count, solved) == (0, 0, 0)
            # no sources: nothing to do, and nothing is read
            assert fn(None, h, None, 0, dtype, 20.0) == capi.OK
        s, keep, dtype = T.make_sources(capi, [src], [n] if plane else None)
        out = capi.IcpStepOut()
        eye = (C.c_double * 16)(*np.eye(4).reshape(-1).tolist())
        assert L.ouster_hip_icp_target_step(None, h, s, 1, dtype, 20.0, eye, C.byref(out)) == capi.ERR_INVALID_ARGUMENT
        assert last_error() == "icp_step: fewer than 20 rows"


def align_error_cases(plane):
    """(code, message, kwargs of make_sources, dtype override, angle, n_sources override)"""
    src = K.published_point()[0]
    n = np.tile([0.0, 0.0, 1.0], (27, 1))
    nan, inf = float("nan"), float("inf")
    nrm = [n, n] if plane else None
    inv, uns = capi.ERR_INVALID_ARGUMENT, capi.ERR_UNSUPPORTED
    cases = []
    if plane:
        cases += [(inv, M.MSG_ANGLE, dict(normals=nrm), None, bad) for bad in (-0.5, 180.5, nan, inf)]
        cases += [(inv, M.MSG_ANGLE, dict(normals=[n, n[:5]]), 99, nan)]                           # the first in order wins
        cases += [(inv, M.MSG_SRC_ROWS, dict(normals=[n, n[:5]]), None, 20.0), (inv, M.MSG_SRC_ROWS, dict(normals=[n[:26], None]), None, 20.0)]
        cases += [(inv, "icp_target: source 1 has no normals and the target has them", dict(normals=[n, None]), None, 20.0),
                  (inv, "icp_target: source 0 has no normals and the target has them", dict(normals=None), 99, 20.0)]
    else:
        cases += [(inv, "icp_target: source 1 has normals and the target has none", dict(normals=[None, n]), None, nan),
                  (inv, "icp_target: source 0 has normals and the target has none", dict(normals=[n[:3], n]), 99, 20.0)]
    cases += [(inv, "dtype must be F32 or F64", dict(normals=nrm, rows={(1, "stride"): 2}), 99, 20.0)]
    cases += [(inv, "a row stride is smaller than 3", dict(normals=nrm, rows={(1, "stride"): 2}), None, 20.0)]
    cases += [(inv, "NULL pointer", dict(normals=nrm, rows={(0, "points"): None}), None, 20.0)]
    big = {(1, "n"): (1 << 29) + 1, (0, "n"): 1 << 29, (1, "n_normals"): (1 << 29) + 1, (0, "n_normals"): 1 << 29}
    cases += [(uns, MSG_ROWS, dict(normals=nrm, rows=big), None, 20.0)]
    return src, cases


def test_align_and_step_validation_leaves_every_output_untouched(small_targets):
    L = capi.load_hip()
    eye2 = (C.c_double * 32)(*(np.eye(4).reshape(-1).tolist() * 2))
    for h, plane in zip(small_targets, (False, True)):
        src, cases = align_error_cases(plane)
        n = np.tile([0.0, 0.0, 1.0], (27, 1))
        for code, message, kw, dtype_over, angle in cases:
            for fn in (L.ouster_hip_icp_target_align, L.ouster_hip_icp_target_align_host):
                s, keep, dtype = T.make_sources(capi, [src, src], **kw)
                assert fn(None, h, s, 2, dtype if dtype_over is None else dtype_over, angle) == code and last_error() == message, (message, last_error())
                assert T.sources_untouched(s, 2)
            s, keep, dtype = T.make_sources(capi, [src, src], **kw)
            outs = (capi.IcpStepOut * 2)()
            nn = np.full(27 + K.GUARD, K.GUARD_NN, np.int32)
            outs[0].nn = outs[1].nn = nn.ctypes.data
            assert L.ouster_hip_icp_target_step(None, h, s, 2, dtype if dtype_over is None else dtype_over, angle, eye2, outs) == code
            assert last_error() == message and (nn == K.GUARD_NN).all() and T.sources_untouched(s, 2)
        good = dict(normals=[n, n]) if plane else {}
        s, keep, dtype = T.make_sources(capi, [src, src], **good)
        # a target made by another context (here: by none) is refused before the sources are looked at
        for fn in (L.ouster_hip_icp_target_align, L.ouster_hip_icp_target_align_host):
            assert fn(OTHER_CTX, h, s, 2, 99, float("nan")) == capi.ERR_INVALID_ARGUMENT and last_error() == MSG_OTHER_CTX and T.sources_untouched(s, 2)
            assert fn(None, None, s, 2, dtype, 20.0) == capi.ERR_INVALID_ARGUMENT and last_error() == "NULL argument"
            assert fn(None, h, None, 2, dtype, 20.0) == capi.ERR_INVALID_ARGUMENT and last_error() == "NULL argument"
        outs = (capi.IcpStepOut * 2)()
        assert L.ouster_hip_icp_target_step(OTHER_CTX, h, s, 2, dtype, 20.0, eye2, outs) == capi.ERR_INVALID_ARGUMENT and last_error() == MSG_OTHER_CTX
        assert L.ouster_hip_icp_target_step(None, h, s, 2, dtype, 20.0, None, outs) == capi.ERR_INVALID_ARGUMENT and last_error() == "NULL argument"
        assert L.ouster_hip_icp_target_step(None, h, s, 2, dtype, 20.0, eye2, None) == capi.ERR_INVALID_ARGUMENT and last_error() == "NULL argument"
        # more than 65 535 sources: the limit comes from the count alone
        many, keep, dtype = T.make_sources(capi, [src[:1]] * 65536, [n[:1]] * 65536 if plane else None)
        assert L.ouster_hip_icp_target_align(None, h, many, 65536, dtype, 20.0) == capi.ERR_UNSUPPORTED
        assert last_error() == "icp_target: more than 65535 sources" and T.sources_untouched(many, 65536)
        assert L.ouster_hip_icp_target_align(None, h, many, 65535, dtype, 20.0) == capi.OK


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_gpu_entry_points_without_a_gpu_fail_loudly():
    tgt = K.published_point()[1]
    n = np.tile([0.0, 0.0, 1.0], (27, 1))
    for host in (True, False):
        for normals in (None, n):
            rc, h = T.create(capi, None, tgt, normals, 0.5, host=host)
            assert rc == capi.ERR_INVALID_ARGUMENT and last_error() == "ctx is NULL" and h.value is None
    from ouster_sdk_amd import core as amd
    with pytest.raises(RuntimeError):
        amd.IcpTarget(tgt, max_corr_dist=0.5)
    with pytest.raises(RuntimeError):
        amd.IcpTarget(tgt, n, 0.5)


def test_python_face_names_defaults_and_errors():
    import ouster.sdk.algorithm as algorithm
    from ouster_sdk_amd import core as amd
    assert algorithm.IcpTarget is amd.IcpTarget
    tgt, n, cases = create_error_cases()
    for message in (M.MSG_DIST, M.MSG_TGT_ROWS):
        for _, kw in [c for c in cases if c[0] == message and "dtype" not in c[1] and "flags" not in c[1]]:
            with pytest.raises(ValueError) as e:
                amd.IcpTarget(tgt, kw.get("normals"), kw.get("max_corr_dist", 0.25))
            assert str(e.value) == message
    with pytest.raises(ValueError, match="target_points must be Nx3"):
        amd.IcpTarget(np.zeros((30, 4)))
    with pytest.raises(ValueError, match="target_normals must be Nx3"):
        amd.IcpTarget(tgt, np.zeros((27, 2)))
    # small targets need no GPU: keywords, defaults, the method fixed by the constructor, every refusal of align
    src = K.published_point()[0]
    guess = np.array(K.POSE_B)
    point = amd.IcpTarget(target_points=tgt[:19])
    plane = amd.IcpTarget(target_points=tgt[:19], target_normals=n[:19], max_corr_dist=0.5)
    assert (point.size, point.has_normals, point.device_bytes, point.max_corr_dist) == (19, False, 0, 0.25)
    assert (plane.size, plane.has_normals, plane.max_corr_dist) == (19, True, 0.5)
    got = point.align(src, initial_guess=guess)
    assert got.shape == (4, 4) and got.dtype == np.float64 and np.array_equal(got, guess)
    got = plane.align_many(sources=[src, src[:3]], normals=[n, n[:3]], initial_guesses=[guess, np.eye(4)], max_normal_angle_deg=30.0)
    assert got.shape == (2, 4, 4) and np.array_equal(got[0], guess) and np.array_equal(got[1], np.eye(4))
    assert point.align_many([]).shape == (0, 4, 4) and np.array_equal(point.align_many([src, src])[1], np.eye(4))
    for bad in (-0.5, 180.5, float("nan")):
        with pytest.raises(ValueError) as e:
            plane.align(src, n, None, bad)
        assert str(e.value) == M.MSG_ANGLE
    for target, args, message in ((plane, ([src], [n[:5]]), M.MSG_SRC_ROWS),
                                  (plane, ([src, src], None), "icp_target: source 0 has no normals and the target has them"),
                                  (point, ([src, src], [n, n]), "icp_target: source 0 has normals and the target has none")):
        with pytest.raises(ValueError) as e:
            target.align_many(*args)
        assert str(e.value) == message
    with pytest.raises(ValueError, match=r"sources\[1\] must be Nx3"):
        point.align_many([src, np.zeros((30, 2))])
    with pytest.raises(ValueError, match="initial_guess must be 4x4"):
        point.align(src, None, np.eye(3))
    with pytest.raises(ValueError, match="one 4x4 per source"):
        point.align_many([src, src], None, [guess])
    with point as t:
        assert t is point
    with pytest.raises(ValueError, match="IcpTarget: closed"):
        point.align(src)
    plane.close()
    plane.close()


def test_cpp_caller_compiles_links_and_runs():
    """tests/cpp/icp_target_snippet.cpp, built by tests/cpp/Makefile with the flags of the other C++ callers (-Werror)"""
    p = cpp_tools.run("icp_target_snippet", [], timeout=300)
    assert "validation ok" in p.stdout and "small targets ok" in p.stdout, p.stdout
    assert p.stdout.splitlines()[-1].startswith("ok" if has_gpu() else "no-gpu"), p.stdout


def test_host_helpers_under_the_sanitizers():
    """tests/cpp/icp_target_ref_main.cpp: the chunk-table builder and the argument checks in a program of their own, built with
    -fsanitize=address,undefined (tests/cpp/Makefile: _build/icp_target_ref_sanitized) and run directly"""
    exe = cpp_tools.build("icp_target_ref_sanitized")[0]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("icp_target_ref_main: ok"), p.stdout + p.stderr


def test_the_align_case_of_the_gpu_file_does_what_it_was_built_for():
    """from the model alone: the seven sources of tests/test_gpu_icp_target.py take different numbers of passes, one is unsolved,
    one stops while later ones go on, one is the early return, and the sizes lie on both sides of one and of two chunks"""
    assert [len(p) for p, _ in T.align_sources()[2]] == list(T.ALIGN_SIZE)
    sizes = set(T.ALIGN_SIZE)
    assert {T.CHUNK, T.CHUNK + 1, 2 * T.CHUNK + 1} <= sizes and any(s < T.CHUNK for s in sizes) and any(T.CHUNK + 1 < s <= 2 * T.CHUNK for s in sizes)
    assert 19 in sizes and 20 in sizes
    for method in (M.POINT, M.PLANE):
        runs = T.align_model(method)
        passes = [r[1] for r in runs]
        assert passes == T.ALIGN_PASSES[method]
        assert len(set(passes)) >= 4
        assert passes[5] == 0 and not runs[5][3]                                   # the 19-row early return
        assert any(0 < passes[k] < max(passes[k + 1:]) for k in range(len(passes) - 1))    # one stops while later ones go on
        assert all(np.array_equal(r[0], np.eye(4)) for r in runs if not r[3])
    point, plane = T.align_model(M.POINT), T.align_model(M.PLANE)
    assert point[4][2] == 30 and point[4][3]                    # ends on 30 correspondences
    assert plane[4][2] == 0 and not plane[4][3] and plane[4][1] == 1       # no correspondence at all: unsolved after one pass
    assert sum(1 for r in plane if not r[3] and r[1] > 0) == 1
    for plane_flag in (False, True):
        assert [m["count"] for g in T.step_groups(plane_flag) for m in g["models"]] == T.STEP_COUNTS[plane_flag]
