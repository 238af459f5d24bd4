"""GPU: the parts of the range-gated frame dewarp (k_dwf_count / k_dwf_scan / k_dwf_frame_scan / k_dwf_emit, k_dewarp.hip and
dwf_dev.h) and of the decode's gate counts (decode_rows, kernels_common.h) that the small, single-LUT, generously sized calls
of test_gpu_parity.py and test_gpu_fastpath.py never run, against the oracle (oracle.dewarp_frame, pinned on the reference by
tests/test_oracle_ref_dewarp.py).  The batches and what they guarantee: tests/dewarp_cases.py, tests/test_dewarp_cases_cpu.py.

  A  wide frames      k_dwf_scan past one block of 2048 columns (carry, first / last valid column in a later block)
  B  long batches     k_dwf_frame_scan past one block of 256 frames (64-bit carry); luts[f % n_luts]; full f64 LUTs
  C  capacity         the EASY = false column loop: cuts inside a run, inside the second row chunk, at column / tile / frame
                      starts; every output caller-owned, larger than `capacity` and pre-filled, so a row too many shows
  D  alignment        a range plane 4 bytes off a 16-byte boundary (element-wise staging of count and emit)
  E  gate counts      the decode's per-column counts on every route, at the chunk limit, on ragged tiles, from RANGE2

Bars (test_gpu_parity.py::test_dewarp_frames_matches_oracle, same kind of input): frame_offsets and provenance bit for bit;
points <= 1e-9 (f64) and <= 1e-4 (f32) against the oracle with the LUT in the same type, <= 3e-5 for a user-supplied f32 full
LUT.  Two runs of the project's own kernels are compared on bytes."""
import ctypes as C

import numpy as np
import pytest

import dewarp_cases as D
from conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from ouster_sdk_amd import _capi as capi
    from ouster_sdk_amd.device import HotPath

from test_gpu_fastpath import _compare  # noqa: E402
from test_gpu_launch_table import GENERIC_BITS  # noqa: E402
from test_gpu_parity import _np, _oracle_frames  # noqa: E402
from test_gpu_standalone_routes import _misaligned  # noqa: E402

PROV = ("frame_idxs", "col_idxs", "timestamps_ns")
GUARD = 64            # elements every caller-owned output has beyond n * h * w
FILL = 0xA5
# form -> (LUT kind, type of the oracle's LUT, output type, float pose rows, bar)
FORMS = {"sep32": ("sep", np.float32, "f32", False, 1e-4), "rows32": ("sep", np.float32, "f32", True, 1e-4),
         "sep64": ("sep", np.float64, "f64", False, 1e-9), "full32": ("full32", np.float32, "f32", False, 3e-5),
         "full64": ("full64", np.float64, "f64", False, 1e-9)}


class _Batch:
    """A case on the device: its HotPath, its LUTs per kind (made when first asked for) and its inputs."""

    def __init__(self, O, case):
        self.O, self.c = O, case
        self.hp = HotPath("RNG15_RFL8_NIR8", case.h, case.w, 4 if case.w % 4 == 0 else 1)
        self._luts = {}
        dev = lambda a: torch.from_numpy(a.copy()).cuda()    # noqa: E731  (the case's arrays are read-only)
        self.r, self.st, self.ts, self.po = dev(case.r), dev(case.status), dev(case.ts), dev(case.poses)
        self.rows = HotPath.pose_rows(case.poses.copy())
        for gate in D.GATES:
            assert self.hp.range_gate(*gate) == (*D.raw_gate(*gate), False)

    def luts(self, kind):
        if kind not in self._luts:
            made = []
            for k, cal in enumerate(self.c.cals(self.O)):
                if kind == "sep":
                    made.append(self.hp.add_lut(cal.beam_to_lidar, cal.lut_transform(True), cal.beam_azimuth_angles,
                                                cal.beam_altitude_angles))
                else:
                    made.append(self.hp.add_lut_arrays(*self.c.lut_arrays(self.O, k, np.float32 if kind == "full32" else np.float64)))
            self._luts[kind] = made
        return self._luts[kind]

    def gate_counts(self, gate):
        return torch.from_numpy(self.c.synthetic_gate_counts(gate).view(np.int16)).cuda().view(torch.uint16)

    def call(self, form, gate, cap=None, prov=PROV, gate_counts=None, points=True, r=None, rows=None, luts=None):
        """ouster_hip_dewarp_frames_counted / _rows through the C ABI into outputs of n * h * w + GUARD elements that start as
        bytes 0xA5.  Returns (return code, outputs)."""
        c, hp = self.c, self.hp
        kind, _, tag, use_rows, _ = FORMS[form]
        tdt = torch.float32 if tag == "f32" else torch.float64
        alloc = c.n * c.h * c.w + GUARD
        cap = c.n * c.h * c.w if cap is None else cap
        assert cap < alloc

        def buf(shape, dt):
            t = torch.empty(shape, dtype=dt, device="cuda")
            t.view(torch.uint8).fill_(FILL)
            return t

        out = {"frame_offsets": buf(c.n + 1, torch.uint64)}
        if points:
            out["points"] = buf((alloc, 3), tdt)
        for k in prov:
            out[k] = buf(alloc, torch.uint64 if k == "timestamps_ns" else torch.uint32)
        luts = self.luts(kind) if luts is None else luts
        luts_arr = (C.c_void_p * len(luts))(*[x.h for x in luts])
        ptr = lambda k: out[k].data_ptr() if k in out else None    # noqa: E731
        r = self.r if r is None else r
        gc = gate_counts.data_ptr() if gate_counts is not None else None
        L = hp.ctx.L
        if use_rows:
            rows = self.rows if rows is None else rows
            rc = L.ouster_hip_dewarp_frames_rows(hp.ctx.h, luts_arr, len(luts), r.data_ptr(), self.st.data_ptr(), self.ts.data_ptr(),
                                                 rows.data_ptr(), c.n, float(gate[0]), float(gate[1]), ptr("points"),
                                                 ptr("frame_idxs"), ptr("col_idxs"), ptr("timestamps_ns"), cap,
                                                 out["frame_offsets"].data_ptr(), gc)
        else:
            rc = L.ouster_hip_dewarp_frames_counted(hp.ctx.h, luts_arr, len(luts), r.data_ptr(), self.st.data_ptr(),
                                                    self.ts.data_ptr(), self.po.data_ptr(), c.n, float(gate[0]), float(gate[1]),
                                                    capi.F32 if tag == "f32" else capi.F64, ptr("points"), ptr("frame_idxs"),
                                                    ptr("col_idxs"), ptr("timestamps_ns"), cap, out["frame_offsets"].data_ptr(), gc)
        hp.sync()
        return rc, out

    def check_oracle(self, out, form, gate, what=""):
        """the bars of the module docstring; returns the total"""
        _, ldt, _, _, tol = FORMS[form]
        want = self.c.want(self.O, gate, ldt)
        assert np.array_equal(_np(out["frame_offsets"]), want["frame_offsets"]), (what, form, gate)
        tot = int(want["frame_offsets"][-1])
        for k in PROV:
            if k in out:
                assert np.array_equal(_np(out[k])[:tot], want[k]), (what, form, gate, k)
        if tot and "points" in out:
            err = np.abs(_np(out["points"])[:tot].astype(np.float64) - want["points"].astype(np.float64)).max()
            print(f"{self.c.name} {what} {form} {gate}: {tot} points, max |dxyz| = {err:.3e} (bar {tol:g})")
            assert err <= tol, (what, form, gate, err)
        for k, t in out.items():
            if k != "frame_offsets":
                assert _untouched(t, tot), (what, form, gate, k, "rows behind the result were written")
        return tot


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _untouched(t, first):
    return bool((_bytes(t[first:]) == FILL).all())


def _same(a, b, rows=None, what=""):
    """every output of two calls, whole buffers (or their first `rows` rows), byte for byte"""
    assert set(a) == set(b)
    for k in a:
        x, y = (a[k], b[k]) if rows is None or k == "frame_offsets" else (a[k][:rows], b[k][:rows])
        assert torch.equal(_bytes(x), _bytes(y)), (what, k)


_batches = {}


def _batch(O, builder, *args):
    key = (builder.__name__,) + args
    if key not in _batches:
        _batches[key] = _Batch(O, builder(*args))
    return _batches[key]


# ----------------------------------------------------------------------------------------------------------------------
# A. wide frames
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sep32", "sep64"])
@pytest.mark.parametrize("h,w,n", D.WIDE_SHAPES)
def test_wide_frames(oracle, h, w, n, form):
    """k_dwf_scan over 1, 1 + a quad, 1 + a column, 2 and 3 blocks of 2048 columns: the carry between blocks, the first valid
    column in a later block, non-valid columns outside the span.  Each call once with k_dwf_count and once with the true
    counts split over the eight slots of gate_counts: the same bytes."""
    b = _batch(oracle, D.wide, h, w, n)
    for gate in D.GATES:
        rc, own = b.call(form, gate)
        assert rc == capi.OK
        assert b.check_oracle(own, form, gate, "k_dwf_count") > 0
        rc, fed = b.call(form, gate, gate_counts=b.gate_counts(gate))
        assert rc == capi.OK
        _same(own, fed, what=("gate_counts", gate))


# ----------------------------------------------------------------------------------------------------------------------
# B. long batches, several LUTs
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["rows32", "sep64"])
@pytest.mark.parametrize("n,empty_256", [(256, False), (257, False), (520, False), (257, True), (520, True)])
def test_long_batches(oracle, n, empty_256, form):
    """k_dwf_frame_scan over exactly one block of 256 frame totals, one frame more, and two blocks and a bit; three LUTs taken
    as luts[f % 3]."""
    b = _batch(oracle, D.long_batch, n, empty_256)
    gate = D.GATES[0]
    rc, out = b.call(form, gate)
    assert rc == capi.OK
    assert b.check_oracle(out, form, gate) > n


@pytest.mark.parametrize("n,kinds", [(7, ("sep32", "sep64")), (5, ("full32", "full64"))])
def test_several_luts(oracle, n, kinds):
    """7 frames of 9 x 100 with three separable LUTs; 5 frames with two full LUTs, both f32 and both f64 (f64 output)"""
    b = _batch(oracle, D.multi_lut, n, 3 if n == 7 else 2)
    for form in kinds:
        for gate in D.GATES:
            rc, out = b.call(form, gate)
            assert rc == capi.OK
            assert b.check_oracle(out, form, gate) > 0


def test_mixed_lut_kinds_are_refused(oracle):
    b = _batch(oracle, D.multi_lut, 5, 2)
    for mix in ([b.luts("sep")[0], b.luts("full32")[1]], [b.luts("full64")[0], b.luts("sep")[1]]):
        rc, out = b.call("sep32", D.GATES[0], luts=mix)
        assert rc == capi.ERR_UNSUPPORTED
        assert all(_untouched(t, 0) for t in out.values())


# ----------------------------------------------------------------------------------------------------------------------
# C. capacity
# ----------------------------------------------------------------------------------------------------------------------
OUTPUTS = {"all": PROV, "frame_idxs": ("frame_idxs",), "col_idxs": ("col_idxs",), "timestamps_ns": ("timestamps_ns",),
           "none": (), "counts": PROV}


@pytest.mark.parametrize("gate", D.GATES, ids=["gate1-60", "gate0-1000"])
@pytest.mark.parametrize("outputs", list(OUTPUTS))
@pytest.mark.parametrize("form", ["sep32", "rows32", "sep64", "full32"])
@pytest.mark.parametrize("h,w,n", D.CAP_SHAPES)
def test_capacity(oracle, h, w, n, form, outputs, gate):
    """`capacity` below, at and above the total, cutting inside a column's run, inside what the second row chunk writes, at a
    column's, a tile's and a frame's first point.  frame_offsets stay complete; the rows below the capacity are the bytes of
    the uncapped call; nothing from row min(capacity, total) on is written."""
    b = _batch(oracle, D.capacity, h, w, n)
    gc = b.gate_counts(gate) if outputs == "counts" else None
    prov = OUTPUTS[outputs]
    rc, full = b.call(form, gate, prov=prov, gate_counts=gc)
    assert rc == capi.OK
    tot = b.check_oracle(full, form, gate, "uncapped")
    caps = D.capacities(b.c, oracle, gate)
    assert len(caps) == (10 if h > 128 else 9)
    for label, cap in caps.items():
        rc, part = b.call(form, gate, cap=cap, prov=prov, gate_counts=gc)
        assert rc == capi.OK, label
        keep = min(cap, tot)
        _same(part, full, rows=keep, what=(label, cap))
        for k, t in part.items():
            if k != "frame_offsets":
                assert _untouched(t, keep), (label, cap, k, "written at or behind the capacity")


def test_capacity_zero_and_null_points(oracle):
    """capacity 0 with points = NULL and no provenance returns the offsets; points = NULL with room asked for is refused"""
    b = _batch(oracle, D.capacity, 64, 128, 2)
    gate = D.GATES[0]
    want = b.c.want(oracle, gate, np.float32)["frame_offsets"]
    for form in ("sep32", "rows32"):
        rc, out = b.call(form, gate, cap=0, prov=(), points=False)
        assert rc == capi.OK and set(out) == {"frame_offsets"}
        assert np.array_equal(_np(out["frame_offsets"]), want)
        rc, out = b.call(form, gate, cap=5, prov=(), points=False)
        assert rc == capi.ERR_INVALID_ARGUMENT
        assert _untouched(out["frame_offsets"], 0)


# ----------------------------------------------------------------------------------------------------------------------
# D. alignment
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,n", D.ALIGN_SHAPES)
def test_misaligned_range_plane(oracle, h, w, n):
    """w % 4 == 0 but the range tensor starts 4 bytes off a 16-byte boundary: k_dwf_count and k_dwf_emit stage element by
    element, and every output is the aligned call's"""
    b = _batch(oracle, D.alignment, h, w, n)
    off = _misaligned(b.c.r, 4)
    assert b.r.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4
    for form in ("sep32", "rows32", "sep64"):
        for gate in D.GATES:
            rc, want = b.call(form, gate)
            assert rc == capi.OK
            assert b.check_oracle(want, form, gate, "aligned") > 0
            rc, got = b.call(form, gate, r=off)
            assert rc == capi.OK
            _same(got, want, what=(form, gate))
    rows = _misaligned(_np(b.rows), 4)
    rc, out = b.call("rows32", D.GATES[0], rows=rows)
    assert rc == capi.ERR_INVALID_ARGUMENT
    assert all(_untouched(t, 0) for t in out.values())


# ----------------------------------------------------------------------------------------------------------------------
# E. the decode's gate counts
# ----------------------------------------------------------------------------------------------------------------------
DUAL, STATIC12, STATIC4 = "RNG15_RFL8_NIR8_DUAL", "RNG19_RFL8_SIG16_NIR16", "RNG15_RFL8_NIR8"
E_GATES = ((2.0, 90.0), (0.0, 1000.0))
N_E = 5
LOST, SWAPPED, ABSENT = (1, [3, 4]), (2, [10, 11]), 3


def _wide(tw, **kw):
    return dict(wide=tw, wide_min_blocks=0, stream=0, fixup_wide=128 if tw == 256 else 256, **kw)


def _narrow(t):
    return dict(tile=t, wide=0, stream=0)


def _stream(tw):
    return dict(stream=tw, stream_min_tiles=0)


# (id, profile, h, w, generic, knobs, kernel the context must report (None: any but k_decode_wide), its tile, gated field)
E_CASES = [
    ("dual32-wide256-8chunks", DUAL, 32, 1024, False, _wide(256, wide_rows=4), "k_decode_wide", (256, 4), "RANGE"),
    ("dual32-wide128-8chunks", DUAL, 32, 1024, False, _wide(128, wide_rows=4), "k_decode_wide", (128, 4), "RANGE"),
    ("dual40-wide256-10chunks", DUAL, 40, 1024, False, _wide(256, wide_rows=4), None, None, "RANGE"),
    ("dual40-wide128-10chunks", DUAL, 40, 1024, False, _wide(128, wide_rows=4), None, None, "RANGE"),
    ("static-narrow16", STATIC12, 16, 1024, False, _narrow(16), "k_decode", (16,), "RANGE"),
    ("static-narrow32", STATIC12, 16, 1024, False, _narrow(32), "k_decode", (32,), "RANGE"),
    ("static-narrow64", STATIC12, 16, 1024, False, _narrow(64), "k_decode", (64,), "RANGE"),
    ("static-stream128", STATIC12, 16, 1024, False, _stream(128), "k_decode_stream", (128,), "RANGE"),
    ("static-stream256", STATIC12, 16, 1024, False, _stream(256), "k_decode_stream", (256,), "RANGE"),
    ("generic-narrow64", STATIC4, 16, 1024, True, _narrow(64), "k_decode", (64,), "RANGE"),
    ("generic-wide128", STATIC4, 16, 1024, True, _wide(128), "k_decode_wide", (128,), "RANGE"),
    ("dual1040-wide256", DUAL, 16, 1040, False, _wide(256), "k_decode_wide", (256,), "RANGE"),
    ("dual1040-narrow64", DUAL, 16, 1040, False, _narrow(64), "k_decode", (64,), "RANGE"),
    ("dual-range2-narrow64", DUAL, 16, 1024, False, _narrow(64), "k_decode", (64,), "RANGE2"),
    ("dual-range2-wide256", DUAL, 16, 1024, False, _wide(256), "k_decode_wide", (256,), "RANGE2"),
]
_decoded = {}


def _packets(O, profile, h, w):
    """Five frames -- clean, two lost packets, two packets swapped (fix-up pass), no packets at all, clean -- and the oracle's
    decode of them: made once per (profile, h, w), never written."""
    key = (profile, h, w)
    if key not in _decoded:
        cal = O.synthetic_calib(h=h, w=w, profile=profile)
        pf = cal.packet_format()
        packets, _ = O.synth_packets(cal, N_E, with_window=True)
        host = packets.copy()
        host[LOST[0], LOST[1]] = 0
        a, b = SWAPPED[1]
        host[SWAPPED[0], [a, b]] = host[SWAPPED[0], [b, a]]
        host[ABSENT] = 0
        by_frame = [host[f] for f in range(N_E)]
        by_frame[LOST[0]] = np.delete(host[LOST[0]], LOST[1], axis=0)
        by_frame[ABSENT] = host[ABSENT][:0]
        ref = _oracle_frames(O, cal, pf, by_frame, True)
        host.setflags(write=False)
        _decoded[key] = (cal, host, ref)
    return _decoded[key]


@pytest.mark.parametrize("label,profile,h,w,generic,knobs,kernel,tile,field", E_CASES, ids=[c[0] for c in E_CASES])
def test_decode_gate_counts(oracle, label, profile, h, w, generic, knobs, kernel, tile, field):
    """gate_counts[f][8][W] of the decode on the routes and shapes the one test of test_gpu_fastpath.py does not take: eight row
    chunks (the limit) and ten (the wide plan must refuse), narrow tiles of 16 / 32 / 64, the persistent kernel, the generic
    path, a ragged last tile, RANGE2 -- into a buffer that starts as 0xCDCD, with a gate whose lower bound is 0 as well.  The
    yardstick is a plain count over the decoded plane, which is itself the oracle's; columns of status 0 are left out (the
    dewarp's scan masks them).  A dewarp fed with the counts gives the bytes of one that counts for itself."""
    O = oracle
    cal, host, ref = _packets(O, profile, h, w)
    hp = HotPath(profile, h, w, cal.cpp, header_type=cal.header_type)
    if generic:
        desc = capi.FormatDesc.from_buffer_copy(hp.desc)
        for i, (name, _) in enumerate(hp.fields):
            desc.fields[i].bits.offset, desc.fields[i].bits.mask, desc.fields[i].bits.shift = GENERIC_BITS[name]
        hp.fmt, hp.static_fmt = hp.ctx.make_format(desc), hp.fmt
    hp.set_pixel_shift_by_row(cal.pixel_shift_by_row)
    hp.add_lut(cal.beam_to_lidar, cal.lut_transform(False), cal.beam_azimuth_angles, cal.beam_altitude_angles)
    for k, v in {"small": 0, **knobs}.items():
        hp.ctx.set_knob(k, v)
    dev = torch.from_numpy(host.copy()).cuda()
    poses = torch.eye(4, dtype=torch.float64, device="cuda").repeat(N_E, w, 1, 1).contiguous()
    poses[:, :, 0, 3] = torch.arange(w, device="cuda", dtype=torch.float64) * 0.01
    for gate in E_GATES:
        lo, hi, empty = hp.range_gate(*gate)
        assert (lo, hi, empty) == (*D.raw_gate(*gate), False)
        out = hp.alloc_outputs(N_E)
        out["gate_counts"] = torch.empty((N_E, D.GATE_CHUNKS, w), dtype=torch.uint16, device="cuda")
        for t in out.values():
            t.view(torch.uint8).fill_(0xCD)
        hp.decode(dev, out, gate=gate, gate_field=field)
        hp.sync()
        ran = (hp.ctx.last_decode_kernel(), hp.ctx.last_decode_tile())
        if kernel is None:
            assert ran[0] != "k_decode_wide", (label, ran)      # more row chunks than count slots: the wide plan refuses
        else:
            assert ran[0].startswith(kernel) and (kernel != "k_decode" or ran[0] == kernel), (label, ran)
            assert ran[1][:len(tile)] == tile, (label, ran)
        gcounts = out.pop("gate_counts")
        _compare(O, cal, hp, out, ref, [], [])                  # the decoded planes and headers are the oracle's
        plane = out[field].to(torch.int64)
        want = ((plane >= lo) & (plane <= hi)).sum(dim=1)       # [n, W]
        got = gcounts.to(torch.int64).sum(dim=1)
        live = out["status"].to(torch.int64) != 0
        left_out = 1.0 - live.double().mean(dim=1)
        for f in range(N_E):
            if f != ABSENT:
                assert float(left_out[f]) < 0.10, (label, f, float(left_out[f]))
        assert abs(float(left_out[LOST[0]]) - 2 * cal.cpp / w) < 1e-9 and not bool(live[ABSENT].any())
        bad = (got != want) & live
        assert not bool(bad.any()), (label, gate, "first wrong (frame, column):", bad.nonzero()[:4].tolist())
        assert int(want[live].sum()) > 1000
        # the dewarp that is fed the counts against the one that counts for itself: whole batch, provenance included
        a = hp.dewarp_frames(out[field], out["status"], poses, *gate, timestamp=out["timestamp"])
        b = hp.dewarp_frames(out[field], out["status"], poses, *gate, timestamp=out["timestamp"], gate_counts=gcounts)
        assert torch.equal(a["frame_offsets"], b["frame_offsets"])
        offs = _np(a["frame_offsets"]).astype(np.int64)
        tot = int(offs[-1])
        assert tot > 1000 and offs[ABSENT + 1] == offs[ABSENT]          # the frame without packets contributes nothing
        for k in ("points", "frame_idxs", "col_idxs", "timestamps_ns"):
            assert torch.equal(_bytes(a[k][:tot]), _bytes(b[k][:tot])), (label, gate, k)
