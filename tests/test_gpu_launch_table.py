"""GPU: every row of the fused decode's launch ladder (csrc/launch_util.h) once, at the smallest shape that reaches it.

A row is (kernel family, tile width, XYZM, POSES) of one packet-profile specialisation.  A case forces one optimistic route
through the knobs of csrc/decode_plan.h and decodes two frames of 16 rows: frame 0 is clean and stays with the optimistic
kernel, frame 1 carries one pair of swapped packets and is redone by the fix-up kernel paired with the route (k_decode_fixup
with the same tile behind k_decode, k_decode_wide_fixup 128 / 256 behind the wide and the persistent kernels).  Where the row
has a POSES form (XYZM 1 / 2 outside the persistent kernels) the same call is made again with per-column poses.

  profiles   RNG19_RFL8_SIG16_NIR16 (static, 12 B/px) and the generic path: RNG15_RFL8_NIR8 described by other offsets, masks and
             shifts for the same bits (as test_gpu_parity.py::test_custom_profile_generic_kernel), which matches no static
             table and runs SpecGeneric from run-time descriptors -- no persistent kernel, which a case of its own asserts.
             The 1024-column persistent tile does not fit twice in LDS at 12 B/px whatever its height (plan_stream,
             decode_plan.cpp), so that one route runs the static RNG15_RFL8_NIR8 (4 B/px) at W = 2048.
  XYZM       0 no xyz | 1 separable tables -> f32 | 2 -> f64 | 3 full LUT arrays (not on the persistent kernels)
  compared   every plane, the column headers, the destaggered RANGE and the frame meta bit for bit with the oracle, xyz by the
             tolerance of test_gpu_parity.py; with poses against dewarp() of the same call's pose-free points by the
             tolerances of test_gpu_fastpath.py::test_poses_fused_behind_the_cartesian
  asserted   the context's last kernel name and tile width, so a row that silently took another route fails.  (The context
             does not report the fix-up kernel: its choice is forced by the `tile` / `fixup_wide` knobs, and frame 1 is
             only right if a fix-up pass ran.)
k_decode_wide_resolved (one launch, no fix-up pass: every tile resolves its frame's column maps itself) exists only in a build
made with EXPERIMENTS=1; its rows skip on a default build.
"""
import numpy as np
import pytest

from conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from ouster_sdk_amd import _capi
    from ouster_sdk_amd.device import HotPath

from test_gpu_fastpath import _compare  # noqa: E402
from test_gpu_parity import XYZ_TOL, _np, _oracle_frames  # noqa: E402

H, N = 16, 2
STATIC, STATIC_4B = "RNG19_RFL8_SIG16_NIR16", "RNG15_RFL8_NIR8"
# (offset, mask, shift) that read the fields of RNG15_RFL8_NIR8 from other bytes than its static table does
GENERIC_BITS = {"RANGE": (0, 0x7fff, -3), "FLAGS": (1, 0x80, 7), "REFLECTIVITY": (1, 0xff00, 8), "NEAR_IR": (2, 0xff00, 4)}


def _routes():
    """(label, profile, W, knobs, kernel the context must report, its tile width, XYZM values the route compiles)"""
    out = []
    for prof, tag in ((STATIC, "static"), (STATIC_4B, "generic")):
        for t in (16, 32, 64):
            out.append((f"{tag}-narrow{t}", prof, 1024, dict(tile=t, wide=0, stream=0), "k_decode", t, (0, 1, 2, 3)))
        for tw in (64, 128, 256, 512):
            out.append((f"{tag}-wide{tw}", prof, 1024, dict(wide=tw, wide_min_blocks=0, stream=0, fixup_wide=128 if tw in (64, 256) else 256),
                        "k_decode_wide", tw, (0, 1, 2, 3)))
        for tw, w in ((256, 1024), (128, 128)):   # the one-launch form takes the widest of 256 / 128 the frame has: W = 128 for the latter
            out.append((f"{tag}-resolved{tw}", prof, w, dict(small=2), "k_decode_wide_resolved", tw, (0, 1, 2, 3)))
    for tw in (128, 256):
        for loader in (0, 4):
            out.append((f"static-stream{tw}-loader{loader}", STATIC, 1024, dict(stream=tw, stream_min_tiles=0, stream_loader=loader),
                        "k_decode_stream2" if loader else "k_decode_stream", tw, (0, 1, 2)))
    out.append(("static-stream512", STATIC, 1024, dict(stream=512, stream_min_tiles=0), "k_decode_stream", 512, (0, 1, 2)))
    out.append(("static4b-stream1024", STATIC_4B, 2048, dict(stream=1024, stream_min_tiles=0), "k_decode_stream", 1024, (0, 1, 2)))
    return out


CASES = [pytest.param(*r[:6], x, id=f"{r[0]}-xyzm{x}") for r in _routes() for x in r[6]]
_data = {}


def _hotpath(cal, profile, w, generic):
    hp = HotPath(profile, H, w, cal.cpp, header_type=cal.header_type)
    if generic:
        desc = _capi.FormatDesc.from_buffer_copy(hp.desc)
        for i, (n, _) in enumerate(hp.fields):
            desc.fields[i].bits.offset, desc.fields[i].bits.mask, desc.fields[i].bits.shift = GENERIC_BITS[n]
        hp.fmt, hp.static_fmt = hp.ctx.make_format(desc), hp.fmt
    hp.set_pixel_shift_by_row(cal.pixel_shift_by_row)
    return hp


def _batch(O, profile, w):
    """The two frames of (profile, w), their oracle frames and poses: made once, shared by every case, never written."""
    if (profile, w) not in _data:
        cal = O.synthetic_calib(h=H, w=w, profile=profile)
        pf = cal.packet_format()
        packets, _ = O.synth_packets(cal, N, with_window=True)
        host = packets.copy()
        host[1, [3, 5]] = host[1, [5, 3]]            # strays: frame 1 needs the fix-up pass
        ref = _oracle_frames(O, cal, pf, [host[f] for f in range(N)], True)
        rng = np.random.default_rng(3)
        poses = np.tile(np.eye(4), (N, w, 1, 1))
        ang = rng.uniform(-0.4, 0.4, size=(N, w))
        poses[..., 0, 0] = np.cos(ang); poses[..., 0, 1] = -np.sin(ang)
        poses[..., 1, 0] = np.sin(ang); poses[..., 1, 1] = np.cos(ang)
        poses[..., :3, 3] = rng.uniform(-30, 30, size=(N, w, 3))
        for a in (host, poses):
            a.setflags(write=False)
        _data[(profile, w)] = (cal, host, ref, poses)
    return _data[(profile, w)]


@pytest.mark.parametrize("label,profile,w,knobs,kernel,cols,xyzm", CASES)
def test_launch_table_row(oracle, label, profile, w, knobs, kernel, cols, xyzm):
    O = oracle
    if kernel == "k_decode_wide_resolved" and b"experiments" not in _capi.load_hip().ouster_hip_version():
        pytest.skip("k_decode_wide_resolved is only in a build made with `make EXPERIMENTS=1`")
    cal, host, ref, poses = _batch(O, profile, w)
    hp = _hotpath(cal, profile, w, label.startswith("generic"))
    if xyzm == 3:
        hp.add_lut_arrays(*cal.xyz_lut(False))
    else:
        hp.add_lut(cal.beam_to_lidar, cal.lut_transform(False), cal.beam_azimuth_angles, cal.beam_altitude_angles)
    for k, v in {"small": 0, **knobs}.items():
        hp.ctx.set_knob(k, v)
    xyz = ["RANGE"] if xyzm else []
    tdt = torch.float64 if xyzm == 2 else torch.float32
    dev = torch.from_numpy(host.copy()).cuda()

    def decode(**kw):
        out = hp.alloc_outputs(N, destagger=["RANGE"], xyz=xyz, xyz_dtype=tdt)
        for t in out.values():
            t.view(torch.uint8).fill_(0xCD)
        hp.decode(dev, out, **kw)
        hp.sync()
        assert (hp.ctx.last_decode_kernel(), hp.ctx.last_decode_tile()[0]) == (kernel, cols), label
        return out

    plain = decode()
    assert _compare(O, cal, hp, plain, ref, ["RANGE"], xyz) <= XYZ_TOL
    if xyzm not in (1, 2) or kernel.startswith("k_decode_stream"):
        return
    fused = decode(poses=torch.from_numpy(poses.copy()).cuda())       # the POSES form of the same row
    for k in plain:
        if not k.startswith("xyz:") and k != "frame_meta":
            assert torch.equal(plain[k].view(torch.uint8), fused[k].view(torch.uint8)), k
    tol = 1e-4 if xyzm == 1 else 1e-9      # as test_poses_fused_behind_the_cartesian: f32 fma contraction vs separate mul / add
    body, got = _np(plain["xyz:RANGE"]), _np(fused["xyz:RANGE"])
    for f in range(N):
        want = O.dewarp(body[f], poses[f], H, w)
        assert np.abs(got[f].astype(np.float64) - want.astype(np.float64)).max() <= tol, (label, f)


def test_generic_format_takes_no_static_route(oracle):
    """The re-described format of the generic rows really is SpecGeneric: the persistent kernels exist for the static profiles
    only, so forcing one leaves the call on k_decode / k_decode_wide, while the profile's own description takes it."""
    cal, host, _, _ = _batch(oracle, STATIC_4B, 1024)
    dev = torch.from_numpy(host.copy()).cuda()
    for generic in (False, True):
        hp = _hotpath(cal, STATIC_4B, 1024, generic)
        for k, v in dict(small=0, stream=128, stream_min_tiles=0).items():
            hp.ctx.set_knob(k, v)
        hp.decode(dev, hp.alloc_outputs(N))
        hp.sync()
        assert hp.ctx.last_decode_kernel().startswith("k_decode_stream") == (not generic), (generic, hp.ctx.last_decode_kernel())
