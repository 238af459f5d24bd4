"""GPU parity: HIP path (through the C ABI) vs the CPU oracle on the same inputs.

Bars (BASELINE.json north_star): bit-exact for every integer plane, column header and
destaggered plane; |dXYZ| <= 1e-4 m for projected points (measured max is ~3e-5 m: one f32
rounding of a value <= 525 m).  Mirrors the reference's tests:
  tests/frame_batcher_test.cpp:548-692   snapshot captures through the batcher
  tests/packet_format_test.cpp:218-406   synthetic encode -> decode identity, dropped packets
  tests/frame_batcher_test.cpp:73-303    invalid columns / custom planes untouched
  tests/destagger_test.cpp:135-210       destagger round trip, vs np.roll
  tests/cartesian_test.cpp:53-99         float vs double projection
"""
import os

import numpy as np
import pytest

from conftest import PCAPS, has_gpu
from test_range_gate_cpu import IDS as RANGE_GATE_IDS, TABLE as RANGE_GATES

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from ouster_sdk_amd.device import HotPath

XYZ_TOL = 1e-4  # metres, north_star tolerance

CAPTURES = [
    "OS-0-128-U1_v2.3.0_1024x10",
    "OS-0-32-U1_v2.2.0_1024x10",
    "OS-1-128_767798045_1024x10_20230712_120049",
    "OS-2-128-U1_v2.3.0_1024x10",
    "OS-2-32-U0_v2.0.0_1024x10",
    "OS-1-32-G_v2.1.1_1024x10",
    "crc_test",
]
PROFILE_NAME = {}


def _pname(O, pid):
    for k, v in O.PROFILES.items():
        if v == pid:
            return k
    raise KeyError(pid)


def _np(t):
    return t.cpu().numpy()


def _oracle_frames(O, cal, pf, packets_by_frame, with_window):
    """Run the oracle batcher on each frame's packets (in the given order)."""
    frames = []
    for pk in packets_by_frame:
        fr = O.Frame.for_profile(cal.profile, cal.h, cal.w, cal.cpp, with_window=with_window)
        fr.fill(0xAB)  # stale content must be overwritten or zeroed
        b = O.Batcher(pf, init_id=O.lib().ora_init_id(pf, pk[0].ctypes.data) if len(pk) else 0,
                      expected_packets=len(pk))
        done = False
        for i, p in enumerate(pk):
            done = b.batch(p, 1 + i, fr)
        if len(pk) == 0:
            fr.fill(0)          # never started: the GPU path defines an empty frame as all zero
        elif not done:
            b.finalize(fr)      # released incomplete (duplicates / missing packets)
        frames.append(fr)
    return frames


def _check_decode(O, cal, packets_by_frame, with_window, slots=None, xyz_dtype=None,
                  use_extrinsics=False):
    """Decode on the GPU and compare everything with the oracle."""
    xyz_dtype = xyz_dtype or torch.float32
    pf = cal.packet_format()
    prof = _pname(O, cal.profile)
    hp = HotPath(prof, cal.h, cal.w, cal.cpp, header_type=cal.header_type, with_window=with_window)
    hp.set_pixel_shift_by_row(cal.pixel_shift_by_row)
    hp.add_lut(cal.beam_to_lidar, cal.lut_transform(use_extrinsics), cal.beam_azimuth_angles,
               cal.beam_altitude_angles)
    n_frames = len(packets_by_frame)
    slots = slots or max(len(p) for p in packets_by_frame)
    host = np.zeros((n_frames, slots, pf.lidar_packet_size), dtype=np.uint8)
    counts = np.zeros(n_frames, dtype=np.uint32)
    for f, pk in enumerate(packets_by_frame):
        host[f, :len(pk)] = pk
        counts[f] = len(pk)
    dev = torch.from_numpy(host).cuda()
    names = [n for n, _ in hp.fields]
    xyz_names = [n for n in ("RANGE", "RANGE2") if n in names]
    dst_names = [n for n in ("RANGE", "RANGE2", "REFLECTIVITY", "REFLECTIVITY2", "NEAR_IR") if n in names]
    out = hp.alloc_outputs(n_frames, destagger=dst_names, xyz=xyz_names, xyz_dtype=xyz_dtype)
    for t in out.values():
        t.view(torch.uint8).fill_(0xCD)
    hp.decode(dev, out, packet_counts=counts)
    hp.sync()

    ref = _oracle_frames(O, cal, pf, packets_by_frame, with_window)
    ldir, lofs = cal.xyz_lut(use_extrinsics)
    max_err = 0.0
    for f, fr in enumerate(ref):
        for n in names:
            got = _np(out[n][f])
            assert np.array_equal(got, fr.plane(n)), (f, n)
        assert np.array_equal(_np(out["timestamp"][f]), fr.timestamp), f
        assert np.array_equal(_np(out["measurement_id"][f]), fr.measurement_id), f
        assert np.array_equal(_np(out["status"][f]), fr.status), f
        for n in dst_names:
            want = O.destagger(fr.plane(n), cal.pixel_shift_by_row)
            assert np.array_equal(_np(out["destaggered:" + n][f]), want), (f, n)
        for n in xyz_names:
            want = O.cartesian(fr.plane(n), ldir, lofs)  # reference cartesian(): double
            got = _np(out["xyz:" + n][f]).astype(np.float64)
            err = np.abs(got - want).max()
            max_err = max(max_err, err)
            assert err <= XYZ_TOL, (f, n, err)
            assert np.all(got[fr.plane(n).reshape(-1) == 0] == 0)
        meta = _np(out["frame_meta"][f]).view(np.int64)
        if len(packets_by_frame[f]):
            assert meta[0] == fr.frame_id
    return max_err


@pytest.mark.parametrize("base", CAPTURES)
def test_captures_match_oracle(oracle, base):
    O = oracle
    cal = O.calib_from_json(os.path.join(PCAPS, base + ".json"))
    pf = cal.packet_format()
    pk = O.lidar_packets_from_pcap(os.path.join(PCAPS, base + ".pcap"), pf)
    assert len(pk) > 0
    # split the capture into frames by frame id, as the host-side batcher does
    import ctypes as C
    fids = [O.lib().ora_frame_id(C.byref(pf), p.ctypes.data) for p in pk]
    frames, cur = [], [0]
    for i in range(1, len(pk)):
        if fids[i] != fids[i - 1]:
            frames.append(pk[cur]); cur = []
        cur.append(i)
    frames.append(pk[cur])
    err = _check_decode(O, cal, frames, with_window=False, slots=cal.w // cal.cpp)
    assert err <= 4e-5


@pytest.mark.parametrize("profile,h,w,hdr", [
    ("RNG15_RFL8_NIR8_DUAL", 128, 2048, 0),
    ("FUSA_RNG15_RFL8_NIR8_DUAL", 128, 1024, 1),
    ("RNG19_RFL8_SIG16_NIR16", 128, 2048, 0),
    ("RNG19_RFL8_SIG16_NIR16_DUAL", 128, 1024, 0),
    ("RNG15_RFL8_NIR8", 64, 512, 0),
    ("LEGACY", 64, 1024, 0),
    ("FIVE_WORD_PIXEL", 32, 512, 0),
    ("RNG19_RFL8_SIG16_NIR16_RGB16", 32, 512, 0),
    ("RNG15_RFL8_NIR8_ZONE16", 16, 512, 0),
])
def test_synthetic_roundtrip(oracle, profile, h, w, hdr):
    """encode -> GPU decode identity + oracle equality, 9 frames (exercises the XCD map)."""
    O = oracle
    cal = O.synthetic_calib(h=h, w=w, profile=profile, header_type=hdr)
    packets, src = O.synth_packets(cal, 9, with_window=True)
    err = _check_decode(O, cal, [packets[f] for f in range(9)], with_window=True)
    # one f32 rounding: half an ulp of the largest coordinate (20-bit LEGACY ranges reach 1048 m)
    assert err <= (6.2e-5 if profile == "LEGACY" else 4e-5)


def test_dropped_invalid_shuffled(oracle):
    """Dropped packets, invalid columns, out-of-range m_id, shuffled order, duplicates."""
    O = oracle
    cal = O.synthetic_calib(h=128, w=1024, profile="RNG15_RFL8_NIR8_DUAL")
    pf = cal.packet_format()
    packets, _ = O.synth_packets(cal, 10)
    rng = np.random.default_rng(7)
    frames = []
    for f in range(10):
        pk = packets[f].copy()
        keep = np.ones(len(pk), bool)
        if f % 3 == 0:
            keep[rng.integers(0, len(pk), 3)] = False      # dropped packets
        if f % 3 == 1:  # invalid columns: clear status bit 0 (packet_format_test.cpp:374-382)
            for p in rng.integers(0, len(pk), 4):
                for c in rng.integers(0, 16, 5):
                    off = pf.packet_header_size + c * pf.col_size + 10
                    pk[p, off] &= 0xFE
        if f == 5:  # one column claims a measurement id beyond the frame
            off = pf.packet_header_size + 3 * pf.col_size + 8
            pk[7, off:off + 2] = np.frombuffer(np.uint16(5000).tobytes(), np.uint8)
        pk = pk[keep]
        if f % 2 == 0:
            pk = pk[rng.permutation(len(pk))]               # any order within a frame
        if f == 9:
            pk = np.concatenate([pk, pk[10:12]])            # duplicate packets (same data)
        frames.append(pk)
    frames.append(np.zeros((0, pf.lidar_packet_size), np.uint8))  # empty frame -> all zero
    _check_decode(O, cal, frames, with_window=True, slots=70)


def test_custom_profile_generic_kernel(oracle):
    """add_custom_profile-style layout (tests/frame_batcher_test.cpp:676-704) through the
    descriptor-driven kernel must equal the built-in profile's result."""
    O = oracle
    import ctypes as C
    from ouster_sdk_amd import _capi as capi
    cal = O.synthetic_calib(h=128, w=1024, profile="RNG15_RFL8_NIR8")
    packets, _ = O.synth_packets(cal, 3)
    hp = HotPath("RNG15_RFL8_NIR8", 128, 1024, 16)
    # alternative encodings of the same bits: REFLECTIVITY read from byte 1 with mask 0xff00>>8, ...
    alt = {"RANGE": (0, 0x7fff, -3), "FLAGS": (1, 0x80, 7), "REFLECTIVITY": (1, 0xff00, 8),
           "NEAR_IR": (2, 0xff00, 4)}
    desc = capi.FormatDesc.from_buffer_copy(hp.desc)
    for i, (n, _) in enumerate(hp.fields):
        desc.fields[i].bits.offset, desc.fields[i].bits.mask, desc.fields[i].bits.shift = alt[n]
    fmt2 = hp.ctx.make_format(desc)
    dev = torch.from_numpy(packets).cuda()
    o1 = hp.alloc_outputs(3)
    hp.decode(dev, o1)
    hp.fmt, keep = fmt2, hp.fmt
    o2 = hp.alloc_outputs(3)
    hp.decode(dev, o2)
    hp.sync()
    for n, _ in hp.fields:
        assert torch.equal(o1[n], o2[n]), n


@pytest.mark.parametrize("dtype,w,extra", [
    (np.uint8, 1024, 1), (np.uint16, 2048, 1), (np.uint32, 2048, 1), (np.uint64, 512, 1),
    (np.float32, 1024, 1), (np.float64, 512, 1), (np.uint16, 512, 3), (np.uint32, 1000, 1),
    (np.uint8, 999, 1),
])
def test_destagger_matches_oracle(oracle, dtype, w, extra):
    O = oracle
    h = 128
    rng = np.random.default_rng(3)
    shifts = rng.integers(-30, 31, h).astype(np.int32)  # destagger_test.cpp:123-133
    shape = (4, h, w) if extra == 1 else (4, h, w, extra)
    img = rng.integers(0, 255, size=shape).astype(dtype)
    hp = HotPath("RNG15_RFL8_NIR8", h, 1024, 16)
    d_img = torch.from_numpy(img.view(np.uint8).reshape(4, h, w, -1)).cuda()
    for inverse in (False, True):
        got = _np(hp.destagger(d_img, shifts, inverse=inverse)).view(dtype).reshape(shape)
        for k in range(4):
            want = O.destagger(img[k], shifts, inverse)
            assert np.array_equal(got[k], want)
            if (w & (w - 1)) == 0:  # power-of-two widths: equals np.roll (reference.py:131-158)
                roll = np.stack([np.roll(img[k][u], (-1 if inverse else 1) * shifts[u], axis=0)
                                 for u in range(h)])
                assert np.array_equal(got[k], roll)
    # round trip: stagger(destagger(x)) == x
    back = hp.destagger(hp.destagger(d_img, shifts), shifts, inverse=True)
    if (w & (w - 1)) == 0:
        assert torch.equal(back, d_img)
    with pytest.raises(ValueError, match="image height does not match shifts size"):
        hp.destagger(d_img, shifts[:-1])


def test_cartesian_standalone(oracle):
    O = oracle
    cal = O.synthetic_calib(h=128, w=1024, b2l_x=15.806)
    ext = np.eye(4)
    ext[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    ext[:3, 3] = [1.5, -2.0, 0.25]
    cal.extrinsic = ext
    rng = np.random.default_rng(11)
    r = rng.integers(0, 2 ** 19, size=(3, 128, 1024)).astype(np.uint32)
    r[rng.random(r.shape) < 0.3] = 0
    r[0, 0, :8] = 2 ** 19 - 8  # max range
    ldir, lofs = cal.xyz_lut(True)
    hp = HotPath("RNG15_RFL8_NIR8", 128, 1024, 16)
    lut = hp.add_lut(cal.beam_to_lidar, cal.lut_transform(True), cal.beam_azimuth_angles,
                     cal.beam_altitude_angles)
    d, o = lut.export(1024, 128)
    assert np.abs(d - ldir).max() < 1e-15 and np.abs(o - lofs).max() < 1e-12
    dr = torch.from_numpy(r).cuda()
    want = np.stack([O.cartesian(r[k], ldir, lofs) for k in range(3)])
    g64 = _np(hp.cartesian(dr, dtype=torch.float64))
    assert np.abs(g64 - want).max() < 1e-9            # separable tables vs full double LUT
    g32 = _np(hp.cartesian(dr, dtype=torch.float32)).astype(np.float64)
    assert np.abs(g32 - want).max() <= 4e-5
    # user-supplied LUT arrays (XYZLutT<float> / XYZLutT<double> objects)
    lut32 = hp.add_lut_arrays(ldir.astype(np.float32), lofs.astype(np.float32))
    want32 = np.stack([O.cartesian(r[k], ldir.astype(np.float32), lofs.astype(np.float32))
                       for k in range(3)])
    got32 = _np(hp.cartesian(dr, lut=lut32, dtype=torch.float32))
    assert np.array_equal(got32, want32)               # same f32 mul+add as cartesianT<float>
    assert np.abs(got32.astype(np.float64) - want).max() <= XYZ_TOL
    lut64 = hp.add_lut_arrays(ldir, lofs)
    got64 = _np(hp.cartesian(dr, lut=lut64, dtype=torch.float64))
    assert np.array_equal(got64, want)
    with pytest.raises(ValueError):
        hp.cartesian(dr[:, :64].contiguous())


def test_lut_dimension_errors(oracle):
    hp = HotPath("RNG15_RFL8_NIR8", 128, 1024, 16)
    az = np.zeros(128)
    with pytest.raises(ValueError, match="unexpected frame dimensions"):
        hp.add_lut(np.eye(4), np.eye(4), az[:-1], az[:-1])
    with pytest.raises(ValueError, match="unexpected frame dimensions"):
        hp.add_lut(np.eye(4), np.eye(4), az, az[:-1])


def test_full_size_properties(oracle):
    """BASELINE config 3 size (128x2048 dual, 64 frames): oracle-free invariants."""
    O = oracle
    cal = O.synthetic_calib(h=128, w=2048, profile="RNG15_RFL8_NIR8_DUAL")
    packets, src = O.synth_packets(cal, 4)
    n = 64
    host = np.concatenate([packets] * (n // 4))
    hp = HotPath("RNG15_RFL8_NIR8_DUAL", 128, 2048, 16)
    hp.set_pixel_shift_by_row(cal.pixel_shift_by_row)
    hp.add_lut(cal.beam_to_lidar, cal.lut_transform(False), cal.beam_azimuth_angles,
               cal.beam_altitude_angles)
    dev = torch.from_numpy(host).cuda()
    out = hp.alloc_outputs(n, destagger=["RANGE", "RANGE2", "REFLECTIVITY", "REFLECTIVITY2"],
                           xyz=["RANGE", "RANGE2"])
    hp.decode(dev, out)
    hp.sync()
    # (1) decode(encode(x)) == x for every plane of every frame
    for f in range(n):
        for name, _ in hp.fields:
            assert np.array_equal(_np(out[name][f]), src[f % 4].plane(name)), (f, name)
    # (2) identical inputs -> identical outputs (frames repeat with period 4)
    for k in ("xyz:RANGE", "xyz:RANGE2", "destaggered:RANGE", "destaggered:REFLECTIVITY2"):
        assert torch.equal(out[k][:4].repeat((n // 4,) + (1,) * (out[k].dim() - 1)), out[k])
    # (3) stagger(destaggered) == staggered plane
    back = hp.destagger(out["destaggered:RANGE"], inverse=True)
    assert torch.equal(back, out["RANGE"])
    # (4) zero range <-> zero point; non-zero range within the sensor's reach
    xyz = out["xyz:RANGE"].view(n, 128, 2048, 3)
    zero = out["RANGE"].to(torch.int64) == 0
    assert torch.all(xyz[zero] == 0)
    norm = torch.linalg.vector_norm(xyz.double(), dim=-1)
    rm = out["RANGE"].to(torch.float64) * 1e-3
    assert torch.all((norm - rm).abs()[~zero] < 0.06)  # |p| ~ r up to the beam origin offset


def test_multi_sensor_batch_per_sensor_extrinsics(oracle):
    """BASELINE config 5: 4 sensors interleaved in one batch (sensor = frame % 4), each with
    its own extrinsics folded into its LUT (xyzlut.cpp:91-102) and applied in-kernel."""
    O = oracle
    n_sensors, ticks = 4, 3
    cals = []
    for s_ in range(n_sensors):
        c = O.synthetic_calib(h=128, w=1024, profile="RNG15_RFL8_NIR8_DUAL")
        a = 0.4 * (s_ + 1)
        ext = np.eye(4)
        ext[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
        ext[:3, 3] = [1.0 * s_, -0.5 * s_, 0.1 * s_]          # metres
        c.extrinsic = ext
        cals.append(c)
    hp = HotPath("RNG15_RFL8_NIR8_DUAL", 128, 1024, 16)
    for c in cals:
        hp.add_lut(c.beam_to_lidar, c.lut_transform(True), c.beam_azimuth_angles,
                   c.beam_altitude_angles)
    packets, src = O.synth_packets(cals[0], n_sensors * ticks)
    out = hp.alloc_outputs(n_sensors * ticks, planes=["RANGE", "RANGE2"], xyz=["RANGE", "RANGE2"])
    hp.decode(torch.from_numpy(packets).cuda(), out)
    hp.sync()
    luts = [c.xyz_lut(True) for c in cals]
    for f in range(n_sensors * ticks):
        d, o = luts[f % n_sensors]
        for name in ("RANGE", "RANGE2"):
            want = O.cartesian(src[f].plane(name), d, o)
            got = _np(out["xyz:" + name][f]).astype(np.float64)
            assert np.abs(got - want).max() <= 4e-5, (f, name)
    # different sensors really produce different clouds for the same ranges
    assert not torch.equal(out["xyz:RANGE"][0], out["xyz:RANGE"][1])


def test_dense_dewarp_matches_oracle(oracle):
    """dewarp<T>(points, poses) (pose_util.h:38-56): per-column pose applied to every point."""
    O = oracle
    h, w, n = 64, 512, 3
    rng = np.random.default_rng(21)
    hp = HotPath("RNG15_RFL8_NIR8", h, w, 16)
    poses = np.tile(np.eye(4), (n, w, 1, 1))
    ang = rng.uniform(-0.2, 0.2, size=(n, w))
    poses[..., 0, 0] = np.cos(ang); poses[..., 0, 1] = -np.sin(ang)
    poses[..., 1, 0] = np.sin(ang); poses[..., 1, 1] = np.cos(ang)
    poses[..., :3, 3] = rng.uniform(-5, 5, size=(n, w, 3))
    for dt, tdt in ((np.float64, torch.float64), (np.float32, torch.float32)):
        pts = rng.uniform(-100, 100, size=(n, h * w, 3)).astype(dt)
        got = _np(hp.dewarp(torch.from_numpy(pts).cuda(), torch.from_numpy(poses).cuda()))
        want = np.stack([O.dewarp(pts[k], poses[k], h, w) for k in range(n)])
        tol = 1e-12 if dt == np.float64 else 2e-5   # f32: fma contraction vs separate mul/add
        assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= tol
    # identity poses leave the cloud unchanged
    ident = torch.from_numpy(np.tile(np.eye(4), (n, w, 1, 1))).cuda()
    p32 = torch.from_numpy(pts).cuda()
    assert torch.equal(hp.dewarp(p32, ident), p32)


@pytest.mark.parametrize("path", ["runs", "single", "stream"])
@pytest.mark.parametrize("h,w,n", [(128, 1024, 3), (64, 512, 4), (32, 512, 2), (9, 100, 2), (70, 130, 2), (130, 64, 1), (260, 72, 2)])
def test_dewarp_frames_matches_oracle(oracle, h, w, n, path):
    """dewarp(LidarFrame / FrameSet, XYZLut, min_range, max_range) with provenance
    (impl/dewarp_impl.h:23-115): order, counts, col/frame indices and timestamps bit-exact;
    points within the XYZ bar."""
    O = oracle
    from ouster_sdk_amd import _capi
    if path in ("single", "stream") and b"experiments" not in _capi.load_hip().ouster_hip_version():
        pytest.skip("the single-pass and the persistent dewarp kernels are only in a build made with `make EXPERIMENTS=1` (round 6 hygiene)")
    rng = np.random.default_rng(h * 31 + w)
    cal = O.synthetic_calib(h=h, w=w, b2l_x=15.806)
    ldir, lofs = cal.xyz_lut(True)
    hp = HotPath("RNG15_RFL8_NIR8", h, w, 4 if w % 4 == 0 else 1)
    # count / scan / emit (the default) or k_dwf_single (one pass, decoupled look-back)
    hp.ctx.set_knob("dewarp_single_pass", 1 if path == "single" else 0)
    # "stream": the persistent, LDS-DMA double-buffered k_dwf_emit_stream wherever the shape allows it (whole 64-column tiles of
    # exactly h = 64 / 128 rows, float output, separable tables; by itself it only takes batches of >= 2048 tiles), else k_dwf_emit
    hp.ctx.set_knob("dwf_stream", 1 if path == "stream" else 0)
    hp.add_lut(cal.beam_to_lidar, cal.lut_transform(True), cal.beam_azimuth_angles,
               cal.beam_altitude_angles)
    r = rng.integers(0, 2 ** 17, size=(n, h, w)).astype(np.uint32)
    r[rng.random(r.shape) < 0.3] = 0
    status = np.ones((n, w), dtype=np.uint32)
    status[0, :5] = 0                       # leading invalid columns
    status[0, w - 3:] = 0                   # trailing invalid columns
    status[0, w // 2] = 0                   # a hole
    status[0, w // 2 + 1] = 2               # non-zero but not "valid": still emitted (status == 0 test)
    if n > 1:
        status[1, :] = 0                    # a frame without valid columns contributes nothing
        status[1, 7] = 2
    ts = (rng.integers(1, 2 ** 62, size=(n, w))).astype(np.uint64)
    poses = np.tile(np.eye(4), (n, w, 1, 1))
    ang = rng.uniform(-0.3, 0.3, size=(n, w))
    poses[..., 0, 0] = np.cos(ang); poses[..., 0, 1] = -np.sin(ang)
    poses[..., 1, 0] = np.sin(ang); poses[..., 1, 1] = np.cos(ang)
    poses[..., :3, 3] = rng.uniform(-20, 20, size=(n, w, 3))
    d_r, d_st = torch.from_numpy(r).cuda(), torch.from_numpy(status).cuda()
    d_ts, d_po = torch.from_numpy(ts).cuda(), torch.from_numpy(poses).cuda()
    for (lo, hi) in ((0.0, 1000.0), (1.0, 60.0), (0.0005, 0.0009), (50.0, 10.0)):
        for ldt, tdt, tol in ((np.float64, torch.float64, 1e-9), (np.float32, torch.float32, 1e-4)):
            want = [O.dewarp_frame(r[k], status[k], ts[k], poses[k], ldir.astype(ldt), lofs.astype(ldt), lo, hi)
                    for k in range(n)]
            offs = np.concatenate([[0], np.cumsum([len(x[0]) for x in want])]).astype(np.uint64)
            got = hp.dewarp_frames(d_r, d_st, d_po, lo, hi, timestamp=d_ts, dtype=tdt)
            g_off = _np(got["frame_offsets"])
            assert np.array_equal(g_off, offs), (lo, hi)
            tot = int(offs[-1])
            assert np.array_equal(_np(got["col_idxs"])[:tot], np.concatenate([x[1] for x in want]))
            assert np.array_equal(_np(got["timestamps_ns"])[:tot], np.concatenate([x[2] for x in want]))
            assert np.array_equal(_np(got["frame_idxs"])[:tot],
                                  np.concatenate([np.full(len(x[0]), k, np.uint32) for k, x in enumerate(want)]))
            if tot:
                wp = np.concatenate([x[0] for x in want]).astype(np.float64)
                assert np.abs(_np(got["points"])[:tot].astype(np.float64) - wp).max() <= tol
            if tdt == torch.float32 and path == "stream":
                # the two emit kernels share their arithmetic: every byte of every output is the same; also where the result
                # does not fit (capacity: the per-point room check of the column loop instead of its easy path)
                hp.ctx.set_knob("dwf_stream", 0)
                plain = hp.dewarp_frames(d_r, d_st, d_po, lo, hi, timestamp=d_ts, dtype=tdt)
                hp.ctx.set_knob("dwf_stream", 1)
                for k in got:
                    n_k = tot if k != "frame_offsets" else len(offs)
                    assert torch.equal(plain[k][:n_k], got[k][:n_k]), (k, lo, hi)
                if tot > 3:
                    cap = tot // 2
                    part = hp.dewarp_frames(d_r, d_st, d_po, lo, hi, timestamp=d_ts, dtype=tdt, capacity=cap)
                    assert np.array_equal(_np(part["frame_offsets"]), offs)
                    for k in ("points", "col_idxs", "frame_idxs", "timestamps_ns"):
                        assert torch.equal(part[k][:cap], got[k][:cap]), (k, lo, hi, "capacity")
            if tdt == torch.float32:
                # the poses as float rows (ouster_hip_dewarp_frames_rows: 48 B per column): dewarp<float> casts the pose to
                # float before it multiplies, so every byte of every output is the same
                rows = hp.dewarp_frames(d_r, d_st, HotPath.pose_rows(poses), lo, hi, timestamp=d_ts, dtype=tdt)
                for k in got:
                    n_k = tot if k != "frame_offsets" else len(offs)
                    assert torch.equal(rows[k][:n_k], got[k][:n_k]), (k, lo, hi)
    # user-supplied f32 LUT: the reference's own XYZLutT<float> arithmetic, then the pose in f32
    l32 = hp.add_lut_arrays(ldir.astype(np.float32), lofs.astype(np.float32))
    got = hp.dewarp_frames(d_r, d_st, d_po, 1.0, 60.0, luts=[l32], dtype=torch.float32, provenance=False)
    want = [O.dewarp_frame(r[k], status[k], ts[k], poses[k], ldir.astype(np.float32), lofs.astype(np.float32), 1.0, 60.0)
            for k in range(n)]
    tot = sum(len(x[0]) for x in want)
    assert int(_np(got["frame_offsets"])[-1]) == tot and set(got) == {"points", "frame_offsets"}
    wp = np.concatenate([x[0] for x in want])
    assert np.abs(_np(got["points"])[:tot].astype(np.float64) - wp.astype(np.float64)).max() <= 3e-5  # fma vs mul+add
    # capacity smaller than the result: offsets still complete, the prefix is intact
    cap = max(tot // 2, 1)
    got2 = hp.dewarp_frames(d_r, d_st, d_po, 1.0, 60.0, luts=[l32], dtype=torch.float32, provenance=False,
                            capacity=cap)
    assert int(_np(got2["frame_offsets"])[-1]) == tot
    assert torch.equal(got2["points"][:cap], got["points"][:cap])


@pytest.mark.parametrize("gate,expected", RANGE_GATES, ids=RANGE_GATE_IDS)
def test_dewarp_frames_range_gates(oracle, gate, expected):
    """The frame dewarp at the edges of its range gate (tests/test_range_gate_cpu.py has the arithmetic): 2 frames of 4 x 16, every
    column valid, ranges from the values a threshold can sit on.  frame_offsets and the points are the oracle's; an empty gate
    leaves frame_offsets all zeros.  The oracle converts its thresholds with a plain C cast, which is defined inside
    [0, 2^32 - 1] only, so it is handed the gate clamped to that interval -- what the saturation does to a gate that is not empty."""
    O = oracle
    h, w, n = 4, 16, 2
    min_r, max_r, empty = expected
    rng = np.random.default_rng(5)
    cal = O.synthetic_calib(h=h, w=w, b2l_x=15.806)
    ldir, lofs = cal.xyz_lut(True)
    hp = HotPath("RNG15_RFL8_NIR8", h, w, 4)
    hp.add_lut(cal.beam_to_lidar, cal.lut_transform(True), cal.beam_azimuth_angles, cal.beam_altitude_angles)
    r = rng.choice(np.array([0, 1, 2, 2000, 2500, 0xffffffff], np.uint32), size=(n, h, w))
    status = np.ones((n, w), dtype=np.uint32)
    ts = rng.integers(1, 2 ** 62, size=(n, w)).astype(np.uint64)
    poses = np.tile(np.eye(4), (n, w, 1, 1))
    ang = rng.uniform(-0.3, 0.3, size=(n, w))
    poses[..., 0, 0] = np.cos(ang); poses[..., 0, 1] = -np.sin(ang)
    poses[..., 1, 0] = np.sin(ang); poses[..., 1, 1] = np.cos(ang)
    poses[..., :3, 3] = rng.uniform(-20, 20, size=(n, w, 3))
    d_r, d_st, d_po = torch.from_numpy(r).cuda(), torch.from_numpy(status).cuda(), torch.from_numpy(poses).cuda()
    lo, hi = gate
    o_lo, o_hi = max(float(lo), 0.0), min(float(hi), 4294967.2951)   # floor(4294967.2951e3) == 2^32 - 1
    for ldt, tdt, tol in ((np.float64, torch.float64, 1e-9), (np.float32, torch.float32, 1e-4)):
        got = hp.dewarp_frames(d_r, d_st, d_po, lo, hi, dtype=tdt, provenance=False)
        g_off = _np(got["frame_offsets"])
        if empty:
            assert np.array_equal(g_off, np.zeros(n + 1, np.uint64)), gate
            continue
        want = [O.dewarp_frame(r[k], status[k], ts[k], poses[k], ldir.astype(ldt), lofs.astype(ldt), o_lo, o_hi)[0] for k in range(n)]
        kept = [int(((r[k] >= min_r) & (r[k] <= max_r)).sum()) for k in range(n)]
        assert [len(x) for x in want] == kept, gate          # the clamped gate is the table's gate
        offs = np.concatenate([[0], np.cumsum(kept)]).astype(np.uint64)
        assert np.array_equal(g_off, offs), gate
        tot = int(offs[-1])
        if tot:
            # the bars of test_dewarp_frames_matches_oracle are for points within 525 m (the f32 one is a few f32 roundings of
            # such a value); range 0xffffffff lies 4.3e6 m out, so a point's bar grows with its own distance beyond 525 m
            wp = np.concatenate(want).astype(np.float64)
            bar = tol * np.maximum(1.0, np.abs(wp).max(axis=1, keepdims=True) / 525.0)
            assert (np.abs(_np(got["points"])[:tot].astype(np.float64) - wp) <= bar).all(), gate


@pytest.mark.parametrize("h,w", [(16, 100), (33, 1001), (7, 36), (128, 2048), (40, 1088)])
def test_standalone_kernels_shapes(oracle, h, w):
    """k_cartesian_tiled / k_dewarp_tiled (W % 4 == 0: full + ragged 64-column tiles, row chunks that
    are not multiples of 16) and the generic fallbacks (W % 4 != 0) against the oracle."""
    O = oracle
    rng = np.random.default_rng(h * 10007 + w)
    cal = O.synthetic_calib(h=h, w=w, b2l_x=27.67)
    ldir, lofs = cal.xyz_lut(True)
    hp = HotPath("RNG15_RFL8_NIR8", h, w, 4 if w % 4 == 0 else 1)
    lut = hp.add_lut(cal.beam_to_lidar, cal.lut_transform(True), cal.beam_azimuth_angles,
                     cal.beam_altitude_angles)
    n = 2
    r = rng.integers(0, 2 ** 19, size=(n, h, w)).astype(np.uint32)
    r[rng.random(r.shape) < 0.2] = 0
    dr = torch.from_numpy(r).cuda()
    want = np.stack([O.cartesian(r[k], ldir, lofs) for k in range(n)])
    assert np.abs(_np(hp.cartesian(dr, dtype=torch.float64)) - want).max() < 1e-9
    assert np.abs(_np(hp.cartesian(dr, dtype=torch.float32)).astype(np.float64) - want).max() <= 4e-5
    for ldt, tdt in ((np.float32, torch.float32), (np.float64, torch.float64)):
        l = hp.add_lut_arrays(ldir.astype(ldt), lofs.astype(ldt))
        w_l = np.stack([O.cartesian(r[k], ldir.astype(ldt), lofs.astype(ldt)) for k in range(n)])
        assert np.array_equal(_np(hp.cartesian(dr, lut=l, dtype=tdt)), w_l), ldt
    poses = np.tile(np.eye(4), (n, w, 1, 1))
    ang = rng.uniform(-0.3, 0.3, size=(n, w))
    poses[..., 0, 0] = np.cos(ang); poses[..., 0, 2] = np.sin(ang)
    poses[..., 2, 0] = -np.sin(ang); poses[..., 2, 2] = np.cos(ang)
    poses[..., :3, 3] = rng.uniform(-5, 5, size=(n, w, 3))
    for dt, tol in ((np.float64, 1e-12), (np.float32, 2e-5)):
        pts = rng.uniform(-100, 100, size=(n, h * w, 3)).astype(dt)
        got = _np(hp.dewarp(torch.from_numpy(pts).cuda(), torch.from_numpy(poses).cuda()))
        want_d = np.stack([O.dewarp(pts[k], poses[k], h, w) for k in range(n)])
        assert np.abs(got.astype(np.float64) - want_d.astype(np.float64)).max() <= tol


@pytest.mark.parametrize("profile,h,w,cpp", [
    ("RNG15_RFL8_NIR8", 30, 1002, 6),             # W % 4 != 0, cpp does not divide the tile, ragged tile
    ("RNG19_RFL8_SIG16_NIR16_DUAL", 17, 136, 8),  # tiny odd frame, 16 B/px
    ("RNG15_RFL8_NIR8_DUAL", 128, 4096, 32),      # widest mode, 32-column packets
    ("LEGACY", 16, 512, 16),
])
def test_odd_geometries(oracle, profile, h, w, cpp):
    """Frame shapes no sensor ships: element-wise store path, per-column staging, ragged tiles."""
    O = oracle
    cal = O.synthetic_calib(h=h, w=w, cpp=cpp, profile=profile)
    packets, _ = O.synth_packets(cal, 3, with_window=True)
    frames = [packets[0], packets[1][::-1].copy(), packets[2][: packets.shape[1] - 2]]
    _check_decode(O, cal, frames, with_window=True, slots=packets.shape[1])


def test_decode_is_graph_capturable(oracle):
    """The launch sequence of ouster_hip_decode (optimistic k_decode pass + fix-up pass) is
    stream-capturable once the scratch / LUT / offset caches are warm and packet_counts is NULL or a
    device array: capture it in a HIP graph, replay it on new packet contents in the same buffers,
    compare with the oracle (loss patterns across replays: tests/test_gpu_fastpath.py)."""
    O = oracle
    cal = O.synthetic_calib(h=64, w=512, profile="RNG15_RFL8_NIR8_DUAL")
    pk_a, _ = O.synth_packets(cal, 2, seed=5, with_window=True)
    pk_b, src_b = O.synth_packets(cal, 2, seed=6, with_window=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        hp = HotPath("RNG15_RFL8_NIR8_DUAL", 64, 512, 16)
        hp.set_pixel_shift_by_row(cal.pixel_shift_by_row)
        hp.add_lut(cal.beam_to_lidar, cal.lut_transform(True), cal.beam_azimuth_angles,
                   cal.beam_altitude_angles)
        d_pk = torch.from_numpy(pk_a).cuda()
        out = hp.alloc_outputs(2, destagger=["RANGE"], xyz=["RANGE", "RANGE2"])
        hp.decode(d_pk, out)          # warm: uploads the offsets / LUT descriptors, allocates scratch
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            hp.decode(d_pk, out)
        d_pk.copy_(torch.from_numpy(pk_b))
        g.replay()
        g.replay()                     # no state survives a replay
        s.synchronize()
    torch.cuda.synchronize()
    ldir, lofs = cal.xyz_lut(True)
    for f in range(2):
        want = src_b[f]                # encode -> decode identity (test_synthetic_roundtrip)
        for name in ("RANGE", "RANGE2", "REFLECTIVITY", "NEAR_IR"):
            assert np.array_equal(_np(out[name][f]), want.plane(name)), name
        assert np.array_equal(_np(out["destaggered:RANGE"][f]),
                              O.destagger(want.plane("RANGE"), cal.pixel_shift_by_row))
        x = O.cartesian(want.plane("RANGE2"), ldir, lofs)
        assert np.abs(_np(out["xyz:RANGE2"][f]).astype(np.float64) - x).max() <= 4e-5


@pytest.mark.parametrize("tw", [128, 256, 512])
@pytest.mark.parametrize("profile,h,w,hdr", [
    ("RNG15_RFL8_NIR8_DUAL", 128, 2048, 0),        # the metric profile: 2 or 4 row chunks per tile
    ("RNG19_RFL8_SIG16_NIR16", 128, 1024, 0),      # 12 B/px: rows per tile not a power of two
    ("RNG19_RFL8_SIG16_NIR16_DUAL", 64, 1024, 0),
    ("LEGACY", 64, 1024, 0),
    ("FIVE_WORD_PIXEL", 32, 512, 0),               # generic descriptors, 20 B/px
    ("RNG19_RFL8_SIG16_NIR16_RGB16", 32, 512, 0),  # 3 x f16 plane (6 B elements, NaN for absent columns)
    ("RNG19_RFL8_SIG16_ZONE16_DUAL", 16, 512, 0),
    ("RNG15_RFL8_NIR8", 30, 1000, 0),              # ragged last tile, W % 64 != 0, short last row chunk
])
def test_wide_tiles_match_oracle(oracle, monkeypatch, tw, profile, h, w, hdr):
    """k_decode_wide (TW columns x TR rows tiles, row-chunked staging) forced for small batches:
    same results as the oracle, incl. dropped packets / invalid columns."""
    O = oracle
    monkeypatch.setenv("OUSTER_HIP_WIDE", str(tw))
    monkeypatch.setenv("OUSTER_HIP_WIDE_MIN_BLOCKS", "0")
    cpp = 8 if w == 1000 else 16
    cal = O.synthetic_calib(h=h, w=w, cpp=cpp, profile=profile, header_type=hdr)
    packets, src = O.synth_packets(cal, 9, with_window=True)
    by_frame = [packets[f] for f in range(9)]
    by_frame[3] = np.delete(by_frame[3], [2, 7], axis=0)          # two dropped packets
    pf = cal.packet_format()
    if hdr == 0 and profile != "LEGACY":   # invalid columns: clear status bit 0 (packet_format_test.cpp:374-382)
        bad = by_frame[5].copy()
        for c in (0, 3, cpp - 1):
            bad[1, pf.packet_header_size + c * pf.col_size + 10] &= 0xFE
        by_frame[5] = bad
    by_frame[6] = by_frame[6][::-1].copy()                         # reversed order
    err = _check_decode(O, cal, by_frame, with_window=True)
    assert err <= (6.2e-5 if profile == "LEGACY" else 4e-5)


def test_variant_tuner_is_transparent(oracle):
    """A batch large enough for the per-workload tuner (>= 512 workgroups): the first calls run the
    256-wide, 128-wide and 64-column kernels (four launches each), then the fastest; every call must produce the
    same bytes, and they must match the oracle."""
    O = oracle
    cal = O.synthetic_calib(h=128, w=2048, profile="RNG15_RFL8_NIR8_DUAL")
    packets, src = O.synth_packets(cal, 4, with_window=True)
    n = 32
    hp = HotPath("RNG15_RFL8_NIR8_DUAL", 128, 2048, 16)
    hp.set_pixel_shift_by_row(cal.pixel_shift_by_row)
    hp.add_lut(cal.beam_to_lidar, cal.lut_transform(True), cal.beam_azimuth_angles, cal.beam_altitude_angles)
    d_pk = torch.from_numpy(packets).cuda().repeat(n // 4, 1, 1).contiguous()
    dst = ["RANGE", "RANGE2", "REFLECTIVITY", "REFLECTIVITY2"]
    seen, first = [], None
    for call in range(15):
        out = hp.alloc_outputs(n, destagger=dst, xyz=["RANGE", "RANGE2"])
        for t in out.values():
            t.view(torch.uint8).fill_(0xA5)
        hp.decode(d_pk, out)
        hp.sync()
        seen.append(hp.ctx.last_decode_tile())
        snap = {k: v.clone() for k, v in out.items()}
        if first is None:
            first = snap
        else:
            for k in first:
                assert torch.equal(first[k].view(torch.uint8), snap[k].view(torch.uint8)), (call, k, seen)
    assert [s[0] for s in seen[:12]] == [256] * 4 + [128] * 4 + [64] * 4, seen      # four launches each
    assert seen[12] == seen[13] == seen[14], seen                  # then the winner, every time
    ldir, lofs = cal.xyz_lut(True)
    for f in (0, 5, 31):
        fr = src[f % 4]
        for name in ("RANGE", "RANGE2", "REFLECTIVITY", "NEAR_IR", "FLAGS", "WINDOW"):
            assert np.array_equal(_np(first[name][f]), fr.plane(name)), (f, name)
        assert np.array_equal(_np(first["destaggered:RANGE2"][f]),
                              O.destagger(fr.plane("RANGE2"), cal.pixel_shift_by_row))
        want = O.cartesian(fr.plane("RANGE"), ldir, lofs)
        assert np.abs(_np(first["xyz:RANGE"][f]).astype(np.float64) - want).max() <= 4e-5


def test_df_sensor_per_pixel_angles(oracle):
    """make_xyz_lut's DF branch (xyzlut.cpp:49-59): azimuth / altitude given per PIXEL (w*h entries,
    encoder angle 0, no sign flip).  The C ABI keeps a full LUT for it; decode + cartesian must match
    the oracle's LUT."""
    O = oracle
    h, w = 32, 512
    g = np.random.default_rng(8)
    az = g.uniform(-60, 60, h * w)
    alt = g.uniform(-25, 25, h * w)
    b2l = np.eye(4); b2l[0, 3] = 12.5; b2l[2, 3] = 3.0   # z offset: n = sqrt(x^2 + z^2)
    tf = np.array([[0, -1, 0, 10.0], [1, 0, 0, -4.0], [0, 0, 1, 36.18], [0, 0, 0, 1]])
    ldir, lofs = O.make_xyz_lut(w, h, 0.001, b2l, tf, az, alt)
    a, e = np.deg2rad(az), np.deg2rad(alt)                # closed form of the branch
    n = np.hypot(12.5, 3.0)
    d = np.stack([np.cos(a) * np.cos(e), np.sin(a) * np.cos(e), np.sin(e)], 1)
    o = np.stack([12.5 - d[:, 0] * n, -d[:, 1] * n, -d[:, 2] * n + 3.0], 1)
    assert np.abs(ldir - d @ tf[:3, :3].T * 0.001).max() < 1e-15
    assert np.abs(lofs - (o @ tf[:3, :3].T + tf[:3, 3]) * 0.001).max() < 1e-12
    hp = HotPath("RNG15_RFL8_NIR8", h, w, 16)
    lut = hp.add_lut(b2l, tf, az, alt)
    ed, eo = lut.export(w, h)
    assert np.abs(ed - ldir).max() < 1e-15 and np.abs(eo - lofs).max() < 1e-12
    r = g.integers(0, 2 ** 18, size=(2, h, w)).astype(np.uint32)
    r[g.random(r.shape) < 0.3] = 0
    want = np.stack([O.cartesian(r[k], ldir, lofs) for k in range(2)])
    got = _np(hp.cartesian(torch.from_numpy(r).cuda(), dtype=torch.float64))
    assert np.abs(got - want).max() < 1e-9                # full f64 LUT built by the library (equal to the
                                                          # oracle's to 1e-15), the reference's own r*dir+ofs
    # and through the fused decode kernel
    cal = O.synthetic_calib(h=h, w=w, profile="RNG15_RFL8_NIR8")
    packets, src = O.synth_packets(cal, 2, with_window=True)
    out = hp.alloc_outputs(2, xyz=["RANGE"], xyz_dtype=torch.float64)
    hp.decode(torch.from_numpy(packets).cuda(), out)
    for f in range(2):
        assert np.abs(_np(out["xyz:RANGE"][f]) - O.cartesian(src[f].plane("RANGE"), ldir, lofs)).max() < 1e-9
    with pytest.raises(ValueError, match="unexpected frame dimensions"):
        hp.add_lut(b2l, tf, az[:-1], alt[:-1])


@pytest.mark.parametrize("profile,hdr", [("RNG15_RFL8_NIR8_DUAL", 0), ("FUSA_RNG15_RFL8_NIR8_DUAL", 1), ("LEGACY", 0)])
def test_packet_level_outputs(oracle, profile, hdr):
    """packet_timestamp / alert_flags (written per packet slot, valid columns or not,
    lidar_frame.cpp:1534-1539) and the frame-level values latched from the first packet
    (start_frame, :1709-1741), through the C ABI with device host_timestamps."""
    O = oracle
    h, w, cpp = 32, 512, 16
    cal = O.synthetic_calib(h=h, w=w, cpp=cpp, profile=profile, header_type=hdr)
    pf = cal.packet_format()
    g = np.random.default_rng(13)
    n = 3
    frames, packets = [], []
    for f in range(n):
        fr = O.Frame.for_profile(cal.profile, h, w, cpp, with_window=True)
        O.randomize_frame(fr, pf, 50 + f, frame_id=800 + f)
        if profile != "LEGACY":
            fr.alert_flags[:] = g.integers(0, 256, fr.alert_flags.shape).astype(np.uint8)
            fr.s.frame_status = int(g.integers(0, 4)) | (int(g.integers(0, 4)) << 4)
            fr.s.shutdown_countdown = int(g.integers(0, 200))
            fr.s.shot_limiting_countdown = int(g.integers(0, 200))
        pk, _ = O.frame_to_packets(fr, pf, cal.init_id & 0xFFFFFF, cal.prod_sn)
        frames.append(fr)
        packets.append(pk.copy())
    ppf = w // cpp
    packets[1] = np.delete(packets[1], 7, axis=0)                 # a packet that never arrived
    if profile != "LEGACY":
        for c in range(cpp):                                      # a packet whose columns are all invalid
            packets[2][4, pf.packet_header_size + c * pf.col_size + 10] &= 0xFE
    host = np.zeros((n, ppf, pf.lidar_packet_size), np.uint8)
    counts = np.zeros(n, np.uint32)
    hts = np.zeros((n, ppf), np.uint64)
    for f in range(n):
        host[f, :len(packets[f])] = packets[f]
        counts[f] = len(packets[f])
        hts[f, :len(packets[f])] = 1000 * (f + 1) + np.arange(len(packets[f]))
    hp = HotPath(profile, h, w, cpp, header_type=hdr)
    out = hp.alloc_outputs(n)
    out["packet_timestamp"] = torch.full((n, ppf), 7, dtype=torch.int64, device="cuda").to(torch.uint64)
    out["alert_flags"] = torch.zeros((n, ppf), dtype=torch.uint8, device="cuda")
    hp.decode(torch.from_numpy(host).cuda(), out, packet_counts=counts,
              host_timestamps=torch.from_numpy(hts).cuda())
    hp.sync()
    meta = _np(out["frame_meta"]).reshape(n, 24)
    for f in range(n):
        ref = O.Frame.for_profile(cal.profile, h, w, cpp, with_window=True)
        ref.fill(0)
        b = O.Batcher(pf, init_id=cal.init_id & 0xFFFFFF, expected_packets=len(packets[f]))
        for i, p in enumerate(packets[f]):
            b.batch(p, int(hts[f, i]), ref)
        if len(packets[f]) < ppf:
            b.finalize(ref)
        assert np.array_equal(_np(out["packet_timestamp"][f]), ref.packet_timestamp), f
        assert np.array_equal(_np(out["alert_flags"][f]), ref.alert_flags), f
        assert np.array_equal(_np(out["status"][f]), ref.status), f
        assert meta[f, :8].view(np.int64)[0] == ref.frame_id == 800 + f
        assert meta[f, 8:16].view(np.uint64)[0] == ref.s.frame_status
        assert meta[f, 16:18].view(np.uint16)[0] == ref.s.shutdown_countdown
        assert meta[f, 18:20].view(np.uint16)[0] == ref.s.shot_limiting_countdown
    assert _np(out["packet_timestamp"][1])[7] == 0 and _np(out["packet_timestamp"][0]).all()
    if profile != "LEGACY":
        assert _np(out["packet_timestamp"][2])[4] == 3004 and not _np(out["status"][2])[64:80].any()


@pytest.mark.parametrize("seed", range(16))
def test_tile_variants_agree_on_random_geometries(oracle, monkeypatch, seed):
    """Random (profile, H, W, columns per packet): the 64-column kernel and the 128 / 256-column wide
    kernels must produce identical bytes for every output, and those bytes must be the oracle's."""
    O = oracle
    g = np.random.default_rng(1000 + seed)
    profile = ["RNG15_RFL8_NIR8_DUAL", "RNG19_RFL8_SIG16_NIR16", "RNG15_RFL8_NIR8", "LEGACY",
               "RNG19_RFL8_SIG16_NIR16_DUAL", "FIVE_WORD_PIXEL"][seed % 6]
    cpp = int(g.choice([4, 8, 16]))
    h = int(g.integers(3, 131))
    w = cpp * int(g.integers(256 // cpp, 1300 // cpp))
    cal = O.synthetic_calib(h=h, w=w, cpp=cpp, profile=profile)
    pf = cal.packet_format()
    n = 3
    packets, src = O.synth_packets(cal, n, with_window=True)
    by_frame = [packets[f] for f in range(n)]
    by_frame[1] = np.delete(by_frame[1], [int(g.integers(0, len(by_frame[1])))], axis=0)
    by_frame[2] = by_frame[2][g.permutation(len(by_frame[2]))]
    slots = w // cpp
    host = np.zeros((n, slots, pf.lidar_packet_size), np.uint8)
    counts = np.zeros(n, np.uint32)
    for f, pk in enumerate(by_frame):
        host[f, :len(pk)] = pk
        counts[f] = len(pk)
    dev = torch.from_numpy(host).cuda()
    monkeypatch.setenv("OUSTER_HIP_WIDE_MIN_BLOCKS", "0")
    results = {}
    for variant in ("0", "128", "256"):
        monkeypatch.setenv("OUSTER_HIP_WIDE", variant)
        hp = HotPath(profile, h, w, cpp)
        hp.set_pixel_shift_by_row(cal.pixel_shift_by_row)
        hp.add_lut(cal.beam_to_lidar, cal.lut_transform(True), cal.beam_azimuth_angles, cal.beam_altitude_angles)
        names = [x for x, _ in hp.fields]
        xyz = [x for x in ("RANGE", "RANGE2") if x in names]
        out = hp.alloc_outputs(n, destagger=[x for x in ("RANGE", "REFLECTIVITY") if x in names], xyz=xyz)
        for t in out.values():
            t.view(torch.uint8).fill_(0x5C)
        hp.decode(dev, out, packet_counts=counts)
        hp.sync()
        tc, _ = hp.ctx.last_decode_tile()
        assert (tc <= 64) == (variant == "0") or w < int(variant), (variant, tc)
        results[variant] = {k: v.cpu().numpy().copy() for k, v in out.items() if k != "frame_meta"}
    for variant in ("128", "256"):
        for k, v in results["0"].items():
            assert np.array_equal(v.view(np.uint8), results[variant][k].view(np.uint8)), (variant, k, profile, h, w, cpp)
    ref = _oracle_frames(O, cal, pf, by_frame, True)
    for f, fr in enumerate(ref):
        for name in names:
            assert np.array_equal(results["256"][name][f], fr.plane(name)), (f, name)
        assert np.array_equal(results["256"]["status"][f], fr.status)
