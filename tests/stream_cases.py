"""The cases the tests of hip::FrameStream share (tests/test_stream_cases_cpu.py, tests/test_gpu_frame_stream.py): no test in here,
numpy and the oracle only.  Two small sensors -- make_info(16, 128, variant, wrap_shifts = false, mounted = true) of
tests/cpp/batch_fixture.h, restated below -- 12 frames each, a table of scenarios that tests/cpp/stream_tool.cpp mirrors by name,
the writer of the packets.bin the tool reads, and want(O, name): what the oracle says every delivered batch must hold.

The frames (KINDS): ranges come from scene(), a wall between 1.6 m and 5.6 m, so every ranged pixel lies inside the gate
G = (1.5 m, 6.0 m) and `keep` alone sets a frame's point count; "far" frames stand 10 m further out (outside G, outside 50 - 60 m,
inside 0 - 1e9 m).  Frame 5 is pushed without its packet 2; frames 2 and 3 have every pixel ranged and every column valid."""
import collections

import numpy as np

H, W, CPP = 16, 128, 16
PPF = W // CPP
N_FRAMES = 12
PROFILE = "RNG15_RFL8_NIR8_DUAL"
INIT_ID = 0x123456
G = (1.5, 6.0)
T0_NS = 1_700_000_123_000_000_000
FRAME_NS, COL_NS = 100_000_000, 100_000_000 // W
MISSING_FRAME, MISSING_PACKET = 5, 2          # every scenario pushes frame 5 of either sensor without its packet 2
LOST_FRAME, LOST_PACKET = 2, 5                # `packets` alone: frame 2 loses packet 5 as well
FAR_MM = 10_000
# frame -> (kind, share of the pixels that carry a range)
KINDS = [("dense", 0.90), ("dense", 0.88), ("full", 1.0), ("full", 1.0), ("dense", 0.95), ("dense", 0.60),
         ("far", 0.9), ("far", 0.9), ("far", 0.9), ("dense", 0.70), ("dense", 0.80), ("dense", 0.75)]
F32_POINT_BAR, F64_POINT_BAR = 1e-4, 1e-9     # tests/test_gpu_dewarp_frames.py::FORMS rows32 / sep64
F32_CLOUD_BAR, F64_CLOUD_BAR = 4e-5, 1e-9     # tests/test_gpu_parity.py

Scenario = collections.namedtuple(
    "Scenario", "name sensors fpb in_flight f64 gate provenance xyz planes destaggered headers keep_planes n_frames finish_after "
                "by_packet")


def _sc(name, fpb, in_flight, n_frames, sensors=1, f64=False, gate=G, provenance=True, xyz=False, planes=(), destaggered=(),
        headers=True, keep_planes=(), finish_after=0, by_packet=False):
    return Scenario(name, sensors, fpb, in_flight, f64, gate, provenance, xyz, tuple(planes), tuple(destaggered), headers,
                    tuple(keep_planes), n_frames, finish_after, by_packet)


INVARIANCE = [(1, 1), (2, 2), (3, 2), (4, 3), (11, 2), (16, 2)]    # (fpb, in flight) the frames of `laps` also go through
_LAPS = dict(n_frames=11, planes=("RANGE",))
SCENARIOS = {s.name: s for s in [
    _sc("laps", 2, 2, 11, xyz=True, planes=("RANGE", "REFLECTIVITY2"), destaggered=("RANGE",)),
    _sc("one_in_flight", 3, 1, 7),
    _sc("f64_three", 1, 3, 7, f64=True, provenance=False, xyz=True),
    _sc("two_sensors", 4, 2, 10, sensors=2, planes=("RANGE",)),
    _sc("at_capacity", 2, 2, 8, gate=(0.0, 1e9)),
    _sc("nothing_kept", 3, 2, 8, gate=(50.0, 60.0)),
    _sc("empty_gate", 2, 2, 5, gate=(0.0011, 0.0019)),
    _sc("finish_midway", 4, 2, 9, finish_after=3),
    _sc("packets", 2, 2, 6, by_packet=True, planes=("RANGE",)),
    _sc("dense_only", 4, 2, 6, gate=None, provenance=False, xyz=True, planes=("RANGE", "REFLECTIVITY"),
        keep_planes=("RANGE", "REFLECTIVITY")),
    _sc("range_added", 2, 2, 11, planes=("REFLECTIVITY",), keep_planes=("REFLECTIVITY",)),
] + [_sc("laps_%dx%d" % fi, fi[0], fi[1], **_LAPS) for fi in INVARIANCE]}


# -- the sensors -------------------------------------------------------------------------------------------------------
def shifts():
    """pixel_shift_by_row of make_info(H, W, variant): both variants share them"""
    return [int(np.rint([4.2, 1.4, -1.4, -4.2][i % 4] / 360.0 * W)) for i in range(H)]


def sensor(O, variant):
    """make_info(H, W, variant, false, true) as the oracle's calibration: an OS-2 beam origin, the beams tilted by 0.7 degrees
    per variant, a sensor_to_body that turns about z by 0.3 + 0.4 * variant rad and has its own offset (metres)"""
    cal = O.synthetic_calib(h=H, w=W, cpp=CPP, profile=PROFILE, b2l_x=13.762)
    cal.beam_azimuth_angles = np.array([[4.2, 1.4, -1.4, -4.2][i % 4] for i in range(H)])
    cal.beam_altitude_angles = np.array([21.0 - 42.0 * i / (H - 1.0) + 0.7 * variant for i in range(H)])
    cal.pixel_shift_by_row = np.array(shifts(), dtype=np.int32)
    a = 0.3 + 0.4 * variant
    ext = np.eye(4)
    ext[0, :2] = np.cos(a), -np.sin(a)
    ext[1, :2] = np.sin(a), np.cos(a)
    ext[:3, 3] = 0.35 - 0.6 * variant, -0.2 + 0.15 * variant, 1.1 + 0.25 * variant
    cal.extrinsic = ext
    cal.init_id = INIT_ID
    return cal


_LUTS = {}


def lut(O, variant, T):
    """(direction, offset) [H * W, 3] of sensor `variant`, extrinsics folded in: oracle.make_xyz_lut, cast to T like XYZLutT<T>"""
    key = (variant, np.dtype(T).name)
    if key not in _LUTS:
        d, o = sensor(O, variant).xyz_lut(True)
        _LUTS[key] = (d.astype(T), o.astype(T))
        for a in _LUTS[key]:
            a.setflags(write=False)
    return _LUTS[key]


# -- the frames --------------------------------------------------------------------------------------------------------
def scene(f, keep, far=False):
    """RANGE / RANGE2 of frame f, (H, W) mm in multiples of 8 (the profile's range unit): the wall of tests/batch_cases.py, first
    return 1.6 - 5.6 m, the second 0.3 - 0.75 m behind it; `far` moves both 10 m out; zero where `keep` is false"""
    u, v = np.mgrid[0:H, 0:W]
    r1 = 2500.0 + 900.0 * np.sin(2 * np.pi * (v + 7 * f) / W) + 60.0 * u + np.where((v + 5 * f) % W < W // 4, 1200.0, 0.0)
    r2 = r1 + 296.0 + 64.0 * ((u + v + f) % 8)
    add = FAR_MM if far else 0
    r1 = (r1.astype(np.int64) // 8 * 8 + add).astype(np.uint32)
    r2 = (r2.astype(np.int64) // 8 * 8 + add).astype(np.uint32)
    return np.where(keep, r1, 0).astype(np.uint32), np.where(keep, r2, 0).astype(np.uint32)


_PACKETS = {}


def frame_packets(O, variant):
    """[N_FRAMES, PPF, lidar_packet_size] u8: the complete frames of one sensor (what is lost is lost when they are pushed)"""
    if variant not in _PACKETS:
        cal = sensor(O, variant)
        pf = cal.packet_format()
        out = []
        for f, (kind, share) in enumerate(KINDS):
            fr = O.Frame.for_profile(cal.profile, H, W, CPP, with_window=cal.with_window)
            O.randomize_frame(fr, pf, 9000 + 100 * variant + f, 0.0, frame_id=700 + f)
            keep = np.random.default_rng(31 * f + variant).random((H, W)) < share
            r1, r2 = scene(f + N_FRAMES * variant, keep, far=kind == "far")
            fr.plane("RANGE")[:] = r1
            fr.plane("RANGE2")[:] = r2
            fr.timestamp[:] = T0_NS + f * FRAME_NS + np.arange(W, dtype=np.uint64) * np.uint64(COL_NS)
            pk, _ = O.frame_to_packets(fr, pf, INIT_ID, cal.prod_sn)
            assert pk.shape[0] == PPF
            out.append(pk.copy())
        _PACKETS[variant] = np.ascontiguousarray(np.stack(out))
        _PACKETS[variant].setflags(write=False)
    return _PACKETS[variant]


def write_packets(O, path):
    """packets.bin of stream_tool: [2 sensors][N_FRAMES][PPF][lidar_packet_size] bytes"""
    np.ascontiguousarray(np.stack([frame_packets(O, 0), frame_packets(O, 1)])).tofile(path)


def pushed_frames(O, sc):
    """the frames of a scenario in push order: (sensor, packets [k, size]) with the lost packets left out -- frame i of the
    stream is frame i // sensors of sensor i % sensors"""
    out = []
    for i in range(sc.n_frames):
        s, f = i % sc.sensors, i // sc.sensors
        lost = [MISSING_PACKET] if f == MISSING_FRAME else []
        if sc.by_packet and f == LOST_FRAME:
            lost.append(LOST_PACKET)
        out.append((s, np.delete(frame_packets(O, s)[f], lost, axis=0)))
    return out


def packet_sequence(O, sc):
    """push_packet's input: the pushed frames' packets end to end, the last packet of frame 0 swapped with the first of frame 1"""
    seq = [p for _, pk in pushed_frames(O, sc) for p in pk]
    seq[PPF - 1], seq[PPF] = seq[PPF], seq[PPF - 1]
    return seq


def _snapshot(fr):
    d = {name: fr.plane(name).copy() for name in fr.plane_names()}
    d.update(timestamp=fr.timestamp.copy(), measurement_id=fr.measurement_id.copy(), status=fr.status.copy())
    return d


def decoded_frames(O, sc):
    """[(sensor, {plane or header name: array})] of the frames the stream sends to the GPU, from oracle.Batcher on exactly the
    packets pushed: per frame for push_frame, the whole sequence through one batcher for push_packet"""
    cal = sensor(O, 0)
    pf = cal.packet_format()
    new = lambda: O.Frame.for_profile(cal.profile, H, W, CPP, with_window=cal.with_window)
    out = []
    if sc.by_packet:
        b, fr = O.Batcher(pf, init_id=INIT_ID), new()
        for p in packet_sequence(O, sc):
            if b.batch(p, 77, fr):
                out.append((0, _snapshot(fr)))
        return out
    for s, pk in pushed_frames(O, sc):
        fr = new()
        fr.fill(0xAB)   # stale content must be overwritten or zeroed
        b = O.Batcher(pf, init_id=INIT_ID, expected_packets=len(pk))
        done = False
        for i, p in enumerate(pk):
            done = b.batch(p, 1 + i, fr)
        if not done:
            b.finalize(fr)
        out.append((s, _snapshot(fr)))
    return out


def batch_spans(sc, n_released):
    """[(first_frame, n_frames)] of the batches a stream delivers: full ones, a partial one at every finish()"""
    spans, first = [], 0
    stops = ([sc.finish_after] if sc.finish_after else []) + [n_released]
    for stop in stops:
        while first < stop:
            n = min(sc.fpb, stop - first)
            spans.append((first, n))
            first += n
    return spans


def frame_points(O, sc, sensor_idx, fr, gate=None, lut_of=None):
    """oracle.dewarp_frame of one decoded frame on identity poses -> (points, col_idxs, timestamps); lut_of: the sensor whose
    LUT is used instead of the frame's own (the CPU preconditions ask what a swapped LUT would give)"""
    T = np.float64 if sc.f64 else np.float32
    d, o = lut(O, sensor_idx if lut_of is None else lut_of, T)
    poses = np.tile(np.eye(4), (W, 1, 1))
    lo, hi = sc.gate if gate is None else gate
    return O.dewarp_frame(fr["RANGE"], fr["status"], fr["timestamp"], poses, d, o, lo, hi)


_WANT = {}


def want(O, name):
    """What every delivered batch of scenario `name` must hold, in delivery order: a list of dicts with first_frame, n_frames,
    planes / destaggered {name: [n_frames, H, W]}, xyz [2] of [n_frames, H * W, 3] (None where not downloaded), timestamp /
    measurement_id / status [n_frames, W], and on the compacting route frame_offsets [fpb + 1] u64, n_points, points
    [n_points, 3], point_col_idxs, point_timestamps_ns, point_frame_idxs (the index within the batch).  Computed once."""
    if name in _WANT:
        return _WANT[name]
    sc = SCENARIOS[name]
    T = np.float64 if sc.f64 else np.float32
    frames = decoded_frames(O, sc)
    sh = shifts()
    batches = []
    for first, n in batch_spans(sc, len(frames)):
        part = frames[first:first + n]
        b = dict(first_frame=first, n_frames=n, planes={}, destaggered={}, xyz=[None, None])
        for p in sc.planes:
            b["planes"][p] = np.stack([fr[p] for _, fr in part])
        for p in sc.destaggered:
            b["destaggered"][p] = np.stack([O.destagger(fr[p], sh) for _, fr in part])    # the FIRST sensor's shifts
        if sc.xyz:
            for k, rname in enumerate(("RANGE", "RANGE2")):
                b["xyz"][k] = np.stack([O.cartesian(fr[rname], *lut(O, s, T)) for s, fr in part])
        for hname in ("timestamp", "measurement_id", "status"):
            b[hname] = np.stack([fr[hname] for _, fr in part]) if sc.headers else None
        if sc.gate is not None:
            per = [frame_points(O, sc, s, fr) for s, fr in part]
            counts = [len(x[0]) for x in per] + [0] * (sc.fpb - n)     # the unused frames of a partial batch add nothing
            b["frame_offsets"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
            b["n_points"] = int(b["frame_offsets"][-1])
            b["points"] = np.concatenate([x[0] for x in per]).reshape(-1, 3).astype(T)
            b["point_col_idxs"] = np.concatenate([x[1] for x in per]).astype(np.uint32)
            b["point_timestamps_ns"] = np.concatenate([x[2] for x in per]).astype(np.uint64)
            b["point_frame_idxs"] = np.concatenate([np.full(len(x[0]), i, np.uint32) for i, x in enumerate(per)])
        for v in list(b.values()) + list(b["planes"].values()) + list(b["destaggered"].values()) + b["xyz"]:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        batches.append(b)
    _WANT[name] = batches
    return batches
