"""The case the resident-batch tests of interp_poses, normals and voxel_downsample share (tests/test_gpu_{pose,normals,voxel}_batch.py):
5 dual-return frames of two small sensors, one packet of one frame left out, column timestamps near 1.7e9 s and a trajectory of 9
known poses spanning the 5 frames; written as the packets.bin / known.bin that tests/cpp/batch_fixture.h reads."""
import numpy as np

H, W, N, K = 8, 128, 5, 9
SKIP_FRAME, SKIP_PACKET = 3, 2
T0_NS = 1_700_000_123_000_000_000
FRAME_NS, COL_NS = 100_000_000, 100_000_000 // W
FILTER_LO, FILTER_HI = 3000.0, 3600.0   # mm: filter_field invalidates the ranges INSIDE


def rodrigues(axis, angle):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def trajectory():
    """9 poses 0.06 - 0.08 s apart, from just before the first column to just after the last: relative rotations of 0.05 - 0.4
    rad, positions within 1e3 m (the conditions of the golden maker)"""
    rng = np.random.default_rng(77)
    span = (N - 1) * FRAME_NS + W * COL_NS
    xk = T0_NS * 1e-9 - 0.01 + np.concatenate([[0.0], np.cumsum(rng.uniform(0.06, 0.08, K - 1))])
    assert xk[-1] > (T0_NS + span) * 1e-9
    rot, poses = rodrigues([0.2, -0.3, 1.0], 0.7), []
    for i in range(K):
        if i:
            rot = rot @ rodrigues(rng.normal(size=3), rng.uniform(0.05, 0.4))
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = rot, rng.uniform(-1e3, 1e3, 3)
        poses.append(m.reshape(16))
    return xk, np.array(poses)


def scene(f, keep):
    """RANGE / RANGE2 of frame f, (H, W) mm in multiples of 8 (the profile's range unit): a wall whose distance varies smoothly
    with row and column and steps by 1.2 m at a quarter of the columns, the second return 296 - 744 mm behind the first (both
    sides of the 500 mm thin-object rule); zero where `keep` is false"""
    u, v = np.mgrid[0:H, 0:W]
    r1 = 2500.0 + 900.0 * np.sin(2 * np.pi * (v + 7 * f) / W) + 60.0 * u + np.where((v + 5 * f) % W < W // 4, 1200.0, 0.0)
    r2 = r1 + 296.0 + 64.0 * ((u + v + f) % 8)
    r1 = (r1.astype(np.int64) // 8 * 8).astype(np.uint32)
    r2 = (r2.astype(np.int64) // 8 * 8).astype(np.uint32)
    return np.where(keep, r1, 0).astype(np.uint32), np.where(keep, r2, 0).astype(np.uint32)


def write_packets(oracle, tmp, ranges=None):
    """tmp / "packets.bin": the N frames' packets, random pixels (a tenth of them without range) under the case's timestamps;
    ranges(f, keep) -> (RANGE, RANGE2), e.g. scene, replaces the random ranges where given"""
    O = oracle
    cal = O.synthetic_calib(h=H, w=W, profile="RNG15_RFL8_NIR8_DUAL")
    pf = cal.packet_format()
    packets = []
    for f in range(N):
        fr = O.Frame.for_profile(cal.profile, cal.h, cal.w, cal.cpp, with_window=cal.with_window)
        O.randomize_frame(fr, pf, 4000 + f, 0.1, frame_id=700 + f)
        if ranges is not None:
            r1, r2 = ranges(f, fr.plane("RANGE") != 0)   # a tenth of the pixels stays without range
            fr.plane("RANGE")[:] = r1
            fr.plane("RANGE2")[:] = r2
        fr.timestamp[:] = T0_NS + f * FRAME_NS + np.arange(W, dtype=np.uint64) * np.uint64(COL_NS)
        pk, _ = O.frame_to_packets(fr, pf, cal.init_id & 0xFFFFFF, cal.prod_sn)
        packets.append(pk)
    np.ascontiguousarray(np.stack(packets)).tofile(tmp / "packets.bin")


def write_known(tmp):
    """tmp / "known.bin": the trajectory's K times, then its K poses -> (times, poses)"""
    xk, poses = trajectory()
    with open(tmp / "known.bin", "wb") as fh:
        fh.write(xk.tobytes())
        fh.write(poses.tobytes())
    return xk, poses
