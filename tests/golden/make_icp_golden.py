#!/usr/bin/env python3
"""Regenerates tests/golden/icp_voxels.npz: the voxel rows with unit normals of the first frame of the golden capture
OS-0-128-U1_v2.3.0_1024x10.pcap, the source cloud of the realistic ICP tests (tests/test_gpu_icp.py, tests/test_icp_model.py).

Everything runs on the CPU through the models the GPU code is held to: the packet oracle decodes and destaggers the frame and
computes its cloud, tests/normals_model.py its normals, tests/voxel_model.py the voxel rows (voxel 1 m).  Takes a few seconds."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
NAME = "OS-0-128-U1_v2.3.0_1024x10"
VOXEL = 1.0


def main():
    from oracle import oracle as O
    import normals_model as N
    import voxel_model as V
    cal = O.calib_from_json(os.path.join(HERE, "pcaps", NAME + ".json"))
    pf = cal.packet_format()
    pk = O.lidar_packets_from_pcap(os.path.join(HERE, "pcaps", NAME + ".pcap"), pf)
    fids = [O.lib().ora_frame_id(C.byref(pf), p.ctypes.data) for p in pk]
    counts = {f: fids.count(f) for f in set(fids)}
    fid = max(sorted(counts), key=lambda f: counts[f])     # the first complete frame
    sel = [i for i, x in enumerate(fids) if x == fid]
    fr = O.Frame.for_profile(cal.profile, cal.h, cal.w, cal.cpp, with_window=False)
    fr.fill(0)
    b = O.Batcher(pf, init_id=O.lib().ora_init_id(C.byref(pf), pk[sel[0]].ctypes.data), expected_packets=len(sel))
    done = False
    for i in sel:
        done = b.batch(pk[i], 1 + i, fr)
    if not done:
        b.finalize(fr)
    ldir, lofs = cal.xyz_lut(False)
    rng = O.destagger(fr.plane("RANGE"), cal.pixel_shift_by_row)
    xyz = O.cartesian(fr.plane("RANGE"), ldir, lofs).reshape(cal.h, cal.w, 3)
    xyz = np.stack([O.destagger(np.ascontiguousarray(xyz[:, :, k]), cal.pixel_shift_by_row) for k in range(3)], axis=2)
    nrm = N.normals(xyz.reshape(-1, 3), rng, sensor_origins_xyz=np.zeros((cal.w, 3)))
    keep = (rng.reshape(-1) != 0) & np.isfinite(nrm).all(axis=1) & (np.abs(nrm).sum(axis=1) > 0)
    pts, nrm = V.voxel_downsample_with_normals(xyz.reshape(-1, 3)[keep], nrm[keep], VOXEL)
    print("%d packets of frame %d, %d points with a normal, %d voxel rows" % (len(sel), fid, int(keep.sum()), len(pts)))
    np.savez_compressed(os.path.join(HERE, "icp_voxels.npz"), points=pts, normals=nrm, voxel_size=np.float64(VOXEL))


if __name__ == "__main__":
    main()
