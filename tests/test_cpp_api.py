"""Runs the C++ test executable of the host API mirror (tests/cpp/test_core_api.cpp) on the
GPU box: PacketFormat / LidarFrame / FrameBatcher / destagger / XYZLut with the reference's
names, every per-pixel result produced by the HIP kernels."""
import os
import subprocess

import pytest

import cpp_tools

pytestmark = pytest.mark.gpu


def test_cpp_core_api():
    exe, env = cpp_tools.build("test_core_api")  # g++ only, incremental
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    print(p.stdout[-4000:])
    print(p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-1000:]
    assert "0 failed" in p.stdout


@pytest.mark.parametrize("switch", ["off", "on"])
def test_eigen_boundary_switch_compiles_and_runs(switch):
    """include/ouster/core/typedefs.h with and without -DOUSTER_HIP_USE_EIGEN: the reference-style
    snippet (Field -> image -> destagger -> cartesian) builds and gives the same answers both ways.
    (Eigen3 is mocked by tests/cpp/mock_eigen: it is not installed in this image.)"""
    exe, env = cpp_tools.build("eigen_switch_" + switch)
    p =subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "0 mismatches" in p.stdout, p.stdout + p.stderr[-2000:]


def test_reference_snapshot_hashes_through_cpp_mirror(oracle):
    """The reference's FrameBatcherSnapshotTest goldens (tests/frame_batcher_test.cpp:553-595),
    reproduced by the C++ mirror: PcapReader -> FrameBatcher (GPU decode) -> matrix_hash."""
    import json
    from conftest import GOLDEN, PCAPS
    O = oracle
    exe, env = cpp_tools.build("snapshot_tool")
    snaps = json.load(open(os.path.join(GOLDEN, "snapshot_hashes.json")))
    names = {v: k for k, v in O.PROFILES.items()}
    assert len(snaps) == 5
    for base, fields in snaps.items():
        cal = O.calib_from_json(os.path.join(PCAPS, base + ".json"))
        args = [exe, os.path.join(PCAPS, base + ".pcap"), names[cal.profile], str(cal.header_type),
                str(cal.h), str(cal.w), str(cal.cpp), str(cal.init_id), "v2.0.0"]
        p = subprocess.run(args, capture_output=True, text=True, env=env, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        got = {}
        for line in p.stdout.splitlines()[1:]:
            k, v = line.split()
            got[k] = int(v)
        for name, want in fields.items():
            assert got.get(name) == want, (base, name, p.stdout)
        # the same capture through the streaming pipeline (FrameStream::push_packet)
        p = subprocess.run(args + ["stream"], capture_output=True, text=True, env=env, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = p.stdout.splitlines()
        if lines[0] == "stream frames 0":      # the 8-packet FUSA capture never completes a frame
            assert "FUSA" in names[cal.profile]
            continue
        got = {k: int(v) for k, v in (ln.split() for ln in lines[1:])}
        for name, want in fields.items():
            assert got.get(name) == want, (base, name, "stream", p.stdout)
