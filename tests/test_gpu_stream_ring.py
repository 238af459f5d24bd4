"""GPU: the tile ring of the persistent decode kernel (k_decode_stream2, knob stream_slots) against the CPU oracle.

The kernel is forced by knob and its ring depth with it; outputs are pre-filled.  Planes, destaggered planes and column headers
must equal the oracle's, xyz within 1e-4 m.  The oracle runs once per profile on a pool of POOL distinct frames (POOL and the
eight XCDs are coprime, so every XCD sees every pool frame); batch frame f carries pool frame f % POOL and is compared on the GPU.

Shapes: 256 x 32 frames of 16-column packets -- one 256-column tile or two 128-column ones, 16 or 32 workgroups per XCD -- so that
a handful of frames gives workgroups with no tile, one tile, fewer tiles than ring slots and XCDs with unequal item counts; the
frame count that gives every workgroup exactly 2 * nslot + 1 tiles wraps the ring twice and ends inside it.

What fits: a 12 B/px context of 128 x 16 is 31 KB (five slots), of 256 x 8 34 KB (four); six slots fit only the 8 B/px profile's
256 x 8 tiles, so depth 6 runs there and is REFUSED for the 12 B/px profile (the call then takes another kernel)."""
import numpy as np
import pytest

from conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch

from test_gpu_fastpath import _compare, _hotpath  # noqa: E402
from test_gpu_parity import _oracle_frames  # noqa: E402

SINGLE, DUAL, LB, LEGACY = "RNG19_RFL8_SIG16_NIR16", "RNG15_RFL8_NIR8_DUAL", "RNG15_RFL8_NIR8", "LEGACY"
POOL = 7
_pools = {}


def _pool(O, profile, h, w, pool=POOL):
    """(cal, pf, packets [pool, slots, stride], oracle frames, expected outputs on the GPU), computed once per shape"""
    key = (profile, h, w, pool)
    if key in _pools:
        return _pools[key]
    cal = O.synthetic_calib(h=h, w=w, profile=profile)
    pf = cal.packet_format()
    packets, _ = O.synth_packets(cal, pool, with_window=True)
    pad = 16 if profile == LEGACY else 0   # no packet footer: the last 16 B cell needs room behind the last column
    host = np.zeros((pool, w // cal.cpp, pf.lidar_packet_size + pad), np.uint8)
    host[:, :, :pf.lidar_packet_size] = packets
    ref = _oracle_frames(O, cal, pf, [packets[f] for f in range(pool)], True)
    _pools[key] = (cal, pf, host, ref)
    return _pools[key]


def _expected(O, cal, hp, ref, dst, xyz, out):
    """the oracle's outputs of the pool frames as CUDA tensors, name -> [pool, bytes of a frame] (xyz: [pool, values], f64)"""
    ldir, lofs = cal.xyz_lut(False)
    exp = {}
    for n, _ in hp.fields:
        exp[n] = np.stack([fr.plane(n) for fr in ref])
    exp["timestamp"] = np.stack([fr.timestamp for fr in ref])
    exp["measurement_id"] = np.stack([fr.measurement_id for fr in ref])
    exp["status"] = np.stack([fr.status for fr in ref])
    for n in dst:
        exp["destaggered:" + n] = np.stack([O.destagger(fr.plane(n), cal.pixel_shift_by_row) for fr in ref])
    for n in xyz:
        exp["xyz:" + n] = np.stack([O.cartesian(fr.plane(n), ldir, lofs) for fr in ref])
    dev = {}
    for k, v in exp.items():
        if k.startswith("xyz:"):
            dev[k] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64).reshape(len(ref), -1)).cuda()
            continue
        dt = np.dtype(str(out[k].dtype).split(".")[1])   # the output's element type: the comparison is of bytes
        assert np.array_equal(v.astype(dt), v), k
        dev[k] = torch.from_numpy(np.ascontiguousarray(v.astype(dt)).view(np.uint8).reshape(len(ref), -1)).cuda()
    return dev


def _outputs_of(hp):
    names = [n for n, _ in hp.fields]
    dst = [n for n in ("RANGE", "REFLECTIVITY") if n in names]
    xyz = [n for n in ("RANGE", "RANGE2") if n in names]
    return dst, xyz


def _decode_and_check(O, profile, h, w, tw, slots, frame_counts, rows=0, expect_ring=True, pool=POOL, loader=None):
    cal, pf, host, ref = _pool(O, profile, h, w, pool)
    hp = _hotpath(cal, profile, wide="s%d" % tw)
    hp.ctx.set_knob("stream_slots", slots)
    if rows:
        hp.ctx.set_knob("stream_rows", rows)
    if loader is not None:
        hp.ctx.set_knob("stream_loader", loader)
    dst, xyz = _outputs_of(hp)
    exp = _expected(O, cal, hp, ref, dst, xyz, hp.alloc_outputs(1, destagger=dst, xyz=xyz))
    d_pool = torch.from_numpy(host).cuda()
    tiles = None
    for n in frame_counts:
        n = n(tiles) if callable(n) else n
        idx = torch.arange(n, device="cuda") % pool
        d_pk = d_pool[idx].contiguous()
        out = hp.alloc_outputs(n, destagger=dst, xyz=xyz)
        for t in out.values():
            t.view(torch.uint8).fill_(0x6B)
        hp.decode(d_pk, out)
        hp.sync()
        kernel, tiles = hp.ctx.last_decode_kernel(), hp.ctx.last_decode_tile()
        if expect_ring:
            assert kernel == "k_decode_stream2" and tiles[0] == tw, (kernel, tiles, n)
            if rows:
                assert tiles[1] == rows
        else:
            assert kernel not in ("k_decode_stream", "k_decode_stream2"), (kernel, tiles)
        for k, want in exp.items():
            got = out[k]
            if k.startswith("xyz:"):
                err = (got.double().reshape(n, -1) - want[idx]).abs().max().item()
                assert err <= 1e-4, (k, n, slots, err)
            else:
                assert torch.equal(got.view(torch.uint8).reshape(n, -1), want[idx]), (k, n, slots)
    return hp


def _wrap_twice(nslot, h, w, tw):
    """frames that give every workgroup exactly 2 * nslot + 1 tiles: 32 / (w / tw) workgroups per XCD and column tile share the
    XCD's (frame, row chunk) items"""
    def frames(tiles):
        nch = h // tiles[1]
        groups = 32 // (w // tw)
        per_xcd = groups * (2 * nslot + 1)
        assert per_xcd % nch == 0
        return 8 * per_xcd // nch
    return frames


COUNTS = [1, 7, 8, 9, 24, 25]


@pytest.mark.parametrize("tw,slots,rows", [(128, 2, 0), (128, 3, 0), (128, 5, 0), (128, 0, 0), (256, 2, 16), (256, 3, 8), (256, 4, 0), (256, 0, 0)])
def test_ring_depths_single_return(oracle, tw, slots, rows):
    """RNG19_RFL8_SIG16_NIR16, 256 x 32: every depth that fits (and the plan's own choice, 0) at 1 .. 25 frames and at
    8 x (2 nslot + 1) frames; then the frame count at which every workgroup walks 2 nslot + 1 tiles."""
    nslot = slots or 2
    _decode_and_check(oracle, SINGLE, 32, 256, tw, slots, COUNTS + [8 * (2 * nslot + 1), _wrap_twice(nslot, 32, 256, tw)], rows=rows)


def test_a_depth_that_does_not_fit_is_refused(oracle):
    """six 12 B/px contexts fit at no tile height: the plan refuses, the call runs on another kernel and is still right"""
    _decode_and_check(oracle, SINGLE, 32, 256, 128, 6, [9], expect_ring=False)


def test_six_slots_on_the_8_byte_profile(oracle):
    _decode_and_check(oracle, LB, 32, 256, 256, 6, [1, 9, 25, 8 * 13, _wrap_twice(6, 32, 256, 256)])


@pytest.mark.parametrize("slots", [2, 3])
def test_dual_return_shares_the_code(oracle, slots):
    _decode_and_check(oracle, DUAL, 32, 256, 256, slots, [1, 9, 25, _wrap_twice(slots, 32, 256, 256)])


@pytest.mark.parametrize("slots", [2, 4])
def test_legacy(oracle, slots):
    _decode_and_check(oracle, LEGACY, 32, 256, 128, slots, [1, 9, 25, _wrap_twice(slots, 32, 256, 128)])


@pytest.mark.parametrize("slots,rows", [(0, 0), (5, 16)])
def test_full_width_single_return(oracle, slots, rows):
    """128 x 2048, nine frames: sixteen column tiles, two workgroups each per XCD, XCD 0 with one frame more than the others"""
    _decode_and_check(oracle, SINGLE, 128, 2048, 128, slots, [9], rows=rows, pool=3)


@pytest.mark.parametrize("slots", [2, 5])
def test_loss_and_strays_behind_the_ring(oracle, slots):
    """a zeroed packet slot (its columns decode as zeros) and a swapped packet pair (the frame is flagged and the fix-up pass
    redoes it behind the ring kernel), in a batch long enough for the ring to turn"""
    O = oracle
    cal, pf, host, _ = _pool(O, SINGLE, 32, 256)
    n = 8 * 16 * 3
    batch = host[np.arange(n) % POOL].copy()
    batch[33, 5] = 0
    batch[70, [10, 11]] = batch[70, [11, 10]]
    by_frame = {33: np.delete(batch[33], [5], axis=0), 70: batch[70], 34: batch[34], 71: batch[71]}
    hp = _hotpath(cal, SINGLE, wide="s128")
    hp.ctx.set_knob("stream_slots", slots)
    dst, xyz = _outputs_of(hp)
    out = hp.alloc_outputs(n, destagger=dst, xyz=xyz)
    for t in out.values():
        t.view(torch.uint8).fill_(0x6B)
    hp.decode(torch.from_numpy(batch).cuda(), out)
    hp.sync()
    assert hp.ctx.last_decode_kernel() == "k_decode_stream2"
    frames = sorted(by_frame)
    ref = _oracle_frames(O, cal, pf, [by_frame[f] for f in frames], True)
    _compare(O, cal, hp, out, ref, dst, xyz, frames=list(zip(frames, ref)))
