"""The variant tuner's samples in flight (ouster_sdk_amd/csrc/decode_tuner.h; the library's samples are pairs of events): the
knob `retune` in the middle of a measurement starts the measurement over, and a context destroyed with decodes, timed samples
and a standalone call still queued gives back everything it allocated.  Both use the 32-frame 128 x 2048 dual-return batch of
test_gpu_parity.test_variant_tuner_is_transparent, the smallest shape of the suite that gives the tuner a choice."""
import gc

import pytest

from conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from ouster_sdk_amd import _capi as capi
    from ouster_sdk_amd.device import HotPath

N = 32
DST = ["RANGE", "RANGE2", "REFLECTIVITY", "REFLECTIVITY2"]


def _batch(O, **kw):
    cal = O.synthetic_calib(h=128, w=2048, profile="RNG15_RFL8_NIR8_DUAL")
    packets, _ = O.synth_packets(cal, 4, with_window=True)
    hp = HotPath("RNG15_RFL8_NIR8_DUAL", 128, 2048, 16, **kw)
    hp.set_pixel_shift_by_row(cal.pixel_shift_by_row)
    hp.add_lut(cal.beam_to_lidar, cal.lut_transform(True), cal.beam_azimuth_angles, cal.beam_altitude_angles)
    d_pk = torch.from_numpy(packets).cuda().repeat(N // 4, 1, 1).contiguous()
    return hp, d_pk


def _u8(t):
    return t.view(torch.uint8)


def test_retune_with_samples_in_flight(oracle):
    hp, d_pk = _batch(oracle)
    out = hp.alloc_outputs(N, destagger=DST, xyz=["RANGE", "RANGE2"])
    tiles, tuners, first = [], [], None
    differs = torch.zeros(20, dtype=torch.bool, device="cuda")   # per call, filled in on the stream: the host waits for nothing
    for call in range(20):
        if call == 5:
            hp.ctx.set_knob("retune", 1)      # samples 0 .. 4 are queued
        if call == 17:
            hp.sync()                         # all twelve samples of the second measurement have landed
        for t in out.values():
            _u8(t).fill_(0xA5)
        hp.decode(d_pk, out)
        tiles.append(hp.ctx.last_decode_tile()[0])
        tuners.append(hp.ctx.last_decode_tuner())
        if first is None:
            first = {k: v.clone() for k, v in out.items()}
        else:
            for k in first:
                differs[call] |= (_u8(first[k]) != _u8(out[k])).any()
    assert tiles[:5] == [256] * 4 + [128], tiles
    assert tiles[5:17] == [256] * 4 + [128] * 4 + [64] * 4, tiles          # from the start again, four launches each
    assert tiles[17] == tiles[18] == tiles[19] and tiles[17] in (256, 128, 64), tiles   # then one winner
    assert tuners == ["measuring"] * 17 + ["measured"] * 3, tuners
    assert not differs.any().item(), (differs.tolist(), tiles)            # every call's outputs are the first call's
    assert _u8(first["RANGE"]).ne(0xA5).any().item()                       # ... and were written


def test_context_destroyed_with_samples_in_flight_frees_everything(oracle):
    gc.collect()                              # contexts of earlier tests go now, not between the two readings
    torch.cuda.synchronize()
    before = capi.alloc_stats()
    hp, d_pk = _batch(oracle, use_torch_stream=False)   # a context with a stream of its own
    out = hp.alloc_outputs(N, destagger=DST, xyz=["RANGE", "RANGE2"])
    torch.cuda.synchronize()                  # the inputs are there; from here on nothing is waited for
    for _ in range(3):
        hp.decode(d_pk, out)
    assert hp.ctx.last_decode_tuner() == "measuring"
    img = hp.destagger(out["RANGE"])          # a standalone call: its tables exist next to the decode's buffers
    inside = capi.alloc_stats()
    assert inside["device_allocs"] - inside["device_frees"] > before["device_allocs"] - before["device_frees"]
    hp.ctx.close()
    for lut in hp.luts:                       # a LUT owns its tables (they outlive the context that uploaded them)
        hp.ctx.L.ouster_hip_lut_destroy(lut.h)
        lut.h = None
    after = capi.alloc_stats()
    assert after["device_allocs"] - after["device_frees"] == before["device_allocs"] - before["device_frees"], (before, inside, after)
    assert after["pinned_allocs"] - after["pinned_frees"] == before["pinned_allocs"] - before["pinned_frees"], (before, inside, after)
    # ouster_hip_ctx_destroy waited for the stream: what was queued has run
    assert torch.equal(_u8(img), _u8(out["destaggered:RANGE"]))
