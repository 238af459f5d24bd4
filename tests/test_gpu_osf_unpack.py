"""GPU: ouster_hip_osf_unpack (k_osf_unpack, k_osf_png_unfilter of csrc/k_osf.hip) called through the C ABI on planes the
fixtures never hold -- ragged widths, every ZPNG pixel size (1..8 bytes), element sizes that differ from the pixel's, the
stagger-back at widths that are no power of two, the unfilter kernel one pixel either side of its block / ring / band sizes and
at its LDS limit, mixed jobs in one launch behind guard bytes, every rejected argument.

Every expectation is the oracle's: oracle/osf_oracle.py (zpng_unfilter, decode_png_field, decode_field; pinned on the reference's
codec and files by tests/test_oracle_osf.py) and oracle.destagger(..., inverse=True) (the reference's size_t arithmetic, not
np.roll).  Inputs come from the encoder models of the tests (tests/zpng_model.py, _png_with_filters of tests/test_gpu_osf.py).
Nothing is compared with the library itself, and everything is bit for bit."""
import zlib

import numpy as np
import pytest

import zpng_model as M
from conftest import has_gpu
from test_gpu_osf import OO_idat, _png_with_filters
from test_gpu_standalone_routes import _shift_passes

pytestmark = pytest.mark.gpu

GRAY8, GRAY16, RGB8, RGBA8, RGBA16, ZPNG = 1, 2, 3, 4, 5, 6        # OUSTER_HIP_OSF_* of include/ouster_hip.h
FILTERED = 1                                                        # OUSTER_HIP_OSF_FLAG_FILTERED
PNG_KIND = {GRAY8: (8, 0, 1), GRAY16: (16, 0, 2), RGB8: (8, 2, 3), RGBA8: (8, 6, 4), RGBA16: (16, 6, 8)}   # depth, colour, pixel bytes
FIELD_TAG = {1: 1, 2: 2, 4: 3, 8: 4}   # element bytes -> ChanFieldType UINT8 / 16 / 32 / 64
GUARD, PATTERN = 64, 0xA5


def _elem(pb):
    """the smallest element that holds a pixel of pb bytes"""
    return 1 if pb == 1 else 2 if pb == 2 else 4 if pb <= 4 else 8


def _values(px, es):
    """pixel bytes uint8 [h, w, pb] -> [h, w] elements of es bytes: the little-endian value, truncated / zero-extended"""
    v = np.zeros(px.shape[:2], np.uint64)
    for k in range(min(px.shape[2], es)):
        v |= px[..., k].astype(np.uint64) << np.uint64(8 * k)
    return v.astype(np.dtype("<u%d" % es))


class Job:
    """One plane of a call: the bytes `src` holds, how they are encoded, the element size asked for and the plane expected."""

    def __init__(self, src, enc, pb, es, want, flags=0, what=""):
        self.src = np.frombuffer(bytes(src), np.uint8)
        self.enc, self.pb, self.es, self.flags, self.what = enc, pb, es, flags, what
        self.want = np.ascontiguousarray(want)
        assert self.want.dtype.itemsize == es, what


def zpng_job(O, res, h, w, pb, es=None, what=""):
    from oracle import osf_oracle as Z
    es = es or _elem(pb)
    return Job(res, ZPNG, pb, es, _values(Z.zpng_unfilter(res, h, w, pb), es), what=what or f"zpng {pb} B -> u{8 * es}")


def png_job(O, rng, enc, h, w, es, filters=None, shifts=None, what=""):
    """A PNG plane of random, correlated pixels: handed over as pixel bytes (filters None) or as the inflated IDAT stream whose
    row y carries filter type filters[y].  Expected: decode_png_field of the PNG, staggered back by the reference's arithmetic."""
    from oracle import osf_oracle as Z
    depth, colour, pb = PNG_KIND[enc]
    px = rng.integers(0, 256, (h, w * pb), dtype=np.uint8)
    px[:, pb:] = (px[:, pb:] // 8 + px[:, :-pb]).astype(np.uint8)
    blob = _png_with_filters(px, depth, colour, np.zeros(h, int) if filters is None else filters)
    want = Z.decode_png_field(blob, np.dtype("<u%d" % es), h, w)
    if shifts is not None:
        want = O.destagger(want, shifts, inverse=True)
    if filters is None:
        assert np.array_equal(Z.png_pixels(blob)[0], px)
        src = px.tobytes()
    else:
        src = zlib.decompress(OO_idat(blob))
        assert len(src) == h * (w * pb + 1) and [src[y * (w * pb + 1)] for y in range(h)] == [int(f) for f in filters]
    return Job(src, enc, pb, es, want, FILTERED if filters is not None else 0,
               what or f"png {enc} -> u{8 * es}" + (" filtered" if filters is not None else ""))


class Unpacker:
    def __init__(self, capi, ctx, torch):
        self.capi, self.ctx, self.torch, self.L = capi, ctx, torch, ctx.L

    def call(self, jobs, h, w, shifts=None, planes_edit=None, n_planes=None, hw=None):
        """ouster_hip_osf_unpack on `jobs`: every dst lies in ONE allocation filled with PATTERN, GUARD bytes in front of and
        behind each plane.  Returns (rc, [plane bytes as written], whether every byte outside the planes still is PATTERN)."""
        torch = self.torch
        src_off, dst_off, s_at, d_at = [], [], 0, 0
        for j in jobs:
            src_off.append(s_at)
            s_at += (j.src.size + 15) & ~15
            d_at = (d_at + 7) & ~7
            dst_off.append(d_at + GUARD)
            d_at += GUARD + h * w * j.es + GUARD
        src = np.zeros(max(s_at, 16), np.uint8)
        for j, o in zip(jobs, src_off):
            src[o:o + j.src.size] = j.src
        d_src = torch.from_numpy(src).cuda()
        d_dst = torch.full((max(d_at, 16),), PATTERN, dtype=torch.uint8, device="cuda")
        arr = (self.capi.OsfPlane * max(len(jobs), 1))()
        for i, j in enumerate(jobs):
            arr[i].src, arr[i].dst = d_src.data_ptr() + src_off[i], d_dst.data_ptr() + dst_off[i]
            arr[i].encoding, arr[i].src_pixel_bytes, arr[i].dst_elem_size, arr[i].flags = j.enc, j.pb, j.es, j.flags
        if planes_edit:
            planes_edit(arr)
        sh = None if shifts is None else np.ascontiguousarray(shifts, dtype=np.int32)
        torch.cuda.synchronize()
        hh, ww = hw or (h, w)
        rc = self.L.ouster_hip_osf_unpack(self.ctx.h, arr, len(jobs) if n_planes is None else n_planes, hh, ww,
                                          None if sh is None else sh.ctypes.data)
        self.ctx.sync()
        out = d_dst.cpu().numpy()
        outside = np.ones(out.size, bool)
        got = []
        for j, o in zip(jobs, dst_off):
            n = h * w * j.es
            got.append(out[o:o + n].copy())
            outside[o:o + n] = False
        return rc, got, bool((out[outside] == PATTERN).all())

    def check(self, jobs, h, w, shifts=None):
        rc, got, guards = self.call(jobs, h, w, shifts)
        assert rc == self.capi.OK, (rc, self.L.ouster_hip_last_error())
        for j, g in zip(jobs, got):
            g = g.view(j.want.dtype).reshape(h, w)
            if not np.array_equal(g, j.want):
                r, c = np.argwhere(g != j.want)[0]
                lo = max(0, int(c) - 4)
                raise AssertionError(f"{j.what} at {h} x {w}: first difference in row {r}, column {c}; columns {lo}..: "
                                     f"got {g[r, lo:lo + 12].tolist()}, want {j.want[r, lo:lo + 12].tolist()}")
        assert guards, ("bytes outside the planes were written", h, w, [j.what for j in jobs])
        return got


@pytest.fixture(scope="module")
def gpu(oracle):
    import torch
    from ouster_sdk_amd import _capi as capi
    assert has_gpu()
    ctx = capi.Context(0)
    yield Unpacker(capi, ctx, torch), oracle
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------
# a. ZPNG: every pixel size at widths around the wave (64) and the block (256), seg = ceil(w / 256) = 1, 2, 4, 9, 17
# ------------------------------------------------------------------------------------------------------------------
ZPNG_WIDTHS = [1, 3, 63, 64, 65, 255, 256, 257, 511, 1000, 2050, 4100]


@pytest.mark.parametrize("h", [1, 3])
def test_zpng_every_pixel_size_at_ragged_widths(gpu, h):
    """Threads without pixels (w < 256 * seg), a last thread with a partial segment, fewer pixels than one wave, one pixel;
    three rows of different random residuals so that a wrong plane stride or row offset of the planar sizes (3, 4) shows."""
    U, O = gpu
    assert sorted({(w + 255) // 256 for w in ZPNG_WIDTHS}) == [1, 2, 4, 9, 17]
    rng = np.random.default_rng(4100 + h)
    for w in ZPNG_WIDTHS:
        U.check([zpng_job(O, rng.integers(0, 256, h * w * pb, dtype=np.uint8), h, w, pb) for pb in range(1, 9)], h, w)


# ------------------------------------------------------------------------------------------------------------------
# b. carries
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", [255, 0, 1])
def test_zpng_carries_wrap_in_every_thread(gpu, byte):
    """Every residual byte 255: every step and every carry between threads and waves wraps mod 256; 0: nothing moves; 1: the
    value of an interleaved lane at column x is (x + 1) mod 256, so a segment that starts one off reads off the message."""
    U, O = gpu
    h = 2
    for w in (257, 1000, 2050):
        jobs = [zpng_job(O, np.full(h * w * pb, byte, np.uint8), h, w, pb) for pb in (1, 3, 4, 8)]
        if byte == 1:
            assert np.array_equal(jobs[0].want[1], (np.arange(w) + 1).astype(np.uint8))
        U.check(jobs, h, w)


# ------------------------------------------------------------------------------------------------------------------
# c. dst_elem_size != src_pixel_bytes
# ------------------------------------------------------------------------------------------------------------------
def test_zpng_values_are_truncated_or_zero_extended_to_the_element(gpu):
    U, O = gpu
    h, w = 3, 257
    rng = np.random.default_rng(257)
    jobs = []
    for pb in (1, 3, 4, 5, 8):
        res = rng.integers(0, 256, h * w * pb, dtype=np.uint8)
        for es in (1, 2, 4, 8):
            j = zpng_job(O, res, h, w, pb, es, what=f"zpng {pb} B -> u{8 * es}")
            full = zpng_job(O, res, h, w, pb, 8).want
            mask = np.uint64((1 << (8 * es)) - 1) if es < 8 else np.uint64(0xFFFFFFFFFFFFFFFF)
            assert np.array_equal(j.want.astype(np.uint64), full & mask)      # the little-endian value masked to the element
            assert es >= pb or not np.array_equal(j.want.astype(np.uint64), full)
            jobs.append(j)
    U.check(jobs, h, w)


# ------------------------------------------------------------------------------------------------------------------
# d. one launch with mixed jobs, guarded
# ------------------------------------------------------------------------------------------------------------------
def _mixed_jobs(O, rng, h, w, shifts):
    jobs = [zpng_job(O, rng.integers(0, 256, h * w * pb, dtype=np.uint8), h, w, pb, es)
            for pb, es in ((1, 2), (3, 4), (4, 4), (8, 8))]
    natural = {GRAY8: 1, GRAY16: 2, RGB8: 4, RGBA8: 4, RGBA16: 8}
    for i, enc in enumerate(natural):
        filters = np.roll([4, 1, 3, 2, 0, 4, 3], i)[:h] if h <= 7 else rng.integers(0, 5, h)
        jobs.append(png_job(O, rng, enc, h, w, natural[enc], None, shifts))
        jobs.append(png_job(O, rng, enc, h, w, natural[enc], filters, shifts))
    jobs.append(png_job(O, rng, GRAY16, h, w, 4, None, shifts, what="png gray16 -> u32"))
    jobs.append(png_job(O, rng, RGBA8, h, w, 2, np.array([2, 4, 4, 1, 3])[:h] if h <= 5 else rng.integers(0, 5, h), shifts,
                        what="png rgba8 -> u16 filtered"))
    jobs.append(png_job(O, rng, GRAY8, h, w, 8, None, shifts, what="png gray8 -> u64"))
    order = rng.permutation(len(jobs))     # ZPNG, flat and filtered planes interleaved
    return [jobs[i] for i in order]


def test_mixed_jobs_in_one_launch_leave_the_guards_alone(gpu):
    """ZPNG of 1, 3, 4, 8 bytes, flat and filtered PNG of all five kinds, elements wider and narrower than the pixel, in one
    call: every plane right, and none of the 64 bytes in front of and behind each plane touched."""
    U, O = gpu
    h, w = 5, 130
    rng = np.random.default_rng(5130)
    shifts = np.array([0, 7, -3, 129, -130], np.int32)
    jobs = _mixed_jobs(O, rng, h, w, shifts)
    assert {j.enc for j in jobs} == {1, 2, 3, 4, 5, 6} and {j.flags for j in jobs} == {0, 1}
    assert len({(j.pb, j.es) for j in jobs}) >= 9
    U.check(jobs, h, w, shifts)


# ------------------------------------------------------------------------------------------------------------------
# e. PNG stagger-back at any width
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [3, 100, 130, 1000])
def test_png_planes_are_staggered_back_at_any_width(gpu, w):
    """dst[r][(c + off[r]) % w] with off = the offsets of destagger for inverse = true: shifts 0, +-1, +-(w-1), +-w, w+3,
    -(2w+5), where the reference's size_t expression is no roll unless w is a power of two.  ZPNG planes are never shifted."""
    U, O = gpu
    h = 5
    rng = np.random.default_rng(w)
    for shifts in _shift_passes(w, h, seed=w):
        zres = rng.integers(0, 256, h * w * 2, dtype=np.uint8)
        jobs = [png_job(O, rng, GRAY16, h, w, 2, None, shifts), png_job(O, rng, RGBA8, h, w, 4, None, shifts),
                zpng_job(O, zres, h, w, 2)]
        U.check(jobs, h, w, shifts)


# ------------------------------------------------------------------------------------------------------------------
# f. k_osf_png_unfilter one pixel either side of its 64-pixel blocks, 192-pixel ring and 64-row bands
# ------------------------------------------------------------------------------------------------------------------
def _decoder(core, h, w, device_unfilter=True):
    info = core.SensorInfo()
    fmt = core.DataFormat()
    fmt.pixels_per_column, fmt.columns_per_frame, fmt.columns_per_packet = h, w, 1
    fmt.pixel_shift_by_row = [0] * h      # where np.roll (osf_oracle.stagger) is the reference's arithmetic at any width
    fmt.udp_profile_lidar = core.UDPProfileLidar.from_string("RNG19_RFL8_SIG16_NIR16")
    info.format = fmt
    dec = core.OsfFrameDecoder(info)
    dec.device_unfilter = device_unfilter
    return dec


PNG_FIELDS = [(GRAY8, np.uint8), (GRAY16, np.uint16), (RGB8, np.uint32), (RGBA8, np.uint32), (RGBA16, np.uint64)]


@pytest.mark.parametrize("h,w", [(2, 1), (3, 63), (3, 65), (2, 127), (2, 129), (2, 191), (2, 192), (2, 193), (63, 9), (65, 9),
                                 (129, 7)])
def test_png_unfilter_at_block_ring_and_band_edges(gpu, h, w):
    """OsfFrameDecoder.decode_fields with the filters reversed on the GPU and on the host, against osf_oracle.decode_field: the
    five PNG kinds, every row with another filter type (three arrangements per kind)."""
    from oracle import osf_oracle as Z
    from ouster_sdk_amd import core
    rng = np.random.default_rng(h * 1000 + w)
    blobs, want = [], []
    for enc, dt in PNG_FIELDS:
        depth, colour, pb = PNG_KIND[enc]
        for filters in (np.arange(h) % 5, (4 - np.arange(h)) % 5, rng.integers(0, 5, h)):
            px = rng.integers(0, 256, (h, w * pb), dtype=np.uint8)
            px[:, pb:] = (px[:, pb:] // 8 + px[:, :-pb]).astype(np.uint8)
            blob = _png_with_filters(px, depth, colour, filters)
            assert np.array_equal(Z.png_pixels(blob)[0], px)
            blobs.append((blob, FIELD_TAG[np.dtype(dt).itemsize]))
            want.append(Z.decode_field(blob, dt, h, w, [0] * h))
    for on in (True, False):
        got = _decoder(core, h, w, on).decode_fields(blobs)
        for i, (g, x) in enumerate(zip(got, want)):
            assert np.array_equal(np.frombuffer(g, x.dtype).reshape(h, w), x), ("gpu" if on else "host", i, PNG_FIELDS[i // 3][0])


# ------------------------------------------------------------------------------------------------------------------
# g. the LDS limit of k_osf_png_unfilter: 64 rings of 192 8-byte pixels + one row = 160 KB at w = 8064
# ------------------------------------------------------------------------------------------------------------------
def _rgba16_plane(w):
    from oracle import osf_oracle as Z
    h = 2
    rng = np.random.default_rng(w)
    px = rng.integers(0, 256, (h, w * 8), dtype=np.uint8)
    px[:, 8:] = (px[:, 8:] // 8 + px[:, :-8]).astype(np.uint8)
    blob = _png_with_filters(px, 16, 6, [3, 4])
    return h, blob, Z.decode_field(blob, np.uint64, h, w, [0] * h)


def test_png_unfilter_at_the_lds_limit(gpu):
    """RGBA16, w = 8064: 64 * (192 * 8 + 16) + 8064 * 8 = 163840 bytes, all the LDS a workgroup can have."""
    from ouster_sdk_amd import core
    U, O = gpu
    w = 8064
    assert 64 * (192 * 8 + 16) + w * 8 == 160 * 1024
    h, blob, want = _rgba16_plane(w)
    got = _decoder(core, h, w, True).decode_fields([(blob, 4)])[0]
    assert np.array_equal(np.frombuffer(got, np.uint64).reshape(h, w), want)
    direct = U.check([Job(zlib.decompress(OO_idat(blob)), RGBA16, 8, 8, want, FILTERED, "rgba16 filtered")], h, w, [0] * h)
    assert bytes(direct[0]) == bytes(got)


def test_png_unfilter_past_the_lds_limit_goes_to_the_host(gpu):
    """w = 8065: the C ABI refuses the filtered plane and writes nothing; the decoder reverses the filters on the host."""
    from ouster_sdk_amd import core
    U, O = gpu
    w = 8065
    h, blob, want = _rgba16_plane(w)
    job = Job(zlib.decompress(OO_idat(blob)), RGBA16, 8, 8, want, FILTERED)
    rc, got, guards = U.call([job], h, w, [0] * h)
    assert rc == U.capi.ERR_UNSUPPORTED and guards and (got[0] == PATTERN).all()
    for on in (True, False):
        g = _decoder(core, h, w, on).decode_fields([(blob, 4)])[0]
        assert np.array_equal(np.frombuffer(g, np.uint64).reshape(h, w), want), on


# ------------------------------------------------------------------------------------------------------------------
# h. arguments
# ------------------------------------------------------------------------------------------------------------------
def test_rejected_arguments_write_nothing(gpu):
    U, O = gpu
    h, w = 2, 5
    rng = np.random.default_rng(25)
    shifts = np.array([1, -1], np.int32)

    def jobs():
        return [png_job(O, rng, GRAY16, h, w, 2, None, shifts), zpng_job(O, rng.integers(0, 256, h * w * 4, dtype=np.uint8), h, w, 4),
                png_job(O, rng, RGBA8, h, w, 4, [1, 4], shifts)]
    U.check(jobs(), h, w, shifts)     # the planes as they are pass

    def setter(i, **kw):
        def edit(arr):
            for k, v in kw.items():
                setattr(arr[i], k, v)
        return edit
    bad = {"NULL src": setter(1, src=None), "NULL dst": setter(2, dst=None), "element size 3": setter(1, dst_elem_size=3),
           "element size 0": setter(0, dst_elem_size=0), "unknown flag bits": setter(2, flags=FILTERED | 2),
           "unknown flag bits on a flat plane": setter(0, flags=4),
           "gray16 with 1-byte pixels": setter(0, src_pixel_bytes=1), "rgba8 with 3-byte pixels": setter(2, src_pixel_bytes=3),
           "rgb8 with 4-byte pixels": setter(2, encoding=RGB8), "zpng with 0 pixel bytes": setter(1, src_pixel_bytes=0),
           "zpng with 9 pixel bytes": setter(1, src_pixel_bytes=9), "zpng with FLAG_FILTERED": setter(1, flags=FILTERED),
           "encoding 0": setter(1, encoding=0), "encoding 7": setter(2, encoding=7)}
    for what, edit in bad.items():
        rc, got, guards = U.call(jobs(), h, w, shifts, planes_edit=edit)
        assert rc == U.capi.ERR_INVALID_ARGUMENT, (what, rc)
        assert guards and all((g == PATTERN).all() for g in got), what
    for what, kw in {"n_planes 0": dict(n_planes=0), "h 0": dict(hw=(0, w)), "w 0": dict(hw=(h, 0))}.items():
        rc, got, guards = U.call(jobs(), h, w, shifts, **kw)
        assert rc == U.capi.OK, (what, rc)
        assert guards and all((g == PATTERN).all() for g in got), what
    U.check(jobs(), h, w, shifts)     # and the context still works


# ------------------------------------------------------------------------------------------------------------------
# i. one context, several calls: the cached offsets table and the grow-only scratch
# ------------------------------------------------------------------------------------------------------------------
def test_one_context_serves_unpack_destagger_unpack(gpu):
    U, O = gpu
    torch = U.torch
    h = 5
    sh130 = np.array([0, 7, -3, 129, -131], np.int32)
    sh100 = np.array([-1, 99, 100, 103, -205], np.int32)

    def first():
        rng = np.random.default_rng(130)
        return [png_job(O, rng, GRAY16, h, 130, 2, None, sh130), png_job(O, rng, RGBA16, h, 130, 8, [4, 3, 2, 1, 4], sh130),
                png_job(O, rng, RGB8, h, 130, 4, [0, 1, 2, 3, 4], sh130)]
    one = U.check(first(), h, 130, sh130)
    # ouster_hip_destagger with the same shifts on the same context: its offsets are the other direction's
    img = np.random.default_rng(131).integers(0, 2 ** 32, (h, 130), dtype=np.uint32)
    d_img = torch.from_numpy(img.view(np.int32)).cuda()
    d_out = torch.zeros_like(d_img)
    torch.cuda.synchronize()
    for inverse in (False, True):
        U.capi.check(U.L.ouster_hip_destagger(U.ctx.h, d_img.data_ptr(), d_out.data_ptr(), h, 130, 4, sh130.ctypes.data, h,
                                              int(inverse), 1))
        U.ctx.sync()
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), O.destagger(img, sh130, inverse)), inverse
    rng = np.random.default_rng(100)
    more = [png_job(O, rng, enc, h, 100, es, f, sh100)
            for enc, es, f in ((RGBA8, 4, None), (GRAY8, 1, [4, 4, 3, 3, 1]), (RGBA16, 8, [2, 4, 0, 3, 1]), (GRAY16, 2, None),
                               (RGB8, 4, [3, 4, 1, 2, 0]), (RGBA16, 8, None))]     # more planes and more filtered bytes than before
    U.check(more, h, 100, sh100)
    four = U.check(first(), h, 130, sh130)
    assert [bytes(a) for a in one] == [bytes(b) for b in four]


# ------------------------------------------------------------------------------------------------------------------
# j. decoder level, ZPNG
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(3, 65), (3, 257), (2, 1000)])
def test_decoder_decodes_model_encoded_zpng_fields(gpu, h, w):
    from ouster_sdk_amd import core
    rng = np.random.default_rng(h * 10000 + w)
    blobs, want = [], []
    for es in (1, 2, 4, 8):
        px = rng.integers(0, 256, (h, w * es), dtype=np.uint8)
        px[:, ::3] >>= 4
        blobs.append((M.encode(px, h, w, *M.LAYOUTS[es]), FIELD_TAG[es]))
        want.append(px.tobytes())
    dec = _decoder(core, h, w)
    got = dec.decode_fields(blobs)         # u8, u16, u32 and u64 in one call
    assert [bytes(g) for g in got] == want

    # headers that disagree with the decoder's geometry or the field's element
    body = M.zstd_compress(M.residuals(np.zeros(h * w * 2, np.uint8), h, w, 2))
    for hdr in (M.header(h, w + 1, 1, 2), M.header(h + 1, w, 1, 2), M.header(h, w, 1, 1), M.header(h, w, 3, 1), M.header(h, w, 2, 2)):
        with pytest.raises(RuntimeError, match="Invalid allocation"):
            dec.decode_fields([(hdr + body, 2)])
        with pytest.raises(RuntimeError, match="Invalid allocation"):
            dec.decode_fields(blobs + [(hdr + body, 2)] + blobs)
    # a zstd frame cut in half; a whole frame that holds fewer bytes than h * w * pb
    frame = blobs[2][0][8:]
    cut = M.header(h, w, 4, 1) + frame[:len(frame) // 2]
    short = M.header(h, w, 4, 1) + M.zstd_compress(M.residuals(np.frombuffer(want[2], np.uint8), h, w, 4)[:-4])
    for bad in (cut, short):
        with pytest.raises(RuntimeError, match="could not decode field"):
            dec.decode_fields([(bad, 3)])
        with pytest.raises(RuntimeError, match="could not decode field"):
            dec.decode_fields(blobs + [(bad, 3)] + blobs)     # in the middle of a batch
        again = dec.decode_fields(blobs + blobs)               # the same decoder serves the next call
        assert [bytes(g) for g in again] == want + want
