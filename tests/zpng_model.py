"""The ENCODER side of the ZPNG codec in plain numpy (test infrastructure): what PackAndFilter<N> of the reference's
thirdparty/zpng/zpng.cpp:47-100, 243-297 leaves for zstd, for every pixel size the header allows (1..8 bytes).  The tests
feed its output to the product's ZPNG path and expect the pixels back; tests/test_oracle_osf.py pins it on the reference's
own codec (byte for byte against the body of ZPNG_Compress, and through ZPNG_Decompress) where that library was built.

  every byte lane of a row     d[x] = p[x] - p[x-1] mod 256, p[-1] = 0
  1, 2, 5, 6, 7, 8-byte pixels the deltas, interleaved as the pixels are
  3 / 4-byte pixels            colour planes of h * w bytes each: y = dB, u = dG - dB, v = dG - dR [, dA] (lanes R, G, B, A =
                               bytes 0, 1, 2, 3 of the pixel)
"""
import ctypes as C
import struct

import numpy as np

MAGIC = 0xFBF8
# one (channels, bytes per channel) for every pixel size
LAYOUTS = {1: (1, 1), 2: (1, 2), 3: (3, 1), 4: (4, 1), 5: (5, 1), 6: (3, 2), 7: (7, 1), 8: (4, 2)}


def residuals(pixels, h: int, w: int, pb: int) -> bytes:
    """pixels: uint8, h * w * pb bytes in any shape -> the h * w * pb residual bytes the codec hands to zstd."""
    p = np.ascontiguousarray(pixels, dtype=np.uint8).reshape(h, w, pb).astype(np.int64)
    d = np.diff(p, axis=1, prepend=0) & 0xFF
    if pb in (3, 4):
        dr, dg, db = d[..., 0], d[..., 1], d[..., 2]
        planes = [db, (dg - db) & 0xFF, (dg - dr) & 0xFF] + ([d[..., 3]] if pb == 4 else [])
        return np.stack(planes).astype(np.uint8).tobytes()
    return d.astype(np.uint8).tobytes()


_zstd = None


def zstd_compress(data: bytes, level: int = 1) -> bytes:
    """ZSTD_compress of the libzstd.so.1 the product links."""
    global _zstd
    if _zstd is None:
        _zstd = C.CDLL("libzstd.so.1")
        _zstd.ZSTD_compress.restype = C.c_size_t
        _zstd.ZSTD_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
        _zstd.ZSTD_compressBound.restype = C.c_size_t
        _zstd.ZSTD_compressBound.argtypes = [C.c_size_t]
        _zstd.ZSTD_isError.restype = C.c_uint
        _zstd.ZSTD_isError.argtypes = [C.c_size_t]
    cap = _zstd.ZSTD_compressBound(len(data))
    out = C.create_string_buffer(cap)
    n = _zstd.ZSTD_compress(out, cap, data, len(data), level)
    if _zstd.ZSTD_isError(n):
        raise RuntimeError("ZSTD_compress failed")
    return out.raw[:n]


def header(h: int, w: int, channels: int, bpc: int) -> bytes:
    return struct.pack("<HHHBB", MAGIC, w, h, channels, bpc)


def encode(pixels, h: int, w: int, channels: int, bpc: int) -> bytes:
    """A ZPNG image: the 8-byte header {magic, width, height, channels, bytes per channel} + the zstd frame of the residuals."""
    return header(h, w, channels, bpc) + zstd_compress(residuals(pixels, h, w, channels * bpc))
