"""ouster_hip_range_gate without a GPU: the raw thresholds of the range-gated frame dewarp.  The reference derives them in two
lines (impl/dewarp_impl.h:33-34): min_r = uint32(ceil(min_range * 1e3)), max_r = uint32(floor(max_range * 1e3)).  Restated here
in numpy with what the conversion to uint32 leaves open made explicit: the values saturate at 0 and 2^32 - 1, and a gate that no
uint32 range can pass (max below 0, min above 2^32 - 1, max below min, a NaN on either side) is empty and reads (0, 0, 1).  The
frame dewarp and the decode's range-gate by-product both take their thresholds from this one function."""
import ctypes as C

import numpy as np
import pytest

from ouster_sdk_amd import _capi as capi

U32_MAX = 4294967295
INF, NAN = float("inf"), float("nan")

# (min_range, max_range) in metres -> (min_r, max_r, empty)
TABLE = [
    ((0, 0), (0, 0, 0)),
    ((0.0005, 0.0015), (1, 1, 0)),
    ((0.0011, 0.0019), (0, 0, 1)),
    ((-1, 2.5), (0, 2500, 0)),
    ((1, -0.0005), (0, 0, 1)),
    ((0, 1e9), (0, 4294967295, 0)),
    ((4294967.296, 1e9), (0, 0, 1)),
    ((NAN, 1), (0, 0, 1)),
    ((0, NAN), (0, 0, 1)),
    ((2, 2), (2000, 2000, 0)),
    ((0.5, 0.25), (0, 0, 1)),
    ((0.001, 4294967), (1, 4294967000, 0)),
    ((-INF, INF), (0, 4294967295, 0)),
    ((INF, INF), (0, 0, 1)),
]
IDS = ["%g..%g" % g for g, _ in TABLE]


def reference_gate(min_range, max_range):
    lo = np.ceil(np.float64(min_range) * 1e3)
    hi = np.floor(np.float64(max_range) * 1e3)
    if not (hi >= 0) or not (lo <= U32_MAX) or hi < lo:
        return (0, 0, 1)
    return (int(np.clip(lo, 0, U32_MAX)), int(np.clip(hi, 0, U32_MAX)), 0)


def c_gate(min_range, max_range, want=(True, True, True)):
    """(min_r, max_r, empty) from the C ABI; an output that is not wanted is passed as NULL and comes back as None"""
    lo, hi, empty = C.c_uint32(0xdeadbeef), C.c_uint32(0xdeadbeef), C.c_int(-7)
    args = [C.byref(v) if w else None for v, w in zip((lo, hi, empty), want)]
    capi.check(capi.load_hip().ouster_hip_range_gate(float(min_range), float(max_range), *args))
    return tuple(int(v.value) if w else None for v, w in zip((lo, hi, empty), want))


@pytest.mark.parametrize("gate,expected", TABLE, ids=IDS)
def test_range_gate_equals_the_reference_arithmetic(gate, expected):
    assert reference_gate(*gate) == expected
    assert c_gate(*gate) == expected


@pytest.mark.parametrize("gate,expected", TABLE, ids=IDS)
def test_range_gate_accepts_null_outputs(gate, expected):
    for skip in range(3):
        want = tuple(i != skip for i in range(3))
        assert c_gate(*gate, want=want) == tuple(e if w else None for e, w in zip(expected, want))
    assert c_gate(*gate, want=(False, False, False)) == (None, None, None)
