"""FDiv (csrc/svc_fdiv.h), the multiply-shift division of the kernels' index arithmetic, compiled on its own for the host: exact for
every dividend below 2^31 at every divisor in use -- k_quantise divides by h * w, 2^16 and more for the big maps -- and wrong
beyond 2^31, where the 64-bit product wraps: the domain the header states."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from test_net_plan_census import DOWN_SHAPES, SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = [(416, 256), (416, 250)]                     # tests/test_gpu_map_shapes.py: the shapes of the saliency entry alone
SPAN = 1000
u32, u64 = ctypes.c_uint32, ctypes.c_uint64


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('native') / 'libfdiv_harness.so')
    subprocess.check_call(['g++', '-O2', '-shared', '-fPIC', '-o', out, os.path.join(ROOT, 'tests', 'native', 'fdiv_harness.cpp')])
    lib = ctypes.CDLL(out)
    lib.fdiv_one.argtypes, lib.fdiv_one.restype = [u32, u32], u32
    lib.fdiv_constants.argtypes, lib.fdiv_constants.restype = [u32, ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_int)], None
    lib.fdiv_sweep.argtypes = [ctypes.c_void_p, ctypes.c_int, u32, u64, u64, ctypes.c_void_p, ctypes.c_void_p]
    lib.fdiv_sweep.restype = u64
    return lib


def _sweep(lib, divisors, limit):
    d = np.ascontiguousarray(divisors, np.uint32)
    bad, checked = np.zeros(3, np.uint64), np.zeros(1, np.uint64)
    failures = lib.fdiv_sweep(d.ctypes.data, len(d), SPAN, limit, 12345, bad.ctypes.data, checked.ctypes.data)
    return int(failures), [int(v) for v in bad], int(checked[0])


def _divisors():
    assert all(s in SHAPES for s in IDENTITY)
    shapes = sorted(set(SHAPES) | set(DOWN_SHAPES) | set(IDENTITY))
    big = [h * w for h, w in shapes]
    assert 416 * 256 in big and 540 * 960 in big and sum(v >= 1 << 16 for v in big) >= 6
    return list(range(1, 1 << 16)) + big + [(1 << 16) - 1, 1 << 16, (1 << 16) + 1]


def test_the_quotient_is_exact_below_two_to_the_31(harness):
    """Every d in 1 .. 65 535, the h * w of every map shape of the device tests, 2^16 - 1, 2^16, 2^16 + 1; n = k d - 1, k d and
    k d + d - 1 for the first and the last 1 000 multiples below 2^31 and 1 000 random ones; and m < 2^33 for every d."""
    divisors = _divisors()
    failures, bad, checked = _sweep(harness, divisors, 1 << 31)
    assert failures == 0, ('(d, n, quotient) of the first failure', bad, failures)
    assert checked > len(divisors) * SPAN * 3                        # (small divisors: all three spans; the largest: kmax + 1 multiples)
    # the harness's arithmetic against Python's own, on a few
    rng = np.random.RandomState(1)
    for d in [1, 2, 3, 7, 255, 65535, 65537, 106496, 518400] + rng.randint(1, 1 << 21, 50).tolist():
        m, s = u64(), ctypes.c_int()
        harness.fdiv_constants(d, ctypes.byref(m), ctypes.byref(s))
        l = (d - 1).bit_length()
        assert (m.value, s.value) == (-(-(1 << (32 + l)) // d), 32 + l) and m.value < 1 << 33, d
        for n in [0, d - 1, d, (1 << 31) - 1, ((1 << 31) - 1) // d * d, ((1 << 31) - 1) // d * d - 1] + rng.randint(0, 1 << 31, 20).tolist():
            if n >= 0:
                assert harness.fdiv_one(d, n) == n // d == (n * m.value) >> s.value, (d, n)


def test_beyond_two_to_the_31_the_product_wraps(harness):
    """The limit that is real: n m needs more than 64 bits, and the quotient is wrong -- at most divisors, not at powers of two
    (m = 2^32 there, and n m < 2^64 for every 32-bit n)."""
    assert harness.fdiv_one(3, 0xFFFFFFFF) == 0x55555555 - (1 << 30) != 0xFFFFFFFF // 3
    failures, bad, _ = _sweep(harness, [3, 7, 250, 35000, 106496, 518400], 1 << 32)
    assert failures > 0 and bad[1] >= 1 << 31, (failures, bad)
    failures, bad, _ = _sweep(harness, [1, 2, 256, 65536, 1 << 20], 1 << 32)
    assert failures == 0, bad


def test_the_library_uses_the_header_and_states_its_domain():
    src = os.path.join(ROOT, 'retargetvid_amd', 'csrc')
    internal = open(os.path.join(src, 'svc_internal.h')).read()
    header = open(os.path.join(src, 'svc_fdiv.h')).read()
    assert '#include "svc_fdiv.h"' in internal and 'struct FDiv' not in internal and 'struct FDiv' in header
    assert re.search(r'uint32_t fdiv\(uint32_t n, const FDiv &f\) \{ return fdiv_q\(n, f\.m, f\.s\); \}', internal)
    assert re.findall(r'#include\s+(\S+)', header) == ['<stdint.h>']
    assert 'd < 2^16' not in internal + header and 'n < 2^31' in internal and 'n < 2^31' in header
    assert 'svc_fdiv.h' in open(os.path.join(src, 'Makefile')).read()
