"""The library's own device-wide primitives (csrc/hip/sd_scan_sort.h: reduce-then-scan prefix sums / running maxima and the stable LSD
radix sort of (key, value) pairs that replaced hipCUB on the hot path; csrc/hip/sd_field_sort.h: the chained sort by several fields of the
grouping modules) through their self-test entry points of the C ABI, against numpy: sizes around the tile (4 096) and workgroup
boundaries, bit ranges that are not multiples of the digit, equal keys (stability)."""
import ctypes as C

import numpy as np
import pytest

from spacedust_amd import _lib
from spacedust_amd._lib import ptr

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('n', [1, 2, 63, 64, 255, 4095, 4096, 4097, 65536, 1000003, 5 * 4096 * 1024 + 17])
def test_radix_sort_pairs_is_stable_and_sorted(gpu, n):
    L = _lib.load()
    L.sd_selftest_sort_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(n)
    for begin, end, spread in ((0, 32, 1 << 32), (0, 16, 1 << 16), (0, 5, 40), (7, 19, 1 << 22), (3, 32, 1 << 32), (0, 32, 3)):
        keys = rng.integers(0, spread, size=n, dtype=np.uint64).astype(np.uint32)
        vals = np.arange(n, dtype=np.uint32)
        ok, ov = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        assert L.sd_selftest_sort_pairs(gpu.h, ptr(keys), ptr(vals), n, begin, end, ptr(ok), ptr(ov)) == 0
        digit = (keys >> np.uint32(begin)) & np.uint32((1 << (end - begin)) - 1 if end - begin < 32 else 0xFFFFFFFF)
        order = np.argsort(digit, kind='stable')
        assert np.array_equal(ov, vals[order]), (n, begin, end)
        assert np.array_equal(ok, keys[order]), (n, begin, end)
        if n > 2000000:
            break   # (one bit range at the largest size)


@pytest.mark.parametrize('n', [1, 15, 16, 4095, 4096, 4097, 8 * 4096 * 1024 + 3])
def test_scans_equal_numpy(gpu, n):
    L = _lib.load()
    L.sd_selftest_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(n + 1)
    x = rng.integers(0, 1 << 31, size=n, dtype=np.uint64).astype(np.uint32)
    ex = np.zeros(n + 1, np.uint64)
    mx = np.zeros(n, np.uint32)
    assert L.sd_selftest_scan(gpu.h, ptr(x), n, ptr(ex), ptr(mx)) == 0
    want = np.zeros(n + 1, np.uint64)
    np.cumsum(x.astype(np.uint64), out=want[1:])
    assert np.array_equal(ex, want)
    assert np.array_equal(mx, np.maximum.accumulate(x))


def _field_and_key(rng, n, mode, width):
    """one field of n values (uint32) whose sort key under `mode` needs `width` bits -> (field, arg, key)"""
    if mode == 0:     # plain
        v = rng.integers(0, 1 << width, size=n, dtype=np.uint64)
        arg = 0
        key = v
    elif mode == 1:   # subtracted from arg, the largest value
        v = rng.integers(0, 1 << width, size=n, dtype=np.uint64)
        arg = int(v.max()) if n else 0
        key = np.uint64(arg) - v
    else:             # biased: negative values stored as uint32, as the kmermatcher's diagonal is
        arg = ((1 << width) - 1) // 2
        d = rng.integers(-arg, arg + 1, size=n, dtype=np.int64)
        v = (d & 0xFFFFFFFF).astype(np.uint64)
        key = (d + arg).astype(np.uint64)
    return v.astype(np.uint32), arg, key


@pytest.mark.parametrize('n', [0, 1, 63, 4096, 4097, 70001])
def test_field_sort_chain(gpu, n):
    """sortByField link by link, least significant field first, and gatherFields (sd_selftest_field_sort) against numpy.lexsort, which is
    stable like the chain: the permutation and the gathered fields are equal, not merely sorted."""
    L = _lib.load()
    rng = np.random.default_rng(1000 + n)

    def check(cols):   # cols: (field, mode, arg, bits, key), least significant first
        nf = len(cols)
        fields = np.ascontiguousarray(np.stack([c[0] for c in cols]).reshape(nf, n))
        modes = np.array([c[1] for c in cols], np.int32)
        args = np.array([c[2] for c in cols], np.uint32)
        bits = np.array([c[3] for c in cols], np.int32)
        perm = np.full(n, 0xFFFFFFFF, np.uint32)
        out = np.full((nf, n), 0xFFFFFFFF, np.uint32)
        assert L.sd_selftest_field_sort(gpu.h, n, nf, ptr(fields), ptr(modes), ptr(args), ptr(bits), ptr(perm), ptr(out)) == 0
        want = np.lexsort([c[4] for c in cols]).astype(np.uint32) if n else np.zeros(0, np.uint32)
        tag = (n, modes.tolist(), bits.tolist())
        assert np.array_equal(perm, want), tag
        assert np.array_equal(out, fields[:, want]), tag
        return perm

    def col(mode, width):
        v, arg, key = _field_and_key(rng, n, mode, width)
        return (v, mode, arg, width, key)

    widths = (1, 8, 9, 32)
    for width in widths:            # one field: every mode at every width
        for mode in (0, 1, 2):
            check([col(mode, width)])
    for nf in (3, 5):               # several fields: every mode in every chain, the widths mixed and alike
        for c, width in enumerate(widths):
            check([col((f + c) % 3, width) for f in range(nf)])
        check([col((f + 1) % 3, widths[f % 4]) for f in range(nf)])
    # every key equal: the order stays the input's
    const = lambda value, mode, arg, bits, key: (np.full(n, value, np.uint32), mode, arg, bits, np.full(n, key, np.uint64))
    same = [const(5, 0, 0, 9, 5), const(7, 1, 7, 8, 0), const(0xFFFFFFFD, 2, 3, 1, 0)]
    assert np.array_equal(check(same), np.arange(n, dtype=np.uint32))
    # only the most significant field differs
    check(same[:2] + [col(0, 9)])
