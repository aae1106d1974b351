"""The device InfoHash without a device: the kernel's own arithmetic (csrc/info_hash_math.hpp:
digit count and emit by multiply-high, the header builder, the byte ring, the padding, the SHA-1
block function) run on the host by krk_info_hash_math_host against krk_info_hash (host bencode
+ SHA-1, which tests/test_capi_cpu.py pins to the oracle), the placement setter and getter,
and krk_info_hash_batch_dev failing loudly where no device is visible."""
import ctypes as C

import numpy as np
import pytest

from kraken_amd import _capi
from kraken_amd import device as D
from kraken_amd._capi import check, lib

DIGIT_SUMS = sorted({0, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1} | {10 ** k - 1 for k in range(1, 10)} |
                    {10 ** k for k in range(1, 10)})
INT64_SET = [0, 1, 9, 10, 2 ** 31, 2 ** 63 - 1, -1, -2 ** 63]


def _both(P, sums, name: bytes, L):
    s = np.ascontiguousarray(sums, dtype=np.uint32)
    sp = s.ctypes.data_as(C.POINTER(C.c_uint32)) if s.size else None
    a, b = (C.c_uint8 * 20)(), (C.c_uint8 * 20)()
    check(lib.krk_info_hash(P, sp, s.size, name or None, len(name), L, a))
    check(lib.krk_info_hash_math_host(P, sp, s.size, name or None, len(name), L, b))
    return bytes(a), bytes(b)


def test_math_host_reference_kat():
    """core/metainfo_test.go:61-76 through the kernel's arithmetic."""
    import json
    import os
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))
    k = gold["kat"]["info_hash"]
    a, b = _both(k["piece_length"], k["piece_sums"], k["name"].encode(), k["length"])
    assert a.hex() == b.hex() == k["expected"]


def test_math_host_digit_counts():
    """Every decimal width of a sum, alone, in one blob, and in lane steps of 64 and 65 copies."""
    a, b = _both(4 << 20, DIGIT_SUMS, b"n", 5)
    assert a == b
    for v in DIGIT_SUMS:
        for reps in (1, 64, 65):
            a, b = _both(1 << 20, [v] * reps, b"abc", 77)
            assert a == b, (v, reps)


def test_math_host_int64_fields():
    """length and piece_length at the digit steps of int64, negative values as put_i64 writes them."""
    for L in INT64_SET:
        for P in INT64_SET:
            a, b = _both(P, [1, 22, 333], b"x" * 7, L)
            assert a == b, (L, P)


def test_math_host_padding_residues():
    """n_sums = 0 and name lengths 0..130: the hashed length takes every residue mod 64 twice
    (55, 56, 63 and 0 among them) and the name-length digits step 9 -> 10 and 99 -> 100."""
    seen = set()
    for n in range(131):
        name = bytes((37 * i + n) % 251 + 1 for i in range(n))
        a, b = _both(1, [], name, 0)
        assert a == b, n
        w = C.c_uint64()
        check(lib.krk_bencode_info(1, None, 0, name or None, n, 0, None, 0, C.byref(w)))
        seen.add(w.value % 64)
    assert seen == set(range(64))


def test_math_host_tile_edges():
    rng = np.random.default_rng(0x1F0)
    for n in (0, 1, 63, 64, 65, 127, 128, 129, 1000, 4097, 81920):
        sums = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
        sums[::3] >>= rng.integers(0, 32, size=sums[::3].size).astype(np.uint32)  # mixed widths
        a, b = _both(1 << 20, sums, rng.bytes(int(rng.integers(0, 70))).hex().encode()[:int(rng.integers(0, 99))], n << 20)
        assert a == b, n


def test_placement_round_trips_without_a_device():
    assert D.info_hash_placement() == _capi.KRK_PLACE_AUTO  # the default
    try:
        for p in (_capi.KRK_PLACE_GPU, _capi.KRK_PLACE_HOST, _capi.KRK_PLACE_AUTO):
            D.set_info_hash_placement(p)
            assert D.info_hash_placement() == p
        for bad in (-1, 3, 99):
            assert lib.krk_set_info_hash_placement(bad) == _capi.KRK_EINVAL
            assert D.info_hash_placement() == _capi.KRK_PLACE_AUTO
        assert lib.krk_info_hash_placement(None) == _capi.KRK_EINVAL
    finally:
        D.set_info_hash_placement(_capi.KRK_PLACE_AUTO)
    assert D.metainfo_batch_last_placement() == _capi.KRK_PLACE_HOST  # no batch ran: the default's


def test_info_hash_batch_dev_needs_a_device():
    n = C.c_int(-1)
    check(lib.krk_device_count(C.byref(n)))
    if n.value > 0:
        pytest.skip("a GPU is visible")
    one = np.ones(1, np.int64)
    z = np.zeros(2, np.uint64)
    i64p, u64p = C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
    out = (C.c_uint8 * 20)()
    rc = lib.krk_info_hash_batch_dev(one.ctypes.data_as(i64p), None, z.ctypes.data_as(u64p), z.ctypes.data_as(u64p),
                                     None, z.ctypes.data_as(u64p), one.ctypes.data_as(i64p), 1, out, None)
    assert rc == _capi.KRK_ENODEV
    assert b"no HIP device" in lib.krk_last_error()
