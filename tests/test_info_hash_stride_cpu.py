"""The 2^20 + 65 job InfoHash batch (tests/info_hash_stride.py) checked where no GPU is: its
bencode is the library's, its 1,757 distinct shapes give the expected digests through the
kernel's own arithmetic on the host (krk_info_hash_math_host), and the expansion to the batch
separates the jobs the way the GPU test relies on."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

from kraken_amd._capi import check, lib
from tests import info_hash_stride as S


def test_bencode_is_the_librarys():
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))
    k = gold["kat"]["info_hash"]  # core/metainfo_test.go:61-76
    enc = S.bencode(k["piece_length"], k["piece_sums"], k["name"].encode(), k["length"])
    assert hashlib.sha1(enc).hexdigest() == k["expected"]
    sums = np.array(S.SUMS, dtype=np.uint32)
    for P, name, L in ((1, b"", 0), (7, b"", 250), (4 << 20, b"x" * 11, 10 ** 12)):
        w = C.c_uint64()
        buf = (C.c_uint8 * 256)()
        check(lib.krk_bencode_info(P, sums.ctypes.data_as(C.POINTER(C.c_uint32)), 3, name or None, len(name), L, buf, 256,
                                   C.byref(w)))
        assert bytes(buf[:w.value]) == S.bencode(P, S.SUMS, name, L)
    assert S.bencode(3, S.SUMS, b"", 17) == b"d6:Lengthi17e4:Name0:11:PieceLengthi3e9:PieceSumsli0ei4294967295ei1000000000eee"


def test_every_shape_through_the_kernels_arithmetic():
    t = S.table()
    assert t.shape == (251, 7, 20) and np.unique(t.reshape(-1, 20), axis=0).shape[0] == 1757
    sums = np.array(S.SUMS, dtype=np.uint32)
    sp = sums.ctypes.data_as(C.POINTER(C.c_uint32))
    out = (C.c_uint8 * 20)()
    for L in range(S.N_LENGTHS):
        for p in range(S.N_PIECE_LENGTHS):
            check(lib.krk_info_hash_math_host(p + 1, sp, 3, None, 0, L, out))
            assert bytes(out) == bytes(t[L, p]), (L, p + 1)
    # every job hashes two SHA-1 blocks: the ring is compressed once before the padding and once
    # after it, so a second job meets a ring, pos and done its first job has moved
    sizes = {len(S.bencode(p + 1, S.SUMS, b"", L)) for L in range(251) for p in range(7)}
    assert sizes == {78, 79, 80} and all(64 <= s and s + 9 <= 128 for s in sizes)


def test_expansion_separates_the_jobs():
    assert S.N_JOBS == 2 ** 20 + 65 > S.MAX_GRID
    ln, pl = S.fields()
    assert ln.size == S.N_JOBS and ln.max() == 250 and pl.min() == 1 and pl.max() == 7
    want = S.expected()
    assert want.shape == (S.N_JOBS, 20)
    t = S.table()
    for i in (0, 1, 250, 251, 1756, 1757, S.MAX_GRID - 1, S.MAX_GRID, S.N_JOBS - 1):
        assert bytes(want[i]) == hashlib.sha1(S.bencode(1 + i % 7, S.SUMS, b"", i % 251)).digest() == bytes(t[i % 251, i % 7])
    # a workgroup's two jobs (j and j + 2^20) differ in both fields, and so do neighbouring rows
    j = np.arange(65)
    assert (ln[j] != ln[j + S.MAX_GRID]).all() and (pl[j] != pl[j + S.MAX_GRID]).all()
    assert (ln[:-1] != ln[1:]).all() and (pl[:-1] != pl[1:]).all()
    assert not (want[j] == want[j + S.MAX_GRID]).all(axis=1).any()
    assert not (want[:-1] == want[1:]).all(axis=1).any()
