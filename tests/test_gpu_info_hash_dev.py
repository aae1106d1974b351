"""krk_info_hash_batch_dev (device.info_hash_batch_dev): info.Hash() (core/metainfo.go:37-44)
computed by the device kernel (csrc/info_hash.hip) from piece sums in device memory, bit for
bit against the oracle's bencode + SHA-1 -- and, for negative Length / PieceLength, against
the library's own krk_info_hash, which defines those bytes -- plus the InfoHash placement of
krk_metainfo_batch_dev (krk_set_info_hash_placement)."""
import ctypes as C

import numpy as np
import pytest

from kraken_amd import _capi
from kraken_amd import device as D
from kraken_amd._capi import check, lib

pytestmark = pytest.mark.gpu

DIGIT_SUMS = sorted({0, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1} | {10 ** k - 1 for k in range(1, 10)} |
                    {10 ** k for k in range(1, 10)})
INT64_SET = [0, 1, 9, 10, 2 ** 31, 2 ** 63 - 1, -1, -2 ** 63]


def _host_hash(P, sums, name, L):
    s = np.ascontiguousarray(sums, dtype=np.uint32)
    out = (C.c_uint8 * 20)()
    nb = name.encode()
    check(lib.krk_info_hash(P, s.ctypes.data_as(C.POINTER(C.c_uint32)) if s.size else None, s.size, nb or None,
                            len(nb), L, out))
    return bytes(out)


class Batch:
    """Blobs as (piece_length, sums, name, length); their sums laid out in one device buffer at
    offsets the caller may permute and space out."""

    def __init__(self, blobs, order=None, gap=0):
        self.blobs = blobs
        n = len(blobs)
        self.ns = np.array([len(b[1]) for b in blobs], dtype=np.uint64)
        self.off = np.zeros(n, dtype=np.uint64)
        at = 0
        for i in (range(n) if order is None else order):
            self.off[i] = at
            at += int(self.ns[i]) + gap
        flat = np.full(max(at, 1), 0xDEADBEEF, dtype=np.uint32)
        for i, b in enumerate(blobs):
            flat[int(self.off[i]):int(self.off[i]) + len(b[1])] = np.asarray(b[1], dtype=np.uint32)
        self.sums = D.DeviceBuffer(flat.nbytes)
        self.sums.from_host(flat)
        self.pl = np.array([b[0] for b in blobs], dtype=np.int64)
        self.ln = np.array([b[3] for b in blobs], dtype=np.int64)
        self.names = [b[2] for b in blobs]

    def run(self, out=None, stream=None, names="given"):
        return D.info_hash_batch_dev(self.pl, self.sums, self.off, self.ns, self.names if names == "given" else names,
                                     self.ln, out=out, stream=stream)

    def check(self, got, orc, host=False):
        assert got.shape == (len(self.blobs), 20)
        for i, (P, sums, name, L) in enumerate(self.blobs):
            want = _host_hash(P, sums, name, L) if host else orc.info_hash(P, sums, name, L)
            assert bytes(got[i]) == want, (i, P, len(sums), name, L)


def test_reference_kat(gpu):
    """core/metainfo_test.go:61-76."""
    import json
    import os
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))
    k = gold["kat"]["info_hash"]
    assert (k["piece_length"], k["piece_sums"], k["length"]) == (4194304, [2131691452], 236)
    b = Batch([(k["piece_length"], k["piece_sums"], k["name"], k["length"])])
    got = b.run()
    assert bytes(got[0]).hex() == k["expected"] == "85b978c4377625b3963df406d0dd3a1da5a7d9c3"


def test_padding_residues(gpu, orc):
    """One launch, 131 blobs, n_sums = 0, name lengths 0..130: the hashed length takes every
    residue mod 64 twice (55, 56, 63, 0) and the name-length digits step 9 -> 10, 99 -> 100."""
    blobs = [(1, [], "".join(chr(97 + (7 * i + n) % 26) for i in range(n)), 0) for n in range(131)]
    res = {len(orc.bencode_info(*b)) % 64 for b in blobs}
    assert res == set(range(64))
    b = Batch(blobs)
    b.check(b.run(), orc)
    empty = Batch([(1, [], "", 0)] * 3)
    empty.check(empty.run(names=None), orc)  # names == NULL: every name empty


def test_digit_counts(gpu, orc):
    blobs = [(4 << 20, DIGIT_SUMS, "digits", 5)]
    for v in DIGIT_SUMS:  # a lane step of equal widths, and the step after it
        blobs += [(1 << 20, [v] * 64, "w64", v), (1 << 20, [v] * 65, "w65", v)]
    b = Batch(blobs)
    b.check(b.run(), orc)


def test_int64_fields(gpu, orc):
    blobs = [(P, [1, 22, 333], "n%d" % k, L) for k, (L, P) in enumerate((L, P) for L in INT64_SET for P in INT64_SET)]
    b = Batch(blobs)
    got = b.run()
    b.check(got, orc, host=True)  # krk_info_hash defines the bytes of negative values
    nonneg = [i for i, x in enumerate(blobs) if x[0] >= 0 and x[3] >= 0]
    for i in nonneg:
        assert bytes(got[i]) == orc.info_hash(*blobs[i]), blobs[i]


def _rand_sums(rng, n):
    s = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    s[::3] >>= rng.integers(0, 32, size=s[::3].size).astype(np.uint32)  # every decimal width
    return s


def _name(rng, n):
    return "".join(chr(c) for c in rng.integers(33, 127, size=n))


def test_tile_edges(gpu, orc):
    """n_sums around the 64-lane step, odd name lengths (unaligned name bytes), sums_off
    permuted and with gaps."""
    rng = np.random.default_rng(0x1F1)
    sizes = [0, 1, 63, 64, 65, 127, 128, 129, 1000, 4097]
    blobs = [(1 << 20, _rand_sums(rng, n), _name(rng, 2 * k + 1), n << 20) for k, n in enumerate(sizes)]
    b = Batch(blobs, order=rng.permutation(len(blobs)), gap=3)
    b.check(b.run(), orc)


def test_c4_sum_count(gpu, orc):
    """One blob of 81,920 sums (config C4's count): about 1 MiB of text through the ring."""
    rng = np.random.default_rng(0xC4)
    b = Batch([(4 << 20, _rand_sums(rng, 81920), "c4" * 32, 81920 * (4 << 20) - 5)])
    b.check(b.run(), orc)


@pytest.mark.parametrize("n_blobs", [1, 63, 64, 65, 257])
def test_blob_counts_mixed_lengths(gpu, orc, n_blobs):
    rng = np.random.default_rng(n_blobs)
    ns = rng.integers(0, 300, n_blobs)
    ns[::5] = 0
    blobs = [(int(rng.integers(1, 1 << 40)), _rand_sums(rng, int(n)), _name(rng, int(rng.integers(0, 80))),
              int(rng.integers(0, 1 << 50))) for n in ns]
    b = Batch(blobs, order=rng.permutation(n_blobs), gap=int(n_blobs % 3))
    b.check(b.run(), orc)


def test_stream_order_and_staging(gpu, orc):
    """krk_piece_sums_dev then krk_info_hash_batch_dev on one stream with no sync between; the
    host descriptor arrays are overwritten right after the call returns."""
    lengths, P = [0, 1, 4097, (1 << 20) + 5, 3 << 18, 300_001], 1 << 16
    ids = [7700 + i for i in range(len(lengths))]
    arena = D.BlobArena(lengths, P, blob_ids=ids)
    out = D.BatchOutputs(arena)
    n = len(lengths)
    names = [f"{i:063x}" for i in ids]  # odd length
    nbuf, noff = D.pack_names(names)
    nb = bytearray(nbuf)
    nbc = (C.c_char * len(nb)).from_buffer(nb)
    pl, ln = arena.piece_lengths.astype(np.int64), arena.lengths.astype(np.int64)
    so, ns = arena.sums_off.copy(), arena.n_pieces.copy()
    dst = D.PinnedArray((n, 20), np.uint8)
    dst.a[:] = 0
    s = C.c_void_p()
    check(lib.krk_stream_create(C.byref(s)))
    try:
        i64p, u64p = C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
        D.piece_sums(arena, out, stream=s)
        check(lib.krk_info_hash_batch_dev(pl.ctypes.data_as(i64p), out.sums.ptr, so.ctypes.data_as(u64p),
                                          ns.ctypes.data_as(u64p), nbc, noff.ctypes.data_as(u64p),
                                          ln.ctypes.data_as(i64p), n, dst.ptr, s))
        for a in (pl, ln):
            a[:] = -12345
        for a in (so, ns, noff):
            a[:] = 0xFFFFFFFFFFFF
        nb[:] = b"\xff" * len(nb)
        check(lib.krk_stream_sync(s))
    finally:
        del nbc
        check(lib.krk_stream_destroy(s))
    sums = out.sums.to_host(np.uint32, max(arena.total_pieces, 1))
    for k, L in enumerate(lengths):
        want = [int(x) for x in orc.calc_piece_sums(orc.synth(ids[k], L), P)[1]]
        o, c = int(arena.sums_off[k]), int(arena.n_pieces[k])
        assert sums[o:o + c].tolist() == want
        assert bytes(dst.a[k]) == orc.info_hash(P, want, names[k], L), k


def test_destinations(gpu, orc):
    rng = np.random.default_rng(0xD5)
    blobs = [(1 << 20, _rand_sums(rng, n), _name(rng, 64), n << 20) for n in (3, 70, 0, 200)]
    b = Batch(blobs)
    n = len(blobs)
    dev = D.DeviceBuffer(20 * n)
    assert b.run(out=dev) is dev
    pin = D.PinnedArray((n, 20), np.uint8)
    assert b.run(out=pin) is pin
    D.synchronize()
    from_dev = dev.to_host(np.uint8, 20 * n).reshape(n, 20)
    assert np.array_equal(from_dev, pin.a)
    b.check(from_dev, orc)
    pageable = np.zeros((n, 20), dtype=np.uint8)
    i64p, u64p = C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
    nbuf, noff = D.pack_names(b.names)
    rc = lib.krk_info_hash_batch_dev(b.pl.ctypes.data_as(i64p), b.sums.ptr, b.off.ctypes.data_as(u64p),
                                     b.ns.ctypes.data_as(u64p), nbuf, noff.ctypes.data_as(u64p),
                                     b.ln.ctypes.data_as(i64p), n, pageable.ctypes.data, None)
    assert rc == _capi.KRK_EINVAL
    assert not pageable.any()
    assert lib.krk_info_hash_batch_dev(None, None, None, None, None, None, None, 0, None, None) == _capi.KRK_OK


@pytest.mark.parametrize("lengths,piece", [
    ([0, 1, 4095, 4096, 4097, 10 * 4096 + 3], 4096),
    ([1 << 20], 1 << 18),
    ([(i * 7919) % 300_000 + 1 for i in range(37)], 1 << 16),
])
def test_metainfo_batch_gpu_placement(gpu, orc, lengths, piece):
    """The shapes of tests/test_gpu_metainfo_batch.py through device.metainfo_batch with the
    InfoHash placed on the device: equal to the HOST placement and to the oracle."""
    ids = [4000 + i for i in range(len(lengths))]
    arena = D.BlobArena(lengths, piece, blob_ids=ids)
    names = [f"{i:064x}" for i in ids]
    res = {}
    assert D.info_hash_placement() == _capi.KRK_PLACE_AUTO
    try:
        for place in (_capi.KRK_PLACE_AUTO, _capi.KRK_PLACE_GPU, _capi.KRK_PLACE_HOST):
            D.set_info_hash_placement(place)
            out = D.BatchOutputs(arena)
            sums_h = np.zeros(max(arena.total_pieces, 1), dtype=np.uint32)
            ih = D.metainfo_batch(arena, out, names, sums_h)
            want_place = _capi.KRK_PLACE_GPU if place == _capi.KRK_PLACE_GPU else _capi.KRK_PLACE_HOST
            assert D.metainfo_batch_last_placement() == want_place  # HOST by default (AUTO)
            dev = out.sums.to_host(np.uint32, max(arena.total_pieces, 1))
            assert np.array_equal(dev[:arena.total_pieces], sums_h[:arena.total_pieces])
            res[place] = (ih.copy(), sums_h)
        assert lib.krk_set_info_hash_placement(3) == _capi.KRK_EINVAL
        assert lib.krk_set_info_hash_placement(-1) == _capi.KRK_EINVAL
    finally:
        D.set_info_hash_placement(_capi.KRK_PLACE_AUTO)
    ih_gpu, sums_gpu = res[_capi.KRK_PLACE_GPU]
    for place in (_capi.KRK_PLACE_AUTO, _capi.KRK_PLACE_HOST):
        assert np.array_equal(res[place][0], ih_gpu) and np.array_equal(res[place][1], sums_gpu)
    for k, L in enumerate(lengths):
        want = [int(x) for x in orc.calc_piece_sums(orc.synth(ids[k], L), piece)[1]]
        o, c = int(arena.sums_off[k]), int(arena.n_pieces[k])
        assert sums_gpu[o:o + c].tolist() == want
        assert bytes(ih_gpu[k]) == orc.info_hash(piece, want, names[k], L)
