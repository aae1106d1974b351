"""Blobs against their stored MetaInfo on the device: krk_verify_batch_dev (piece_bitfield.hip:
one wave ballots 64 consecutive pieces of one blob into one willf/bitset word, as
Torrent.Bitfield() answers, lib/torrent/storage/agentstorage/torrent.go:130-140; with digests
the SHA-256 of uploader.verify compared too), krk_verify_files through the windows, and
Generator.VerifyAll with its digest pass.  Expected sums and digests come from the oracle,
bitfields from numpy.packbits."""
import ctypes as C
import json

import numpy as np
import pytest

from kraken_amd import _capi, device as D, metainfogen
from kraken_amd._capi import check, lib
from tests import verify_cache as VC

pytestmark = pytest.mark.gpu

u8p, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
P = 48
PIECES = [0, 1, 63, 64, 65, 127, 128, 129, 513, 1]
SHORT = {1, 3, 5, 7, 9}  # these end in a 7-byte piece


def _edges(n):
    return sorted({p for p in (0, 63, 64, n - 1) if 0 <= p < n})


@pytest.fixture(scope="module")
def edge(gpu, orc):
    """The edge batch in HBM (blobs 3 bytes off the arena's alignment, so no piece starts
    aligned) and the oracle's sums and digests of it."""
    lens = [n * P if i not in SHORT else (n - 1) * P + 7 for i, n in enumerate(PIECES)]
    assert 50_000 < sum(lens) < 60_000
    ids = [7700 + i for i in range(len(lens))]
    arena = D.BlobArena(lens, P, blob_ids=ids, misalign=3)
    assert arena.n_pieces.tolist() == PIECES
    datas = [orc.synth(b, L) for b, L in zip(ids, lens)]
    sums = np.concatenate([np.asarray(orc.calc_piece_sums(d, P)[1], dtype=np.uint32) if d.size
                           else np.zeros(0, np.uint32) for d in datas])
    digests = np.frombuffer(b"".join(orc.sha256(d) for d in datas), dtype=np.uint8).reshape(-1, 32)
    sums.setflags(write=False)
    digests.setflags(write=False)
    return arena, sums, digests


def _want(arena, bad_of):
    """(words, n_bad) for {blob: bad pieces} from numpy alone."""
    words, n_bad = [], []
    for i, n in enumerate(arena.n_pieces.tolist()):
        ok = np.ones(n, dtype=bool)
        ok[bad_of.get(i, [])] = False
        words.append(VC.ref_words(ok))
        n_bad.append(n - int(ok.sum()))
    return np.concatenate(words), np.asarray(n_bad, dtype=np.uint32)


@pytest.mark.parametrize("pinned", [False, True], ids=["device_out", "host_alloc_out"])
def test_edge_batch_every_word_count_and_flag(edge, pinned):
    arena, sums, digests = edge
    n = len(PIECES)
    so = arena.sums_off.astype(np.int64)
    bad_of = {i: _edges(c) for i, c in enumerate(PIECES) if c}
    expected = sums.copy()
    for i, ps in bad_of.items():
        expected[so[i] + np.asarray(ps)] ^= 0x00010000
    exp_dg = digests.copy()
    exp_dg[2, 31] ^= 1
    exp_dg[8, 0] ^= 0x80
    want_dg = np.ones(n, dtype=bool)
    want_dg[[2, 8]] = False  # the empty blob's digest (blob 0) verifies
    out = D.VerifyOutputs(arena, digests=True, pinned=pinned)
    assert out.words == sum((c + 63) // 64 for c in PIECES)
    cases = [(expected, exp_dg, _want(arena, bad_of), want_dg),
             (sums, digests, _want(arena, {}), np.ones(n, dtype=bool)),
             (~sums, ~digests, _want(arena, {i: list(range(c)) for i, c in enumerate(PIECES)}), np.zeros(n, dtype=bool))]
    for exp, dg, (want_bits, want_bad), want_ok in cases:
        out.fill(0xFF)  # the call writes every word, count and flag itself
        assert D.verify_batch(arena, exp, dg, out=out) is out
        D.synchronize()
        bits, n_bad, ok = out.to_host()
        assert np.array_equal(bits, want_bits)
        assert np.array_equal(n_bad, want_bad)
        assert np.array_equal(ok, want_ok)
    # without digests: the piece-sum pass alone, the same words
    bits, n_bad, ok = D.verify_batch(arena, expected)
    assert ok is None and np.array_equal(bits, cases[0][2][0]) and np.array_equal(n_bad, cases[0][2][1])


def test_many_small_blobs_one_word_each(gpu, orc):
    """5,000 blobs of 1-3 pieces of 16 bytes: every word belongs to another blob."""
    rng = np.random.default_rng(5000)
    n = 5000
    counts = rng.integers(1, 4, n)
    lens = counts * 16 - rng.integers(0, 16, n)  # a short last piece on most
    arena = D.BlobArena(lens, 16, fill=False)
    assert np.array_equal(arena.n_pieces, counts.astype(np.uint64))
    host = rng.integers(0, 256, arena.nbytes, dtype=np.uint8)
    arena.buf.from_host(host)
    sums = np.concatenate([np.asarray(orc.calc_piece_sums(host[int(o):int(o) + int(L)], 16)[1], dtype=np.uint32)
                           for o, L in zip(arena.offsets, lens)])
    expected = sums.copy()
    bad = rng.random(sums.size) < 0.07
    expected[bad] ^= 0xA5
    bits, n_bad, ok = D.verify_batch(arena, expected)
    assert ok is None and bits.size == n
    good = ~bad
    so = arena.sums_off.astype(np.int64)
    want_bits = np.zeros(n, dtype=np.uint64)
    for k in range(3):
        has = counts > k
        want_bits[has] |= good[so[has] + k].astype(np.uint64) << np.uint64(k)
    assert np.array_equal(bits, want_bits)
    assert np.array_equal(bits, np.concatenate([VC.ref_words(good[so[i]:so[i] + counts[i]]) for i in range(n)]))
    assert np.array_equal(n_bad, np.add.reduceat(bad.astype(np.uint32), so).astype(np.uint32))


def test_agrees_with_the_one_blob_path(edge):
    arena, sums, _ = edge
    i, c = 8, 513
    o = int(arena.sums_off[i])
    expected = sums.copy()
    expected[o + np.asarray([0, 63, 64, 200, 511, 512])] ^= 2
    blob = _capi.krk_blob(arena.buf.ptr + int(arena.offsets[i]), int(arena.lengths[i]), P, 0)
    exp_i = np.ascontiguousarray(expected[o:o + c])
    ok = np.zeros(c, dtype=np.uint8)
    check(lib.krk_verify_pieces_dev(C.byref(blob), exp_i.ctypes.data_as(u32p), ok.ctypes.data_as(u8p), None))
    assert int(c - ok.sum()) == 6
    bits, n_bad, _ = D.verify_batch(arena, expected)
    w = int(D.bitfield_offsets(arena.n_pieces)[i])
    assert np.array_equal(bits[w:w + 9], VC.ref_words(ok.astype(bool)))
    assert n_bad.tolist() == [0] * 8 + [6, 0]


def test_refusals_before_any_launch(edge):
    arena, sums, digests = edge
    n = len(PIECES)
    out = D.VerifyOutputs(arena, digests=True)
    out.fill(0xFF)
    pageable = np.full(out.words, 0x1111111111111111, dtype=np.uint64)
    with D.KernelTimer():
        rc = lib.krk_verify_batch_dev(arena.blob_structs(), n, sums.ctypes.data_as(u32p), None, pageable.ctypes.data,
                                      out.n_bad.ptr, None, None)
        assert rc == _capi.KRK_EINVAL and b"page-locked" in lib.krk_last_error()
        rc = lib.krk_verify_batch_dev(arena.blob_structs(), n, sums.ctypes.data_as(u32p), digests.ctypes.data_as(u8p),
                                      out.bits.ptr, out.n_bad.ptr, None, None)
        assert rc == _capi.KRK_EINVAL and b"digest_ok_out" in lib.krk_last_error()
        D.synchronize()
        for k in ("piece_bitfield", "crc32_pieces", "sha256_multi"):
            assert D.KernelTimer.stats(k)[0] == 0, k  # nothing ran
    assert (pageable == 0x1111111111111111).all()
    bits, n_bad, ok = out.to_host()
    assert (bits == 0xFFFFFFFFFFFFFFFF).all() and (n_bad == 0xFFFFFFFF).all()
    assert lib.krk_verify_batch_dev(None, 0, None, None, None, None, None, None) == _capi.KRK_OK


def test_files_through_the_windows_with_digests(gpu, orc, tmp_path):
    """The suite's CRC placement is the GPU (conftest): with digests the files go through the
    pinned windows and both kernels, without them through krk_piece_sums_files' GPU pass."""
    PL = 65536
    lens = [0, 1, 4095, 65536, 65537, 200_000, 1 << 20, (1 << 20) + 1, 3 * (1 << 20) + 5, 700_001, 64 * 65536, 2_500_000]
    datas = [orc.synth(9900 + i, L) for i, L in enumerate(lens)]
    sums = [np.asarray(orc.calc_piece_sums(d, PL)[1], dtype=np.uint32) if d.size else np.zeros(0, np.uint32) for d in datas]
    digests = np.frombuffer(b"".join(orc.sha256(d) for d in datas), dtype=np.uint8).reshape(-1, 32).copy()
    flips = {6: (1 << 20) - 1, 10: 63 * 65536}  # file -> flipped byte: the last piece of each
    paths = []
    for i, d in enumerate(datas):
        d = d.copy()
        if i in flips:
            d[flips[i]] ^= 1
        paths.append(str(tmp_path / f"v{i}"))
        with open(paths[-1], "wb") as f:
            f.write(memoryview(d))
    digests[3, 7] ^= 0x10  # a wrong name for intact bytes
    want_ok = np.ones(len(lens), dtype=bool)
    want_ok[[3, 6, 10]] = False
    want_bits, want_bad = [], []
    for i, s in enumerate(sums):
        ok = np.ones(s.size, dtype=bool)
        if i in flips:
            ok[flips[i] // PL] = False
        want_bits.append(VC.ref_words(ok))
        want_bad.append(int((~ok).sum()))
    want_bits = np.concatenate(want_bits)
    bits, woff, n_bad, ok = D.verify_files(paths, lens, PL, np.concatenate(sums), digests)
    assert D.windows_last_call()["windows"] >= 1
    assert np.array_equal(bits, want_bits) and n_bad.tolist() == want_bad and np.array_equal(ok, want_ok)
    assert int(woff[-1]) == want_bits.size
    bits2, _, n_bad2, ok2 = D.verify_files(paths, lens, PL, np.concatenate(sums))
    g, h, _ = D.crc_host_split()
    assert ok2 is None and g == sum(lens) and h == 0
    assert np.array_equal(bits2, want_bits) and n_bad2.tolist() == want_bad


def test_verify_all_with_the_digest_pass(gpu, orc, tmp_path, capsys):
    root = str(tmp_path / "cache")
    cas, names = VC.build_cache(orc, root)
    before = VC.snapshot(root)
    g = metainfogen.New(VC.CONFIG, cas)
    VC.check_report(g.VerifyAll(), names, check_digest=True)
    VC.check_report(g.VerifyAll(batch_bytes=1), names, check_digest=True)
    capsys.readouterr()
    assert metainfogen.main([root, "--verify"]) == 1
    VC.check_report(json.loads(capsys.readouterr().out), names, check_digest=True)
    assert VC.snapshot(root) == before
    clean = str(tmp_path / "clean")
    VC.build_cache(orc, clean, only_good=True)
    assert metainfogen.main([clean, "--verify"]) == 0
    assert json.loads(capsys.readouterr().out) == {"blobs": 6, "ok": 6, "corrupt": []}
