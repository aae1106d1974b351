"""Blobs against their stored MetaInfo, the parts that need no device: the host bitfield packer
(krk_bitfield_words, krk_piece_bitfield -- willf/bitset words as Torrent.Bitfield() returns them,
lib/torrent/storage/agentstorage/torrent.go:130-140), krk_verify_files on the HOST CRC
placement, agentstorage.Torrent.Recheck and metainfogen.Generator.VerifyAll with its command
line.  Expected sums come from the oracle, bitfields from numpy.packbits."""
import ctypes as C
import shutil

import numpy as np
import pytest

from kraken_amd import _capi, agentstorage, core, device as D, metainfogen
from kraken_amd._capi import check, lib
from tests import verify_cache as VC

u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


@pytest.fixture
def host_crc():
    """The CRC placement of the file calls pinned to the host (what AUTO is without a device)."""
    check(lib.krk_set_crc_placement(_capi.KRK_PLACE_HOST))
    yield
    check(lib.krk_set_crc_placement(_capi.KRK_PLACE_AUTO))


def test_bitfield_words():
    for n, want in [(0, 0), (1, 1), (63, 1), (64, 1), (65, 2), ((1 << 32) + 1, (1 << 26) + 1)]:
        assert lib.krk_bitfield_words(n) == want, n


def _bad_sets(n):
    edges = [p for p in (0, 63, 64, n - 1) if 0 <= p < n]
    sets = [set(), set(range(n)), set(edges)] + [{p} for p in edges]
    return [s for k, s in enumerate(sets) if s not in sets[:k]]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 128, 129])
def test_piece_bitfield_matches_numpy(n):
    rng = np.random.default_rng(1000 + n)
    expected = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    words = (n + 63) // 64
    for bad in _bad_sets(n):
        sums = expected.copy()
        for p in bad:
            sums[p] ^= 1 << (p % 32)
        bits = np.full(words + 1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)  # one guard word behind
        n_bad = C.c_uint32(0xFFFFFFFF)
        check(lib.krk_piece_bitfield(sums.ctypes.data_as(u32p) if n else None, expected.ctypes.data_as(u32p) if n else None,
                                     n, bits.ctypes.data_as(u64p), C.byref(n_bad)))
        ok = np.ones(n, dtype=bool)
        ok[sorted(bad)] = False
        assert np.array_equal(bits[:words], VC.ref_words(ok)), (n, sorted(bad))
        assert bits[words] == 0xFFFFFFFFFFFFFFFF and n_bad.value == len(bad), (n, sorted(bad))
        got_bits, got_bad = D.piece_bitfield(sums, expected)
        assert np.array_equal(got_bits, bits[:words]) and got_bad == len(bad)
        assert np.array_equal(D.bitfield_bools(got_bits, n), ok)


def test_piece_bitfield_refuses_null():
    bits = np.zeros(1, dtype=np.uint64)
    assert lib.krk_piece_bitfield(None, None, 3, bits.ctypes.data_as(u64p), None) == _capi.KRK_EINVAL


def test_verify_batch_dev_without_a_device():
    """An empty batch is KRK_OK anywhere; a real one needs a gfx950 device (KRK_ENODEV here
    when there is none -- with one, tests/test_gpu_verify.py runs it)."""
    assert lib.krk_verify_batch_dev(None, 0, None, None, None, None, None, None) == _capi.KRK_OK
    if D.device_count() == 0:
        blob = _capi.krk_blob(None, 0, 1, 0)
        bad = C.c_uint32()
        rc = lib.krk_verify_batch_dev(C.byref(blob), 1, None, None, None, C.byref(bad), None, None)
        assert rc == _capi.KRK_ENODEV


def test_verify_files_host_placement_matches_oracle(orc, tmp_path, host_crc):
    P = 1000
    lens = [0, 1, 999, 1000, 1001, 64 * P, 64 * P + 1, 130 * P + 7, 0, 3 * P]  # empty files, short last pieces
    datas = [orc.synth(9100 + i, L) for i, L in enumerate(lens)]
    paths = []
    for i, d in enumerate(datas):
        paths.append(str(tmp_path / f"f{i}"))
        with open(paths[-1], "wb") as f:
            f.write(memoryview(d))
    sums = [np.asarray(orc.calc_piece_sums(d, P)[1], dtype=np.uint32) if d.size else np.zeros(0, np.uint32)
            for d in datas]
    counts = [s.size for s in sums]
    assert counts == [0, 1, 1, 1, 2, 64, 65, 131, 0, 3]
    bad = {1: [0], 5: [0, 63], 6: [63, 64], 7: [0, 63, 64, 130], 9: [1]}
    expected = [s.copy() for s in sums]
    for i, ps in bad.items():
        for p in ps:
            expected[i][p] ^= 0x80000000
    bits, woff, n_bad, ok = D.verify_files(paths, lens, P, np.concatenate(expected))
    assert ok is None
    assert woff.tolist() == np.concatenate([[0], np.cumsum([(c + 63) // 64 for c in counts])]).tolist()
    for i, c in enumerate(counts):
        good = np.ones(c, dtype=bool)
        good[bad.get(i, [])] = False
        assert np.array_equal(bits[int(woff[i]):int(woff[i + 1])], VC.ref_words(good)), i
        assert n_bad[i] == len(bad.get(i, [])), i
    g, h, _ = D.crc_host_split()
    assert g == 0 and h == sum(lens)  # the split krk_piece_sums_files reports still holds
    # all good, straight through the C ABI into 0xFF-filled outputs
    n = len(paths)
    arr = (_capi.krk_file_blob * n)()
    off = 0
    for i in range(n):
        arr[i] = _capi.krk_file_blob(paths[i].encode(), lens[i], P, off)
        off += counts[i]
    allsums = np.concatenate(sums)
    bits2 = np.full(int(woff[-1]) + 1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    bad2 = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    check(lib.krk_verify_files(arr, n, allsums.ctypes.data_as(u32p), None, bits2.ctypes.data_as(u64p),
                               bad2.ctypes.data_as(u32p), None))
    assert not bad2.any() and bits2[-1] == 0xFFFFFFFFFFFFFFFF
    for i, c in enumerate(counts):
        assert np.array_equal(bits2[int(woff[i]):int(woff[i + 1])], VC.ref_words(np.ones(c, dtype=bool))), i
    # the underlying call's errors: a file shorter than stat-ed, digest_ok without digests
    with pytest.raises(_capi.KrakenError) as e:
        D.verify_files([paths[3]], [1010], P, np.zeros(2, np.uint32))
    assert e.value.code == _capi.KRK_EIO and str(e.value).endswith(f"read blob: {paths[3]}: unexpected EOF")
    ok8 = np.zeros(n, dtype=np.uint8)
    rc = lib.krk_verify_files(arr, n, allsums.ctypes.data_as(u32p), None, bits2.ctypes.data_as(u64p),
                              bad2.ctypes.data_as(u32p), ok8.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert rc == _capi.KRK_EINVAL


def test_torrent_recheck_finds_exactly_the_written_pieces(orc, tmp_path, host_crc):
    P, n = 64, 130
    L = (n - 1) * P + 17
    data = orc.synth(20240607, L)
    sums = np.asarray(orc.calc_piece_sums(data, P)[1], dtype=np.uint32)
    assert sums.size == n
    name = orc.sha256(data).hex()
    mi = core.MetaInfo(P, sums, name, L, core.NewSHA256DigestFromHex(name), core._info_hash(P, sums, name, L))
    written = {0, 63, 64, 129, 5, 77, 100}
    # an unwritten piece is zero bytes in the download file: none may verify by accident
    for pi in set(range(n)) - written:
        assert sums[pi] != orc.crc32(bytes(mi.GetPieceLength(pi))), pi
    t = agentstorage.Torrent(mi, str(tmp_path / "download"))
    assert not t.complete.any()
    with open(t.path, "r+b") as f:
        for pi in written:
            f.seek(pi * P)
            f.write(memoryview(data[pi * P:pi * P + mi.GetPieceLength(pi)]))
    got = t.Recheck()
    assert got.dtype == bool and got.shape == (n,) and got is t.complete
    assert set(np.flatnonzero(t.complete).tolist()) == written
    assert not t.Complete()
    with pytest.raises(agentstorage.ErrPieceComplete):  # the rechecked status is the torrent's own
        t.WritePiece(data[:P], 0)


def test_verify_all_reports_every_case_and_writes_nothing(orc, tmp_path, host_crc, capsys):
    """check_digest=True needs a device (krk_metainfo_digest_files), so the digest reason is
    covered in tests/test_gpu_verify.py; here the sidecar regenerated over rotten bytes passes,
    which is exactly why the digest pass exists."""
    root = str(tmp_path / "cache")
    cas, names = VC.build_cache(orc, root)
    before = VC.snapshot(root)
    g = metainfogen.New(VC.CONFIG, cas)
    VC.check_report(g.VerifyAll(check_digest=False), names, check_digest=False)
    # batches of one blob give the same report
    VC.check_report(g.VerifyAll(batch_bytes=1, check_digest=False), names, check_digest=False)
    # a config that disagrees with the sidecars changes nothing: the STORED piece length is used
    VC.check_report(metainfogen.New({0: 4096}, cas).VerifyAll(check_digest=False), names, check_digest=False)
    capsys.readouterr()
    assert metainfogen.main([root, "--verify", "--no-digest"]) == 1
    import json
    VC.check_report(json.loads(capsys.readouterr().out), names, check_digest=False)
    assert VC.snapshot(root) == before  # every file's bytes and mtime
    clean = str(tmp_path / "clean")
    cas2, names2 = VC.build_cache(orc, clean, only_good=True)
    before2 = VC.snapshot(clean)
    assert metainfogen.main([clean, "--verify", "--no-digest"]) == 0
    assert json.loads(capsys.readouterr().out) == {"blobs": 6, "ok": 6, "corrupt": []}
    assert VC.snapshot(clean) == before2
    shutil.rmtree(clean)
