"""Stored MetaInfo re-pieced to a coarser piece length, the parts that need no device:
core.MetaInfo.Repiece against NewMetaInfo over the bytes, Generator.OverwriteMetaInfo with and
without a usable sidecar, and Generator.RepieceAll with its command line on a temporary DirCAS
against a RegenerateAll under the new config on a copy of the cache."""
import json
import os
import shutil

import numpy as np
import pytest

from kraken_amd import _capi, core, metainfogen
from kraken_amd._capi import check, lib
from tests.repiece_cache import KIB, NEW, OLD, SIZES, blob as _blob, build_cache as _build_cache, meta_path as _meta_path
from tests.repiece_cache import sidecars as _sidecars, zero_data as _zero_data


@pytest.fixture
def host_crc():
    """The CRC placement pinned to the host (what AUTO is without a device)."""
    check(lib.krk_set_crc_placement(_capi.KRK_PLACE_HOST))
    yield
    check(lib.krk_set_crc_placement(_capi.KRK_PLACE_AUTO))


def _same(a: core.MetaInfo, b: core.MetaInfo):
    assert (a.PieceLength(), a.Length(), a.NumPieces(), a.Digest()) == (b.PieceLength(), b.Length(), b.NumPieces(), b.Digest())
    assert np.array_equal(a.PieceSums(), b.PieceSums()) and (a._sums is None) == (b._sums is None)
    assert a.InfoHash() == b.InfoHash() and a.Serialize() == b.Serialize()


def test_metainfo_repiece_equals_newmetainfo(host_crc):
    P = 64
    for k in (1, 2, 3, 4, 64, 65):
        N = P * k
        for L in sorted({0, 1, P - 1, P, P + 1, N - 1, N, N + 1, 2 * N - 1, 2 * N, 2 * N + P + 1, 5 * N + 7}):
            data, d = _blob(7000 + L, L)
            mi = core.NewMetaInfo(d, data, P)
            _same(mi.Repiece(N), core.NewMetaInfo(d, data, N))
    data, d = _blob(1, 1000)
    mi = core.NewMetaInfo(d, data, P)
    _same(mi.Repiece(1 << 40), core.NewMetaInfo(d, data, 1 << 40))  # one sum: the blob's CRC-32
    _same(mi.Repiece(128).Repiece(1024), core.NewMetaInfo(d, data, 1024))
    for bad, text in ((96, "new piece length 96 is not a multiple of piece length 64"),
                      (32, "new piece length 32 is not a multiple of piece length 64"),
                      (0, "piece length must be positive"), (-64, "piece length must be positive")):
        with pytest.raises(ValueError) as e:
            mi.Repiece(bad)
        assert str(e.value) == text


def test_overwrite_metainfo_both_ways(tmp_path, host_crc):
    cas = metainfogen.DirCAS(str(tmp_path / "cache"))
    g = metainfogen.New(OLD, cas)
    data, d = _blob(42, 700_000)
    cas.WriteCacheFileAs(d, data)
    g.Generate(d)
    stored = core.DeserializeMetaInfo(cas.GetCacheFileMetadata(d.Hex()))
    assert stored.PieceLength() == 64 * KIB
    # the stored piece length divides the new one: re-pieced, the blob is not read
    _zero_data(cas, d.Hex())
    g.OverwriteMetaInfo(d, 256 * KIB)
    assert cas.GetCacheFileMetadata(d.Hex()) == core.NewMetaInfo(d, data, 256 * KIB).Serialize()
    # it does not: the blob is read, as the reference does (here: the zeros now in the file)
    g.OverwriteMetaInfo(d, 384 * KIB)
    assert cas.GetCacheFileMetadata(d.Hex()) == core.NewMetaInfo(d, bytes(len(data)), 384 * KIB).Serialize()
    # no sidecar, and a sidecar that does not describe the file: read
    cas.WriteCacheFileAs(d, data)
    os.remove(_meta_path(cas, d.Hex()))
    g.OverwriteMetaInfo(d, 128 * KIB)
    assert cas.GetCacheFileMetadata(d.Hex()) == core.NewMetaInfo(d, data, 128 * KIB).Serialize()
    other, _ = _blob(43, 700_000)
    cas.SetCacheFileMetadata(d.Hex(), core.NewMetaInfo(d, other[:-1], 64 * KIB))  # a wrong stored Length
    g.OverwriteMetaInfo(d, 128 * KIB)
    assert cas.GetCacheFileMetadata(d.Hex()) == core.NewMetaInfo(d, data, 128 * KIB).Serialize()
    # the reference's error prefixes
    with pytest.raises(IOError) as e:
        g.OverwriteMetaInfo(d, 0)
    assert str(e.value) == "create metainfo: piece length must be positive"
    with pytest.raises(IOError) as e:
        g.OverwriteMetaInfo(core.NewSHA256DigestFromHex("ab" * 32), 128 * KIB)
    assert str(e.value).startswith("get cache file: ")


def test_repiece_all_matches_regenerate_all(tmp_path, host_crc, capsys):
    root, ref_root, cli_root = (str(tmp_path / x) for x in ("cache", "ref", "cli"))
    cas, names = _build_cache(root)
    size_of = dict(zip(names, SIZES))
    # what RegenerateAll writes under the new config, on a copy of the cache
    shutil.copytree(root, ref_root)
    ref = metainfogen.DirCAS(ref_root)
    assert metainfogen.New(NEW, ref).RegenerateAll()["blobs"] == len(SIZES)
    want = _sidecars(ref)
    assert {core.DeserializeMetaInfo(v).PieceLength() for v in want.values()} == {256 * KIB, 1024 * KIB}
    # one sidecar missing, one with a wrong stored Length, one already at its target
    missing, wrong_len, at_target = names[4], names[7], names[10]
    os.remove(_meta_path(cas, missing))
    raw = json.loads(cas.GetCacheFileMetadata(wrong_len))
    raw["Info"]["Length"] += 1
    with open(_meta_path(cas, wrong_len), "wb") as f:
        f.write(json.dumps(raw, separators=(",", ":")).encode())
    with open(_meta_path(cas, at_target), "wb") as f:
        f.write(want[at_target])
    shutil.copytree(root, cli_root)
    # the re-pieced blobs' bytes are never read: zeros of the same size from here on
    repieced = [n for n in names if n not in (missing, wrong_len, at_target)]
    for n in repieced:
        _zero_data(cas, n)
    report = metainfogen.New(NEW, cas).RepieceAll()
    assert report == {"blobs": 12, "unchanged": 1, "repieced": 9, "reread": 2, "changed": 11,
                      "bytes_not_read": sum(size_of[n] for n in repieced + [at_target])}
    assert _sidecars(cas) == want
    # a second pass finds everything at its target and writes nothing
    again = metainfogen.New(NEW, cas).RepieceAll()
    assert again == {"blobs": 12, "unchanged": 12, "repieced": 0, "reread": 0, "changed": 0,
                     "bytes_not_read": sum(SIZES)}
    assert _sidecars(cas) == want
    # the command line: the same report and sidecars, exit code 0
    capsys.readouterr()
    assert metainfogen.main([cli_root, "--repiece", "--piece-lengths", "0:262144,524288:1048576"]) == 0
    assert json.loads(capsys.readouterr().out) == report
    assert _sidecars(metainfogen.DirCAS(cli_root)) == want
    # a change the stored piece lengths do not divide (256 KiB -> 384 KiB): every blob is reread
    third = {0: 384 * KIB}
    assert metainfogen.New(third, ref).RegenerateAll()["blobs"] == 12
    cli = metainfogen.DirCAS(cli_root)
    assert metainfogen.New(third, cli).RepieceAll() == {"blobs": 12, "unchanged": 0, "repieced": 0, "reread": 12,
                                                        "changed": 12, "bytes_not_read": 0}
    assert _sidecars(cli) == _sidecars(ref)
    with pytest.raises(ValueError):
        metainfogen.New(NEW, cli).RepieceAll(placement="tpu")
