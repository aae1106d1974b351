"""The _torrentmeta JSON codec on the device (metainfo_json.hip behind
krk_metainfo_serialize_batch_dev and krk_metainfo_parse_sums_batch_dev) against the host form and
the plain-Python restatement (tests/metainfo_json_ref.py), byte for byte: the sum-count / value /
header matrix, every destination and span alignment, the unit edges, buffers pre-filled with
canaries, 64-bit offsets, and Generator.RepieceAll(placement="gpu") as one device chain."""
import ctypes as C
import hashlib
import os
import shutil

import numpy as np
import pytest

from kraken_amd import _capi, core, device as D, metainfogen
from kraken_amd._capi import KRK_EINVAL, check, lib
from tests import metainfo_json_ref as R

pytestmark = pytest.mark.gpu

GAP = 24  # canary bytes between two documents' slots


def bound(n):
    return int(lib.krk_metainfo_json_bound(n))


def layout(cases, residues=(0, 1, 2, 3)):
    """(descriptor array, concatenated sums, out size): case i = (piece_length, sums or None, name,
    length), its slot GAP bytes after the one before at out_off % 4 == residues[i % len]."""
    n = len(cases)
    arr = (_capi.krk_metainfo_json_blob * n)()
    off = s_off = 0
    parts = []
    for i, (pl, sums, name, length) in enumerate(cases):
        k = 0 if sums is None else len(sums)
        off += GAP
        off += (residues[i % len(residues)] - off) % 4
        arr[i] = _capi.krk_metainfo_json_blob(s_off, k, pl, length, off, sums is None, 0, name.encode())
        if k:
            parts.append(np.asarray(sums, dtype=np.uint32))
        s_off += k + (i % 3)  # unused sums between two blobs' ranges
        if i % 3:
            parts.append(np.full(i % 3, 0x0BADBAD0, dtype=np.uint32))
        off += bound(k)
    return arr, np.concatenate(parts + [np.zeros(1, np.uint32)]), off + GAP


def serialize_dev(arr, sums, out_size, fill, pinned=False):
    """(out bytes, out_len) after one call into buffers pre-filled with `fill`."""
    n = len(arr)
    d_sums = D.DeviceBuffer(sums.nbytes)
    d_sums.from_host(sums)
    if pinned:
        out, lens = D.PinnedArray((out_size,), np.uint8), D.PinnedArray((n,), np.uint64)
        out.a[:] = fill
        lens.a.view(np.uint8)[:] = fill
    else:
        out, lens = D.DeviceBuffer(out_size), D.DeviceBuffer(8 * n)
        out.from_host(np.full(out_size, fill, np.uint8))
        lens.from_host(np.full(8 * n, fill, np.uint8))
    check(lib.krk_metainfo_serialize_batch_dev(arr, n, d_sums.ptr, out.ptr, lens.ptr, None))
    check(lib.krk_stream_sync(None))
    if pinned:
        return out.a.copy(), lens.a.copy()
    return out.to_host(np.uint8, out_size), lens.to_host(np.uint64, n)


def expect_image(arr, cases, out_size, fill):
    """The whole output buffer as it must look: the restatement's documents, `fill` elsewhere."""
    img = np.full(out_size, fill, np.uint8)
    lens = np.zeros(len(cases), np.uint64)
    for i, (pl, sums, name, length) in enumerate(cases):
        doc = R.serialize(pl, sums, name, length)
        o = int(arr[i].out_off)
        img[o:o + len(doc)] = np.frombuffer(doc, np.uint8)
        lens[i] = len(doc)
    return img, lens


@pytest.fixture(scope="module")
def cases():
    """The matrix, a no-piece blob between two with pieces, and 1,000 blobs of <= 3 sums."""
    out = R.matrix()
    out.insert(5, (7, None, R.NAME_LOWER, 0))
    out.insert(9, (7, np.zeros(0, np.uint32), R.NAME_UPPER, 0))
    rng = np.random.default_rng(7)
    for i in range(1000):
        k = i % 4
        out.append((1 << (i % 40), None if (k == 0 and i % 8) else R.sum_values("random", k, i), R.NAME_MIXED,
                    int(rng.integers(0, 1 << 40))))
    return out


@pytest.fixture(scope="module")
def matrix_run(gpu, cases):
    arr, sums, size = layout(cases)
    return arr, sums, size, expect_image(arr, cases, size, 0xA5), serialize_dev(arr, sums, size, 0xA5)


def test_serialize_matrix_every_byte_inside_and_nothing_outside(matrix_run):
    _, _, _, (img, want_len), (out, lens) = matrix_run
    assert np.array_equal(lens, want_len)
    bad = np.flatnonzero(out != img)
    assert bad.size == 0, bad[:8]


def test_serialize_second_run_into_ff_gives_the_same_documents(matrix_run, cases):
    arr, sums, size, _, (first, lens) = matrix_run
    out, lens2 = serialize_dev(arr, sums, size, 0xFF)
    img, _ = expect_image(arr, cases, size, 0xFF)
    assert np.array_equal(lens2, lens) and np.array_equal(out, img)


def test_serialize_equals_the_host_form(matrix_run, cases):
    arr, _, _, _, (out, lens) = matrix_run
    for i in range(0, len(cases), 7):
        doc = core.MetaInfo(cases[i][0], cases[i][1], cases[i][2], cases[i][3], None, None).Serialize()
        o = int(arr[i].out_off)
        assert out[o:o + int(lens[i])].tobytes() == doc


def test_serialize_every_destination_and_array_start_residue(gpu):
    """out_off % 4 over 0..3 crossed with header lengths that move the array's first byte over
    every residue; a few steps and a tail of sums each."""
    sums = R.sum_values("random", 70 + 64, 3)
    cs, res = [], []
    for r in range(4):
        for digits in range(1, 5):
            cs.append((10 ** digits - 1, sums[:70 + 16 * r], R.NAME_LOWER, r))
            res.append(r)
    arr, flat, size = layout(cs, residues=res)
    assert {(int(a.out_off) % 4, (int(a.out_off) + 23 + len(str(a.piece_length)) + 14) % 4) for a in arr} == {
        (x, y) for x in range(4) for y in range(4)}
    out, lens = serialize_dev(arr, flat, size, 0xA5)
    img, want_len = expect_image(arr, cs, size, 0xA5)
    assert np.array_equal(lens, want_len) and np.array_equal(out, img)


def test_serialize_into_page_locked_host_memory_and_pageable_refused(gpu, cases):
    sub = cases[:40]
    arr, sums, size = layout(sub)
    out, lens = serialize_dev(arr, sums, size, 0xA5, pinned=True)
    img, want_len = expect_image(arr, sub, size, 0xA5)
    assert np.array_equal(lens, want_len) and np.array_equal(out, img)
    d_sums = D.DeviceBuffer(sums.nbytes)
    d_lens = D.DeviceBuffer(8 * len(arr))
    pageable = np.full(size, 0xA5, np.uint8)
    with D.KernelTimer():
        rc = lib.krk_metainfo_serialize_batch_dev(arr, len(arr), d_sums.ptr, pageable.ctypes.data, d_lens.ptr, None)
        D.synchronize()
        assert rc == KRK_EINVAL and D.KernelTimer.stats("metainfo_serialize")[0] == 0
        spans = (_capi.krk_metainfo_json_span * 1)(_capi.krk_metainfo_json_span(0, 1, 0, 1))
        rc = lib.krk_metainfo_parse_sums_batch_dev(spans, 1, d_sums.ptr, pageable.ctypes.data, d_lens.ptr, None)
        assert rc == KRK_EINVAL and D.KernelTimer.stats("metainfo_parse")[0] == 0
    assert (pageable == 0xA5).all()


def test_serialize_one_c4_sized_blob_and_parse_it_back(gpu):
    sums = np.random.default_rng(20261020).integers(0, 1 << 32, size=81_920, dtype=np.uint64).astype(np.uint32)
    cs = [(256 << 10, sums, R.NAME_LOWER, 81_920 * (256 << 10) - 12_345)]
    arr, flat, size = layout(cs)
    out, lens = serialize_dev(arr, flat, size, 0xA5)
    img, want_len = expect_image(arr, cs, size, 0xA5)
    assert np.array_equal(lens, want_len) and np.array_equal(out, img)
    o = int(arr[0].out_off)
    doc = out[o:o + int(lens[0])].tobytes()
    a, b = R.bracket_span(doc)
    got, status = parse_dev([(doc[a:b], 81_920)])
    assert status[0] == 0 and np.array_equal(got[0], sums)


def test_serialize_offsets_straddling_2_to_the_32(gpu):
    """One blob whose document lies across out + 2^32 and one whose sums lie across byte 2^32 of
    sums_dev, in buffers allocated large and touched only there."""
    big = (1 << 32) + (1 << 16)
    sums = R.sum_values("random", 600, 5)
    o0, o1 = (1 << 32) - 1001, 64
    s0, s1 = 16, (1 << 30) - 250
    arr = (_capi.krk_metainfo_json_blob * 2)(
        _capi.krk_metainfo_json_blob(s0, 300, 4, 9, o0, 0, 0, R.NAME_LOWER.encode()),
        _capi.krk_metainfo_json_blob(s1, 600, 5, 10, o1, 0, 0, R.NAME_UPPER.encode()))
    d_sums, d_out, d_len = D.DeviceBuffer(big), D.DeviceBuffer(big), D.DeviceBuffer(16)
    d_sums.from_host(sums[:300], 4 * s0)
    d_sums.from_host(sums, 4 * s1)
    lo0, lo1, win = o0 - 4096, 0, 16384
    d_out.from_host(np.full(win, 0xA5, np.uint8), lo0)
    d_out.from_host(np.full(win, 0xA5, np.uint8), lo1)
    check(lib.krk_metainfo_serialize_batch_dev(arr, 2, d_sums.ptr, d_out.ptr, d_len.ptr, None))
    check(lib.krk_stream_sync(None))
    lens = d_len.to_host(np.uint64, 2)
    for (lo, o, doc) in ((lo0, o0, R.serialize(4, sums[:300], R.NAME_LOWER, 9)),
                         (lo1, o1, R.serialize(5, sums, R.NAME_UPPER, 10))):
        img = np.full(win, 0xA5, np.uint8)
        img[o - lo:o - lo + len(doc)] = np.frombuffer(doc, np.uint8)
        assert np.array_equal(d_out.to_host(np.uint8, win, lo), img)
    assert lens.tolist() == [len(R.serialize(4, sums[:300], R.NAME_LOWER, 9)), len(R.serialize(5, sums, R.NAME_UPPER, 10))]
    assert o0 < (1 << 32) < o0 + int(lens[0]) and 4 * s1 < (1 << 32) < 4 * (s1 + 600)
    for b in (d_sums, d_out, d_len):
        b.free()


# ------------------------------------------------------------------ parse
CANARY = 0x5AFEC0DE


def parse_dev(items, fill=0xA5, pad=5):
    """items: [(span bytes, expect_n)].  Span i starts at text_off % 16 == i % 16; the blobs' sum
    ranges are `pad` canary words apart.  ([expect_n sums of each blob], status), after checking
    the canaries."""
    n = len(items)
    arr = (_capi.krk_metainfo_json_span * n)()
    text = bytearray()
    s_off = pad
    for i, (span, expect_n) in enumerate(items):
        text += b"#" * ((i - len(text)) % 16)
        arr[i] = _capi.krk_metainfo_json_span(len(text), len(span), s_off, expect_n)
        text += span
        s_off += expect_n + pad
    text += b"#"
    d_text, d_sums, d_st = D.DeviceBuffer(len(text)), D.DeviceBuffer(4 * s_off), D.DeviceBuffer(4 * n)
    d_text.from_host(np.frombuffer(bytes(text), np.uint8))
    d_sums.from_host(np.full(s_off, CANARY, np.uint32))
    d_st.from_host(np.full(4 * n, fill, np.uint8))
    check(lib.krk_metainfo_parse_sums_batch_dev(arr, n, d_text.ptr, d_sums.ptr, d_st.ptr, None))
    check(lib.krk_stream_sync(None))
    sums, status = d_sums.to_host(np.uint32, s_off), d_st.to_host(np.uint32, n)
    out, at = [], 0
    for a in arr:
        assert (sums[at:int(a.sums_off)] == CANARY).all()  # the words between two blobs' ranges
        out.append(sums[int(a.sums_off):int(a.sums_off) + int(a.expect_n)])
        at = int(a.sums_off) + int(a.expect_n)
    assert (sums[at:] == CANARY).all()
    return out, status


def test_parse_round_trips_the_matrix_at_every_span_alignment(gpu, cases):
    sub = [c for c in cases[:120] if c[1] is not None]
    items = []
    for pl, sums, name, length in sub:
        doc = R.serialize(pl, sums, name, length)
        a, b = R.bracket_span(doc)
        items.append((doc[a:b], len(sums)))
    assert len(items) >= 64
    got, status = parse_dev(items)
    assert not status.any()
    for (pl, sums, *_), g in zip(sub, got):
        assert np.array_equal(g, np.asarray(sums, dtype=np.uint32))
    got2, status2 = parse_dev(items, fill=0xFF)  # a second call into 0xFF gives the same
    assert not status2.any() and all(np.array_equal(x, y) for x, y in zip(got, got2))


def test_parse_ten_digit_number_at_every_phase_of_a_unit_edge(gpu):
    _, unit = R.geometry()
    items, want = [], []
    for k in range(0, 11):
        head = b"7," * ((unit - k) // 2)
        if (unit - k) % 2:
            head = b"1" + head  # 17,7,7,...
        assert len(head) == unit - k
        span = head + b"4294967295,12,0"
        vals = [int(x) for x in span.split(b",")]
        items.append((span, len(vals)))
        want.append(vals)
        if k == 10:  # the span ends with the number, exactly on the unit edge
            span = head + b"4294967295"
            assert len(span) == unit
            items.append((span, len(vals) - 2))
            want.append(vals[:-2])
    items.append((b"", 0))  # [] with expect_n == 0
    want.append([])
    got, status = parse_dev(items)
    assert not status.any()
    for g, w in zip(got, want):
        assert g.tolist() == w


REFUSALS = {
    "leading zero": (b"1,02,3", 3),
    "2^32": (b"1,4294967296,3", 3),
    "11 digits": (b"1,10000000000,3", 3),
    "double comma": (b"1,,3", 3),
    "leading comma": (b",1,2", 3),
    "trailing comma": (b"1,2,", 3),
    "space": (b"1, 2,3", 3),
    "negative": (b"-1,2,3", 3),
    "1.0": (b"1.0,2,3", 3),
    "1e3": (b"1e3,2,3", 3),
    "one too few": (b"1,2", 3),
    "one too many": (b"1,2,3,4", 3),
    "empty for three": (b"", 3),
    "one for none": (b"0", 0),
}


def test_parse_refusals_next_to_valid_neighbours(gpu):
    _, unit = R.geometry()
    good = (b"10,20,30," * (unit // 9 + 3))[:-1]
    good_vals = [int(x) for x in good.split(b",")]
    items = [(good, len(good_vals))]
    for case in REFUSALS.values():
        items += [case, (good, len(good_vals))]
    got, status = parse_dev(items)
    for i, name in enumerate(REFUSALS):
        assert status[2 * i + 1] != 0, name
    for i in range(0, len(items), 2):
        assert status[i] == 0 and got[i].tolist() == good_vals


# ------------------------------------------------------------------ the chain
MIB = 1 << 20
CHAIN_OLD, CHAIN_NEW = {0: MIB}, {0: 4 * MIB}
CHAIN_SIZES = (0, 1, 4 * MIB - 1, 4 * MIB, 4 * MIB + 1, 9 * MIB + 3, 2 * MIB + 5, 3 * MIB, 5 * MIB)


def test_repiece_all_is_one_device_chain_equal_to_host_and_regenerate_all(gpu, tmp_path):
    roots = {k: str(tmp_path / k) for k in ("gpu", "host", "regen")}
    cas = metainfogen.DirCAS(roots["gpu"])
    names = []
    for k, size in enumerate(CHAIN_SIZES):
        data = np.random.default_rng(500 + k).integers(0, 256, size=size, dtype=np.uint8).tobytes()
        d = core.NewSHA256DigestFromHex(hashlib.sha256(data).hexdigest())
        cas.WriteCacheFileAs(d, data)
        names.append(d.Hex())
    assert metainfogen.New(CHAIN_OLD, cas).RegenerateAll() == {"blobs": 9, "changed": 9}
    # one sidecar with whitespace (valid, not canonical), one truncated, one missing
    meta = lambda name: cas.GetCacheFilePath(name)[:-len("data")] + "_torrentmeta"
    ws = cas.GetCacheFileMetadata(names[6])
    open(meta(names[6]), "wb").write(ws.replace(b",", b", ").replace(b":", b": ", 1) + b"\n")
    assert core.DeserializeMetaInfo(cas.GetCacheFileMetadata(names[6])).Serialize() == ws
    open(meta(names[7]), "wb").write(cas.GetCacheFileMetadata(names[7])[:50])
    os.remove(meta(names[8]))
    shutil.copytree(roots["gpu"], roots["host"])
    shutil.copytree(roots["gpu"], roots["regen"])
    with D.KernelTimer():
        report = metainfogen.New(CHAIN_NEW, cas).RepieceAll(placement="gpu")
        D.synchronize()
        for kernel in ("metainfo_parse", "piece_repiece", "info_hash", "metainfo_serialize"):
            assert D.KernelTimer.stats(kernel)[0] == 1, kernel
    assert report == {"blobs": 9, "unchanged": 0, "repieced": 7, "reread": 2, "changed": 9,
                      "bytes_not_read": sum(CHAIN_SIZES[:7])}
    host = metainfogen.DirCAS(roots["host"])
    assert metainfogen.New(CHAIN_NEW, host).RepieceAll(placement="host") == report
    regen = metainfogen.DirCAS(roots["regen"])
    assert metainfogen.New(CHAIN_NEW, regen).RegenerateAll() == {"blobs": 9, "changed": 9}
    side = lambda c: {n: c.GetCacheFileMetadata(n) for n in c.ListNames()}
    want = side(regen)
    assert len(want) == 9 and side(cas) == want and side(host) == want
