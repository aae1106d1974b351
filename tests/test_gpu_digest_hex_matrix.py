"""GPU parity: the digest hex kernels (digest_hex.hip) at their lane, wave and workgroup edges and
at every text alignment through krk_digest_parse_hex_dev / krk_digest_format_hex_dev -- digests,
status words and the valid bitset against the plain-Python transcription of the contract (the
cases and the comparison live in tests/digest_hex_matrix.py; tests/test_digest_hex_matrix_cpu.py
proves them on the host forms); the round trip; a name that straddles the 4 GiB line of its text;
and the pointer refusals."""
import ctypes as C

import numpy as np
import pytest

from kraken_amd import _capi, device as D
from kraken_amd._capi import check, lib
from tests import digest_hex_matrix as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def data():
    return M.Data()


def test_parse_every_shape_lead_and_listing_in_device_memory(gpu, data):
    calls, bad = M.run_parse(M.DeviceBackend(data), M.cases())
    assert calls > 0 and bad == [], f"{len(bad)} mismatches of {calls} calls, first {bad[:5]}"


def test_parse_into_page_locked_memory(gpu, data):
    calls, bad = M.run_parse(M.DeviceBackend(data, pinned=True), M.cases((0, 65, M.G + 1, M.N_MAX)))
    assert calls > 0 and bad == [], f"first {bad[:5]}"


def test_text_one_byte_past_an_aligned_base_and_digests_at_an_odd_address(gpu, data):
    calls, bad = M.run_parse(M.DeviceBackend(data, text_shift=1, out_shift=1), M.cases((65, M.G + 1, M.N_MAX)))
    assert calls > 0 and bad == [], f"first {bad[:5]}"


def test_format_every_shape_and_the_round_trip(gpu, data):
    for b in (M.DeviceBackend(data), M.DeviceBackend(data, text_shift=1, out_shift=3),
              M.DeviceBackend(data, pinned=True)):
        calls, bad = M.run_format(b)
        assert calls > 0 and bad == [], f"first {bad[:5]}"
        assert M.run_round_trip(b) == []


def test_device_equals_the_host_form_byte_for_byte(gpu, data):
    dev, host = M.DeviceBackend(data), M.HostBackend(data)
    for case in (M.Case("mixed", M.N_MAX, 7), M.Case("injected", None, 13)):
        g, h = dev.parse(case), host.parse(case)
        assert g[0] == h[0] and all(np.array_equal(a, b) for a, b in zip(g[1:], h[1:])), case.label


def test_a_decreasing_offset_pair_is_a_length_error(gpu, data):
    """len is the unsigned difference: nothing of that name is read, the next name is unharmed."""
    off = np.array([64, 0, 64], dtype=np.uint64)
    n, dig, status, valid = M.DeviceBackend(data).parse_text(b"a" * 64, off, 2)
    assert status[:2].tolist() == [M.KRK_DHEX_LEN | 0x3FFFFFFF, 0] and int(valid[0]) == 2
    assert not dig[:32].any() and (dig[32:64] == 0xAA).all()


def test_a_name_across_the_4_gib_line(gpu, data):
    """Eight names in a device allocation of 2^32 + 4,096 bytes with off[0] = 2^32 - 209: the
    fourth straddles byte 2^32 of the text.  Only the tail of the allocation is written; the
    results equal the host form's on the same names, and the transcription."""
    names = [data.listings["aligned"][k] for k in range(8)]
    names[1] = names[1][:63]                     # odd length: the later names start at odd offsets
    names[5] = names[5][:20] + b"G" + names[5][21:]
    base = (1 << 32) - 209
    lens = np.array([len(x) for x in names], dtype=np.uint64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64) + np.uint64(base)
    assert off[3] < 1 << 32 < off[4] and int(off[4] - off[3]) == 64
    text = np.frombuffer(b"".join(names), dtype=np.uint8)
    buf = D.DeviceBuffer((1 << 32) + 4096)
    buf.from_host(text, offset=base)
    obuf = D.DeviceBuffer(off.nbytes)
    obuf.from_host(off)
    dig, status, valid = D.PinnedArray((8 * 32 + 8,), np.uint8), D.PinnedArray((10,), np.uint32), D.PinnedArray((2,), np.uint64)
    dig.a[:], status.a[:], valid.a[:] = 0xFF, 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
    check(lib.krk_digest_parse_hex_dev(buf.ptr, obuf.ptr, 8, dig.ptr, status.ptr, valid.ptr, None))
    check(lib.krk_stream_sync(None))
    want = [M.ref_parse(x) for x in names]
    assert status.a[:8].tolist() == [s for s, _ in want] and (status.a[8:] == 0xFFFFFFFF).all()
    assert bytes(dig.a[:256]) == b"".join(d for _, d in want) and (dig.a[256:] == 0xFF).all()
    assert int(valid.a[0]) == sum(1 << i for i, (s, _) in enumerate(want) if s == 0) == 0b11011101
    assert int(valid.a[1]) == 0xFFFFFFFFFFFFFFFF
    # the host form on the same names, at offsets from 0
    hd = np.zeros(256, dtype=np.uint8)
    hs = np.zeros(8, dtype=np.uint32)
    h_off = off - np.uint64(base)
    check(lib.krk_digest_parse_hex(text.ctypes.data, h_off.ctypes.data_as(M.u64p), 8, hd.ctypes.data,
                                   hs.ctypes.data_as(C.POINTER(C.c_uint32)), None))
    assert np.array_equal(hd, dig.a[:256]) and np.array_equal(hs, status.a[:8])


def test_pageable_and_misaligned_pointers_are_refused_before_any_launch(gpu, data):
    n = 65
    text, off = data.pack("mixed", n, 0)
    tbuf, obuf = D.DeviceBuffer(len(text) + 8), D.DeviceBuffer(off.nbytes + 8)
    tbuf.from_host(np.frombuffer(text, dtype=np.uint8))
    obuf.from_host(off)
    dig, status, valid, hex_ = (D.DeviceBuffer(32 * n), D.DeviceBuffer(4 * n + 8), D.DeviceBuffer(16 + 8),
                                D.DeviceBuffer(64 * n))
    canary = {b: np.full(b.nbytes, 0xFF, dtype=np.uint8) for b in (dig, status, valid, hex_)}
    for b, c in canary.items():
        b.from_host(c)
    pageable = np.full(64 * n, 0xFF, dtype=np.uint8)
    pg = pageable.ctypes.data
    E = _capi.KRK_EINVAL

    def parse(t, o, d, s, v):
        return lib.krk_digest_parse_hex_dev(t, o, n, d, s, v, None)

    with D.KernelTimer():
        assert parse(pg, obuf.ptr, dig.ptr, status.ptr, valid.ptr) == E
        assert b"digest_parse_hex_dev" in lib.krk_last_error()
        assert parse(tbuf.ptr, off.ctypes.data, dig.ptr, status.ptr, valid.ptr) == E
        assert parse(tbuf.ptr, obuf.ptr, pg, status.ptr, valid.ptr) == E
        assert parse(tbuf.ptr, obuf.ptr, dig.ptr, pg, valid.ptr) == E
        assert parse(tbuf.ptr, obuf.ptr, dig.ptr, status.ptr, pg) == E
        assert parse(tbuf.ptr, obuf.ptr + 4, dig.ptr, status.ptr, valid.ptr) == E
        assert parse(tbuf.ptr, obuf.ptr, dig.ptr, status.ptr + 2, valid.ptr) == E
        assert parse(tbuf.ptr, obuf.ptr, dig.ptr, status.ptr, valid.ptr + 4) == E
        assert parse(None, obuf.ptr, dig.ptr, status.ptr, valid.ptr) == E
        assert parse(tbuf.ptr, None, dig.ptr, status.ptr, valid.ptr) == E
        assert parse(tbuf.ptr, obuf.ptr, None, status.ptr, valid.ptr) == E
        assert lib.krk_digest_format_hex_dev(pg, n, hex_.ptr, None) == E
        assert b"digest_format_hex_dev" in lib.krk_last_error()
        assert lib.krk_digest_format_hex_dev(dig.ptr, n, pg, None) == E
        assert lib.krk_digest_format_hex_dev(None, n, hex_.ptr, None) == E
        assert lib.krk_digest_format_hex_dev(dig.ptr, n, None, None) == E
        D.synchronize()
        assert D.KernelTimer.stats("digest_parse_hex")[0] == 0 and D.KernelTimer.stats("digest_format_hex")[0] == 0
        for b, c in canary.items():
            assert np.array_equal(b.to_host(np.uint8), c)
        assert (pageable == 0xFF).all()
        # the accepted neighbours: one timed launch each, its work units the names
        assert parse(tbuf.ptr, obuf.ptr, dig.ptr, status.ptr, valid.ptr) == _capi.KRK_OK
        assert lib.krk_digest_format_hex_dev(dig.ptr, n, hex_.ptr, None) == _capi.KRK_OK
        D.synchronize()
        assert [u for _, u, _, _ in D.KernelTimer.timeline("digest_parse_hex")] == [n]
        assert [u for _, u, _, _ in D.KernelTimer.timeline("digest_format_hex")] == [n]
    wd, ws, wv = data.reference("mixed", n)
    assert np.array_equal(dig.to_host(np.uint8), wd) and np.array_equal(status.to_host(np.uint32, n), ws)
    assert np.array_equal(valid.to_host(np.uint64, 2), wv)
    # n == 0: nothing to do, nothing touched
    assert lib.krk_digest_parse_hex_dev(None, None, 0, None, None, None, None) == _capi.KRK_OK
    assert lib.krk_digest_format_hex_dev(None, 0, None, None) == _capi.KRK_OK
