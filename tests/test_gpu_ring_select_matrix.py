"""GPU parity: the ring-select kernels (ring_select.hip) at their lane, wave, workgroup and
scan-tile edges through krk_ring_select_dev -- bits, count and the ascending index list against
the numpy transcription of the contract and, bit for bit, against the host form krk_ring_select
(the cases and the comparison live in tests/ring_select_matrix.py; tests/test_ring_select_matrix_cpu.py
proves them on the host form); OwnsBatch and ShardMaskMoved against the oracle's Locations on a
sample; the pointer refusals; and the asynchronous contract of the mask."""
import ctypes as C

import numpy as np
import pytest

from kraken_amd import _capi, device as D, hashring
from kraken_amd._capi import lib
from tests import ring_select_matrix as M

pytestmark = pytest.mark.gpu

CANARY = M.CANARY


@pytest.fixture(scope="module")
def data():
    return M.Data()


@pytest.fixture(scope="module")
def device(gpu, data):
    return M.DeviceBackend(data)


def test_small_shapes_every_cap_in_device_memory(device):
    calls, bad = M.run_cases(device, M.cases(M.SMALL))
    assert calls > 0 and bad == [], f"{len(bad)} mismatches of {calls} calls, first {bad[:5]}"


def test_small_shapes_every_cap_in_page_locked_memory(device):
    calls, bad = M.run_cases(device, M.cases(M.SMALL), pinned=True)
    assert calls > 0 and bad == [], f"{len(bad)} mismatches of {calls} calls, first {bad[:5]}"


@pytest.mark.parametrize("n", M.LARGE)
def test_scan_tile_shapes(device, n):
    """T W - 1, T W + 1 and two full scan tiles plus a ragged tail: the edges mask at every cap
    (its index list is exactly the EDGES below n), the other masks with the whole list."""
    calls, bad = M.run_cases(device, [c for c in M.cases([n]) if c.mask == "edges"])
    calls2, bad2 = M.run_cases(device, [c for c in M.cases([n]) if c.mask != "edges"], all_caps=False)
    assert calls and calls2 and bad + bad2 == [], f"first {(bad + bad2)[:5]}"


def test_scan_tile_tail_into_page_locked_memory(device):
    calls, bad = M.run_cases(device, [c for c in M.cases([M.N_TAIL]) if c.mask in ("edges", "ones")], all_caps=False,
                             pinned=True)
    assert calls > 0 and bad == [], f"first {bad[:5]}"


def test_device_equals_the_host_form_bit_for_bit(device, data):
    host = M.HostBackend(data)
    for case in M.cases((65, M.W + 1, M.T * M.W + 1)):
        want = data.reference(case)
        cap = int(want[1].size) + 1
        g, h = device.run(case, cap), host.run(case, cap)
        assert g[1] == h[1] and np.array_equal(g[0], h[0]) and np.array_equal(g[2], h[2]), case.label


def test_digests_at_an_odd_address(gpu, data):
    shifted = M.DeviceBackend(data, shift=1)
    calls, bad = M.run_cases(shifted, M.cases((65, M.W + 1)), all_caps=False)
    calls2, bad2 = M.run_cases(shifted, [M.Case(M.N_TAIL, "random", False, True)], all_caps=False)
    assert calls and calls2 and bad + bad2 == [], f"first {(bad + bad2)[:5]}"


def test_pageable_and_misaligned_outputs_are_refused_before_any_launch(device, data):
    n = M.W + 1
    mask = data.masks["random"]
    mp = mask.ctypes.data_as(M.u64p)
    bits = D.DeviceBuffer(8 * M.words(n))
    idx = D.DeviceBuffer(8 * n)
    count = D.DeviceBuffer(8)
    canary = {b: np.full(b.nbytes // 8, CANARY, dtype=np.uint64) for b in (bits, idx, count)}
    for b, c in canary.items():
        b.from_host(c)
    pageable = np.full(n, CANARY, dtype=np.uint64)
    pg = pageable.ctypes.data

    def call(digests, orb, b, i, cap, c):
        return lib.krk_ring_select_dev(digests, n, mp, 0, orb, b, i, cap, c, None)

    with D.KernelTimer():
        assert call(device.dev.ptr, None, pg, idx.ptr, n, count.ptr) == _capi.KRK_EINVAL
        assert b"ring_select_dev" in lib.krk_last_error()
        assert call(device.dev.ptr, None, bits.ptr, pg, n, count.ptr) == _capi.KRK_EINVAL
        assert call(device.dev.ptr, None, bits.ptr, idx.ptr, n, pg) == _capi.KRK_EINVAL
        assert call(device.dev.ptr, pg, bits.ptr, idx.ptr, n, count.ptr) == _capi.KRK_EINVAL
        assert call(data.digests.ctypes.data, None, bits.ptr, idx.ptr, n, count.ptr) == _capi.KRK_EINVAL
        assert call(device.dev.ptr, None, bits.ptr + 4, idx.ptr, n - 1, count.ptr) == _capi.KRK_EINVAL
        assert call(device.dev.ptr, None, bits.ptr, None, n, count.ptr) == _capi.KRK_EINVAL
        assert call(None, None, bits.ptr, idx.ptr, n, count.ptr) == _capi.KRK_EINVAL
        D.synchronize()
        assert D.KernelTimer.stats("ring_select")[0] == 0
        for b, c in canary.items():
            assert np.array_equal(b.to_host(np.uint64), c)
        assert (pageable == CANARY).all()
        # the accepted neighbour: one timed call, its work units the digests
        assert call(device.dev.ptr, None, bits.ptr, idx.ptr, n, count.ptr) == _capi.KRK_OK
        D.synchronize()
        assert D.KernelTimer.stats("ring_select")[0] == 1
        assert [u for _, u, _, _ in D.KernelTimer.timeline("ring_select")] == [n]
    want = data.reference(M.Case(n, "random", False, False))
    assert np.array_equal(bits.to_host(np.uint64), want[0]) and int(count.to_host(np.uint64)[0]) == want[1].size
    assert np.array_equal(idx.to_host(np.uint64)[:want[1].size], want[1])


def test_the_mask_may_be_overwritten_when_the_call_returns(device, data):
    """mask_host is staged before krk_ring_select_dev returns: overwritten right after, before the
    stream has run, the result is still the original mask's."""
    for pinned in (False, True):
        case = M.Case(M.N_TAIL, "random", False, False)
        want = data.reference(case)
        cap = int(want[1].size)
        got = device.run(case, cap, pinned=pinned, mask_after=CANARY)
        assert M.compare(case, cap, got, want) == []


def test_owns_and_moved_against_the_oracle_on_a_sample(gpu, orc):
    labels = [f"origin-{i:03d}.kraken.test:15002" for i in range(5)]
    healthy = np.array([1, 1, 0, 1, 1], dtype=np.uint8)
    rng = np.random.default_rng(5)
    d = rng.integers(0, 256, size=(1000, 32), dtype=np.uint8)

    def owners(names, h, max_replica, x):
        order = orc.hrw_ordered(bytes(x[:2]).hex(), names, [100] * len(names))
        return [names[j] for j in orc.ring_locations(order, h, max_replica)]

    ring = hashring.Ring(labels, [l for l, h in zip(labels, healthy) if h], 3)
    addr = labels[3]
    bits = ring.OwnsBatch(addr, d)
    got = np.unpackbits(bits.view(np.uint8), bitorder="little")[:1000].astype(bool)
    a = [owners(labels, healthy, 3, x) for x in d]
    assert got.tolist() == [addr in o for o in a] and 0 < got.sum() < 1000
    # the ring after origin-002 comes back and origin-004 leaves
    labels_b = labels[:4]
    other = hashring.Ring(labels_b, labels_b, 3)
    b = [owners(labels_b, np.ones(4, dtype=np.uint8), 3, x) for x in d]
    sel, idx = ring.Select(d, ring.ShardMaskMoved(other))
    want = [i for i in range(1000) if set(a[i]) != set(b[i])]
    assert idx.tolist() == want and 0 < len(want) < 1000
    assert np.flatnonzero(np.unpackbits(sel.view(np.uint8), bitorder="little")).tolist() == want


def test_empty_call_stores_the_count(device, data):
    count = D.PinnedArray((1,), np.uint64)
    count.a[:] = CANARY
    mp = data.masks["ones"].ctypes.data_as(M.u64p)
    assert lib.krk_ring_select_dev(None, 0, mp, 0, None, None, None, 0, count.ptr, None) == _capi.KRK_OK
    _capi.check(lib.krk_stream_sync(None))
    assert int(count.a[0]) == 0


def test_byte_offsets_past_4_gib(gpu):
    """2^27 digests and a ragged tail: record offsets (32 i) pass 2^32.  The digests are generated
    on the device; the call over all of them must agree, for the slices on both sides of the 4 GiB
    line, with the host form over those slices copied back, and its index list with its own bits."""
    n = (1 << 27) + 197
    off = (1 << 27) - 2048  # a multiple of 64: the tail slice straddles byte 2^32
    dev = D.DeviceBuffer(32 * n)
    _capi.check(lib.krk_synth_fill_dev(dev.ptr, 7, 0, 32 * n, 0, None))
    rng = np.random.default_rng(M.SEED + 1)
    mask = np.uint64(1) << rng.integers(0, 64, size=1024).astype(np.uint64)  # 1/64 of the shards
    nw = M.words(n)
    cap = n // 32
    bits, idx, count = D.DeviceBuffer(8 * nw), D.DeviceBuffer(8 * cap), D.PinnedArray((1,), np.uint64)
    _capi.check(lib.krk_ring_select_dev(dev.ptr, n, mask.ctypes.data_as(M.u64p), 0, None, bits.ptr, idx.ptr, cap,
                                        count.ptr, None))
    _capi.check(lib.krk_stream_sync(None))
    c = int(count.a[0])
    got_bits = bits.to_host(np.uint64, nw)
    got_idx = idx.to_host(np.uint64, c)
    assert n // 128 < c < cap  # about n / 64
    # the index list is the set bits, ascending
    assert np.array_equal(np.flatnonzero(np.unpackbits(got_bits.view(np.uint8), bitorder="little")), got_idx.astype(np.int64))
    for lo, m in ((0, 4096), (off, n - off)):
        d = dev.to_host(np.uint8, 32 * m, offset=32 * lo)
        hb, hi = hashring.select_host(d, mask)
        assert np.array_equal(got_bits[lo // 64:lo // 64 + M.words(m)], hb), lo
        assert np.array_equal(got_idx[(got_idx >= lo) & (got_idx < lo + m)], hi + np.uint64(lo)) and hi.size > 8, lo
