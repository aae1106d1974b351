"""GPU parity: cleanup plans from a listing's text through krk_cleanup_plan_dev -- digest_hex.hip's
fused phase 1 (parse, shard lookup, expiry, the ballots of sel and valid) in front of
ring_select.hip's scan and scatter -- at the lane, wave, workgroup and scan-tile edges: bits,
valid, count and the ascending index list against the numpy transcription of the contract (the
cases and the comparison live in tests/cleanup_plan_matrix.py; tests/test_cleanup_plan_matrix_cpu.py
proves them on the host form), bit for bit against krk_cleanup_plan, and against the unfused
chain krk_digest_parse_hex_dev -> krk_expiry_bits -> krk_ring_select_dev; the pointer refusals;
and the asynchronous contract of the mask."""
import numpy as np
import pytest

from kraken_amd import _capi, device as D, hashring
from kraken_amd._capi import check, lib
from tests import cleanup_plan_matrix as M

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
    """T W - 1, T W + 1 and two full scan tiles plus a ragged tail: the edges mask without mtimes at
    every cap (its index list is exactly the EDGES below n), the other cases with the whole list."""
    every = [c for c in M.cases([n]) if c.mask == "edges" and c.times == "none"]
    calls, bad = M.run_cases(device, every)
    calls2, bad2 = M.run_cases(device, [c for c in M.cases([n]) if c not in every], all_caps=False)
    assert calls and calls2 and bad + bad2 == [], f"first {(bad + bad2)[:5]}"


def test_scan_tile_tail_into_page_locked_memory(device):
    calls, bad = M.run_cases(device, [c for c in M.cases([M.N_MAX]) if c.mask in ("edges", "ones")], all_caps=False,
                             pinned=True)
    assert calls > 0 and bad == [], f"first {bad[:5]}"


def test_text_at_an_odd_address(gpu, data):
    shifted = M.DeviceBackend(data, shift=1)
    calls, bad = M.run_cases(shifted, M.cases((65, M.W + 1)), all_caps=False)
    calls2, bad2 = M.run_cases(shifted, [M.Case(M.N_MAX, "random", True, "mtime")], all_caps=False)
    assert calls and calls2 and bad + bad2 == [], f"first {(bad + bad2)[:5]}"


def test_fused_call_equals_the_host_form_and_the_unfused_chain(device, data):
    """Three ways to the same plan, each against the transcription: the fused device call, the host
    form, and parse on the device -> expiry bits -> ring selection on the device over the valid-only
    sublisting, mapped back to listing positions."""
    host = M.HostBackend(data)

    def parse(n):
        d = D.PinnedArray((n, 32), np.uint8)
        v = D.PinnedArray((M.words(n),), np.uint64)
        check(lib.krk_digest_parse_hex_dev(device.text.ptr, device.off.ptr, n, d.ptr, None, v.ptr, None))
        check(lib.krk_stream_sync(None))
        return d.a.copy(), v.a.copy()

    def select(digests, mask, invert, or_bits):
        return hashring.select_dev(digests, mask, invert, or_bits)[1]

    for case in M.cases((65, M.W + 1, M.T * M.W + 1)):
        want = data.reference(case)
        cap = int(want[1].size) + M.SPARE
        g, h = device.run(case, cap), host.run(case, cap)
        assert M.compare(case, cap, g, want) == [] and M.compare(case, cap, h, want) == [], case.label
        assert g[1] == h[1] and all(np.array_equal(a, b) for a, b in zip((g[0], g[2], g[3]), (h[0], h[2], h[3]))), case.label
        idx, valid = M.chain(data, case, parse, select)
        assert np.array_equal(idx, want[1]), case.label
        assert np.array_equal(M.R._pack(valid)[:M.words(case.n)], want[2]), case.label


def test_pageable_and_misaligned_pointers_are_refused_before_any_launch(device, data):
    n = M.W + 1
    mp = data.masks["random"].ctypes.data_as(M.u64p)
    bits, valid, idx, count = D.DeviceBuffer(8 * M.words(n) + 8), D.DeviceBuffer(8 * M.words(n) + 8), D.DeviceBuffer(8 * n), D.DeviceBuffer(8)
    canary = {b: np.full(b.nbytes // 8, CANARY, dtype=np.uint64) for b in (bits, valid, idx, count)}
    for b, c in canary.items():
        b.from_host(c)
    pageable = np.full(n, CANARY, dtype=np.uint64)
    pg = pageable.ctypes.data
    text, off, mt = device.text.ptr, device.off.ptr, device.mt["mtime"].ptr
    E = _capi.KRK_EINVAL

    def call(t, o, m, b, v, i, cap, c):
        return lib.krk_cleanup_plan_dev(t, o, n, m, M.NOW, M.TTL, mp, 1, b, v, i, cap, c, None)

    with D.KernelTimer():
        assert call(data.text.ctypes.data, off, mt, bits.ptr, valid.ptr, idx.ptr, n, count.ptr) == E
        assert b"cleanup_plan_dev" in lib.krk_last_error()
        assert call(text, data.off.ctypes.data, mt, bits.ptr, valid.ptr, idx.ptr, n, count.ptr) == E
        assert call(text, off, data.mtime.ctypes.data, bits.ptr, valid.ptr, idx.ptr, n, count.ptr) == E
        assert call(text, off, mt, pg, valid.ptr, idx.ptr, n, count.ptr) == E
        assert call(text, off, mt, bits.ptr, pg, idx.ptr, n, count.ptr) == E
        assert call(text, off, mt, bits.ptr, valid.ptr, pg, n, count.ptr) == E
        assert call(text, off, mt, bits.ptr, valid.ptr, idx.ptr, n, pg) == E
        assert call(text, off + 4, mt, bits.ptr, valid.ptr, idx.ptr, n, count.ptr) == E
        assert call(text, off, mt + 4, bits.ptr, valid.ptr, idx.ptr, n, count.ptr) == E
        assert call(text, off, mt, bits.ptr + 4, valid.ptr, idx.ptr, n, count.ptr) == E
        assert call(text, off, mt, bits.ptr, valid.ptr + 4, idx.ptr, n, count.ptr) == E
        assert call(text, off, mt, bits.ptr, valid.ptr, None, n, count.ptr) == E
        assert call(None, off, mt, bits.ptr, valid.ptr, idx.ptr, n, count.ptr) == E
        assert call(text, None, mt, bits.ptr, valid.ptr, idx.ptr, n, count.ptr) == E
        assert call(text, off, mt, None, valid.ptr, idx.ptr, n, count.ptr) == E
        assert call(text, off, mt, bits.ptr, valid.ptr, idx.ptr, n, None) == E
        D.synchronize()
        assert D.KernelTimer.stats("cleanup_plan")[0] == 0
        for b, c in canary.items():
            assert np.array_equal(b.to_host(np.uint64), c)
        assert (pageable == CANARY).all()
        # the accepted neighbour: one timed call, its work units the names; no ring_select launch of its own
        assert call(text, off, mt, bits.ptr, valid.ptr, idx.ptr, n, count.ptr) == _capi.KRK_OK
        D.synchronize()
        assert D.KernelTimer.stats("cleanup_plan")[0] == 1 and D.KernelTimer.stats("ring_select")[0] == 0
        assert [u for _, u, _, _ in D.KernelTimer.timeline("cleanup_plan")] == [n]
    want = data.reference(M.Case(n, "random", True, "mtime"))
    nw = M.words(n)
    assert np.array_equal(bits.to_host(np.uint64, nw), want[0]) and np.array_equal(valid.to_host(np.uint64, nw), want[2])
    assert int(count.to_host(np.uint64)[0]) == want[1].size
    assert np.array_equal(idx.to_host(np.uint64)[:want[1].size], want[1])


def test_the_mask_may_be_overwritten_when_the_call_returns(device, data):
    """mask_host is staged before krk_cleanup_plan_dev returns: overwritten right after, before the
    stream has run, the result is still the original mask's."""
    for pinned in (False, True):
        case = M.Case(M.N_MAX, "random", True, "mtime")
        want = data.reference(case)
        cap = int(want[1].size)
        got = device.run(case, cap, pinned=pinned, mask_after=CANARY)
        assert M.compare(case, cap, got, want) == []


def test_empty_call_stores_the_count(gpu, data):
    count = D.PinnedArray((1,), np.uint64)
    count.a[:] = CANARY
    mp = data.masks["ones"].ctypes.data_as(M.u64p)
    assert lib.krk_cleanup_plan_dev(None, None, 0, None, M.NOW, M.TTL, mp, 0, None, None, None, 0, count.ptr,
                                    None) == _capi.KRK_OK
    check(lib.krk_stream_sync(None))
    assert int(count.a[0]) == 0
