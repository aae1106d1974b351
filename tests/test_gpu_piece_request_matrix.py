"""GPU parity: the piece request kernels (piece_request.hip) at their word, wave, thread-stride
and launch edges through krk_piece_request_round_dev -- counts, picks and n_picked against
tests/piece_request_ref.py's restatement and, bit for bit, against the host form
krk_piece_request_round (the cases and the comparison live in tests/piece_request_matrix.py;
tests/test_piece_request_matrix_cpu.py proves them on the host form); outputs in device memory and
in page-locked host memory; the pointer refusals; the staging of the torrent array; and two calls
back to back on one stream."""
import numpy as np
import pytest

from kraken_amd import _capi, device as D
from kraken_amd._capi import check, lib
from tests import piece_request_matrix as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device(gpu):
    return M.DeviceBackend()


def small(b):
    return b.torrents[0].n <= 2 * M.G + 1


def test_small_shapes_in_device_memory(device):
    calls, bad = M.run_cases(device, [b for b in M.cases() if small(b)])
    assert calls > 0 and bad == [], f"{len(bad)} mismatches of {calls} calls, first {bad[:5]}"


def test_small_shapes_in_page_locked_memory(device):
    calls, bad = M.run_cases(device, [b for b in M.cases() if small(b) and b.torrents[0].n_peers <= 10], pinned=True)
    assert calls > 0 and bad == [], f"{len(bad)} mismatches of {calls} calls, first {bad[:5]}"


def test_c4_shapes(device):
    """81,920 pieces: 320 passes a scan, every kind, both policies."""
    big = [b for b in M.cases() if not small(b)]
    calls, bad = M.run_cases(device, big)
    calls2, bad2 = M.run_cases(device, big[:4], pinned=True)
    assert calls and calls2 and bad + bad2 == [], f"first {(bad + bad2)[:5]}"


@pytest.mark.parametrize("k", [0, 1, 3, 70])
def test_batches(device, k):
    """0, 1, 3 and 70 torrents that mix the N of the matrix, a zero-piece and a zero-peer torrent in
    the middle, no array starting at 0; 70 torrents have more count units than the count launch has
    workgroups, so those stride."""
    for limit in (3, M.LMAX) if k == 3 else (3,):
        b = M.batch(k, limit)
        for pinned in (False, True):
            calls, bad = M.run_cases(device, [b], pinned=pinned)
            assert calls == 2 and bad == [], bad[:5]


def test_device_equals_the_host_form_bit_for_bit(device):
    host = M.HostBackend()
    picked = [b for b in M.cases() if b.torrents[0].n in (65, M.S + 1, M.G + 1, M.N_C4)][::3] + [M.batch(3), M.batch(70)]
    for b in picked:
        for counts in (True, False):
            g, h = device.run(b, counts=counts), host.run(b, counts=counts)
            assert all(np.array_equal(x, y) for x, y in zip(g, h)), b.label


def test_two_calls_back_to_back_on_one_stream(device):
    """Both calls queued before either has run: each has its own staged torrents and its own
    scratch, and the second's outputs are not the first's."""
    a, b = M.batch(70), M.batch(3, M.LMAX)
    oa, ob = device.outputs(a, False), device.outputs(b, True)
    device.upload(a), device.upload(b)
    device.launch(a, oa)
    device.launch(b, ob)
    check(lib.krk_stream_sync(None))
    assert M.compare(a, device.read(a, oa, False)) == [] and M.compare(b, device.read(b, ob, True)) == []


def test_the_torrent_array_may_be_overwritten_when_the_call_returns(device):
    b = M.batch(70)
    outs = device.outputs(b, False)
    bits, quota = device.upload(b)
    structs = (_capi.krk_request_torrent * len(b.torrents))(*b.structs)
    check(lib.krk_piece_request_round_dev(structs, len(b.torrents), bits.ptr, quota.ptr, b.limit, outs[0].ptr,
                                          outs[1].ptr, outs[2].ptr, None))
    for s in structs:  # the call has staged its copy
        s.n_pieces, s.n_peers, s.bits_off = 1, 1, 0
    check(lib.krk_stream_sync(None))
    assert M.compare(b, device.read(b, outs, False)) == []


def test_pageable_and_misaligned_pointers_are_refused_before_any_launch(device):
    b = M.single("random", M.S + 1, 2, M.RAREST, 3, quota=[3, 3])
    bits, quota = device.upload(b)
    outs = device.outputs(b, False)
    pageable = [M.prefilled(k) for k in b.sizes()]
    host_bits, host_quota = b.bits.copy(), b.quota.copy()
    good = [b.structs, 1, bits.ptr, quota.ptr, b.limit, outs[0].ptr, outs[1].ptr, outs[2].ptr, None]

    def call(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.krk_piece_request_round_dev(*a)

    E = _capi.KRK_EINVAL
    with D.KernelTimer():
        assert call(_2=host_bits.ctypes.data) == E and b"piece_request_round_dev" in lib.krk_last_error()
        assert call(_3=host_quota.ctypes.data) == E
        for k in range(3):
            assert call(**{f"_{5 + k}": pageable[k].ctypes.data}) == E
        assert call(_2=bits.ptr + 4) == E and b"aligned" in lib.krk_last_error()
        assert call(_3=quota.ptr + 2) == E
        for k in range(3):
            assert call(**{f"_{5 + k}": outs[k].ptr + 2}) == E
        assert call(_4=0) == E and call(_4=M.LMAX + 1) == E
        assert call(_6=None) == E and call(_7=None) == E and call(_2=None) == E and call(_3=None) == E
        D.synchronize()
        assert D.KernelTimer.stats("piece_request")[0] == 0
        for o, k in zip(outs, b.sizes()):
            assert (o.to_host(np.uint32, k) == M.CANARY32).all()
        for p in pageable:
            assert (p == M.CANARY32).all()
        # the accepted neighbour: one timed call, its work units the torrents
        assert call() == _capi.KRK_OK
        D.synchronize()
        assert D.KernelTimer.stats("piece_request")[0] == 1
        assert [u for _, u, _, _ in D.KernelTimer.timeline("piece_request")] == [1]
    assert M.compare(b, device.read(b, outs, False)) == []


def test_wrappers_and_output_holder(device):
    """device.piece_request_round_dev over a RequestBatch with a RequestOutputs holder (device and
    pinned) and without one, against device.piece_request_round."""
    rng = np.random.default_rng(M.SEED)
    batch = D.RequestBatch([1000, 65, 0, 1], [5, 2, 1, 3], [D.PR_RAREST_FIRST, D.PR_SAMPLE, 0, D.PR_ALLOW_DUPLICATES],
                           [0, 77, 0, 0])
    bits = rng.integers(0, 1 << 64, size=batch.total_words, dtype=np.uint64)
    quota = rng.integers(-1, 4, size=batch.total_peers).astype(np.int32)
    want = D.piece_request_round(batch, bits, quota, 3, counts=True)
    bits_dev, quota_dev = D.DeviceBuffer(bits.nbytes), D.DeviceBuffer(quota.nbytes)
    bits_dev.from_host(bits)
    quota_dev.from_host(quota)
    for pinned in (False, True):
        out = D.RequestOutputs(batch, 3, counts=True, pinned=pinned)
        out.fill(0xA5)
        assert D.piece_request_round_dev(batch, bits_dev, quota_dev, 3, out=out) is out
        check(lib.krk_stream_sync(None))
        assert all(np.array_equal(g, w) for g, w in zip(out.to_host(), want))
    c, pk, npk = D.piece_request_round_dev(batch, bits_dev, quota_dev, 3)
    assert c is None and np.array_equal(pk, want[1]) and np.array_equal(npk, want[2])
