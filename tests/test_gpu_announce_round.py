"""GPU: krk_announce_round_dev around its kernels -- the refusals with no launch, no output and no
bit touched; the staging of the torrent and announce arrays; two rounds queued back to back on one
stream, the second over the rows the first updated; the device.py wrappers with outputs in device
and in page-locked memory; and peerstore.AnnounceRound(placement="gpu") against placement="host"
(the cases and the comparison live in tests/announce_matrix.py)."""
import numpy as np
import pytest

from kraken_amd import _capi, device as D, peerstore as PS
from kraken_amd._capi import check, lib
from kraken_amd.piecerequest import MockClock
from tests import announce_matrix as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device(gpu):
    return M.DeviceBackend()


def buffers(c):
    bits = D.DeviceBuffer(c.bits.nbytes)
    bits.from_host(c.bits)
    outs = [D.DeviceBuffer(4 * k) for k in c.sizes()]
    for o, k in zip(outs, c.sizes()):
        o.from_host(M.prefilled(k))
    return bits, outs


def read(c, bits, outs):
    return (bits.to_host(np.uint64, c.bits.size), *(o.to_host(np.uint32, k) for o, k in zip(outs, c.sizes())))


def test_refusals_come_before_any_launch(device):
    c = M.refusal_case()
    bits, outs = buffers(c)
    pageable = [M.prefilled(k) for k in c.sizes()]
    host_bits = c.bits.copy()

    def call(change=None, **kw):
        a = M.call_args(c, bits.ptr, [o.ptr for o in outs])
        if change:
            change(a)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.krk_announce_round_dev(*a, None)

    E = _capi.KRK_EINVAL
    with D.KernelTimer():
        for label, change in M.invalid_calls():  # every check runs on the host, before the launch
            assert call(change) == E and b"announce_round_dev" in lib.krk_last_error(), label
        assert call(_2=host_bits.ctypes.data) == E
        for k in range(3):
            assert call(**{f"_{7 + k}": pageable[k].ctypes.data}) == E
        assert call(_2=bits.ptr + 4) == E and b"aligned" in lib.krk_last_error()
        for k in range(3):
            assert call(**{f"_{7 + k}": outs[k].ptr + 2}) == E
        D.synchronize()
        assert D.KernelTimer.stats("announce_round")[0] == 0
        got = read(c, bits, outs)
        assert np.array_equal(got[0], c.bits) and all((g == M.CANARY32).all() for g in got[1:])
        assert np.array_equal(host_bits, c.bits) and all((p == M.CANARY32).all() for p in pageable)
        # the accepted neighbour: one timed call, its work units the announces
        assert call() == _capi.KRK_OK
        D.synchronize()
        assert D.KernelTimer.stats("announce_round")[0] == 1
        assert [u for _, u, _, _ in D.KernelTimer.timeline("announce_round")] == [len(c.announces)]
    assert M.compare(c, read(c, bits, outs)) == []


def test_the_host_arrays_may_be_overwritten_when_the_call_returns(device):
    c = M.case("A=257 over three torrents")
    bits, outs = buffers(c)
    a = M.call_args(c, bits.ptr, [o.ptr for o in outs])
    check(lib.krk_announce_round_dev(*a, None))
    for t in a[0]:  # the call has staged its copies
        t.n_peers, t.n_windows, t.cur_row, t.n_origins, t.bits_off = 1, 1, 0, 0, 0
    for e in a[3]:
        e.torrent, e.peer, e.flags, e.source, e.seed = 0, 0, 1, 0, 0
    check(lib.krk_stream_sync(None))
    assert M.compare(c, read(c, bits, outs)) == []


def test_two_rounds_back_to_back_on_one_stream(device):
    """Both rounds queued before either has run, over ONE bits array: the second round's handouts see
    the first round's announcers."""
    first = D.AnnounceBatch([(130, 3, 2, 3)], [(0, k, k % 2, D.AN_NONE, 100 + k) for k in range(0, 130, 7)])
    second = D.AnnounceBatch([(130, 3, 2, 3)], [(0, 129, 0, 129, 7), (0, 64, 0, D.AN_NONE, 8)])
    host_bits = np.zeros(first.total_words, dtype=np.uint64)
    want = [D.announce_round(b, host_bits, 50, D.AN_COMPLETENESS) for b in (first, second)]
    bits = D.DeviceBuffer(host_bits.nbytes)
    bits.zero()
    outs = [D.AnnounceOutputs(first, 50), D.AnnounceOutputs(second, 50, pinned=True)]
    for b, o in zip((first, second), outs):
        o.fill(0xA5)
        assert D.announce_round_dev(b, bits, 50, D.AN_COMPLETENESS, out=o) is o
    check(lib.krk_stream_sync(None))
    for o, w in zip(outs, want):
        assert all(np.array_equal(g, h) for g, h in zip(o.to_host(), w))
    assert np.array_equal(bits.to_host(np.uint64, host_bits.size), host_bits)
    assert int(want[1][1][0]) == len(range(0, 130, 7)) + 1 + 3  # the first round's 19, peer 64 and the origins


def test_wrappers_without_an_output_holder(device):
    c = M.case("a window all of whose members are already selected")
    b = D.AnnounceBatch([t[:4] for t in c.torrents], c.announces)
    host_bits = c.bits[M.BASE:M.BASE + b.total_words].copy()
    want = D.announce_round(b, host_bits, c.limit, c.policy)
    bits = D.DeviceBuffer(8 * b.total_words)
    bits.from_host(c.bits[M.BASE:M.BASE + b.total_words])
    got = D.announce_round_dev(b, bits, c.limit, c.policy)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert np.array_equal(bits.to_host(np.uint64, b.total_words), host_bits)


def test_announce_round_gpu_equals_host_through_the_store(device):
    origins = {f"digest-{t}": [PS.PeerInfo(f"origin-{t}-{k}", "10.1.0.1", 15002 + k, Origin=True, Complete=True)
                               for k in range((0, 3, 8)[t])] for t in range(3)}

    def interval(k0, n):
        return [(f"digest-{k % 3}", f"hash-{k % 3}",
                 PS.PeerInfo(f"peer-{(k * 7) % 151:03d}", f"10.0.{k % 3}.{(k * 7) % 151}", 8000, Complete=k % 6 == 0))
                for k in range(k0, k0 + n)]

    got = {}
    for placement in ("host", "gpu"):
        clk = MockClock(0)
        s = PS.LocalStore(clk, 10, 5, seed=42)
        rounds = []
        for k in range(4):  # four announce intervals, a window apart: the handouts reach back across windows
            rounds.append(PS.AnnounceRound(s, origins, interval(100 * k, 257), 50, PS.CompletenessPolicy, placement))
            clk.Add(10)
        got[placement] = (rounds, {h: (T.rows.copy(), T.cur_row) for h, T in s.torrents.items()})
    for (hh, hl), (gh, gl) in zip(got["host"][0], got["gpu"][0]):
        assert gh == hh and np.array_equal(gl, hl)
    assert any(len(h) == 58 for h in got["host"][0][-1][0])  # a full handout: 50 peers and 8 origins
    for h, (rows, cur) in got["host"][1].items():
        assert cur == got["gpu"][1][h][1] and np.array_equal(rows, got["gpu"][1][h][0])
