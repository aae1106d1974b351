"""GPU: krk_conn_round_dev and krk_conn_preempt_dev around their kernels -- the refusals with no
launch, no output and no state touched; the staging of the torrents and lists; two rounds queued
back to back on one stream, the second over the first's state; the device.py wrappers with outputs
in device and in page-locked memory; and connstate.ConnRound / PreemptionSweep with placement "gpu"
against placement "host" (the cases and the comparison live in tests/conn_matrix.py)."""
import numpy as np
import pytest

from kraken_amd import _capi, connstate as CS, device as D
from kraken_amd._capi import check, lib
from kraken_amd.piecerequest import MockClock
from tests import conn_matrix as M
from tests import test_connstate as TC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device(gpu):
    return M.DeviceBackend()


def buffers(device, c):
    state = [device.upload(a) for a in (c.bits, c.expiry, c.capacity)]
    neigh = device.upload(c.neighbors)
    outs = [device.upload(M.prefilled(k)) for k in c.out_sizes()]
    return state, neigh, outs


def read(c, state, outs):
    return (state[0].to_host(np.uint64, c.bits.size), state[1].to_host(np.int64, c.expiry.size),
            state[2].to_host(np.uint32, c.capacity.size), *(o.to_host(np.uint32, k) for o, k in zip(outs, c.out_sizes())))


def untouched(c, got):
    return all(np.array_equal(g, w) for g, w in zip(got[:3], (c.bits, c.expiry, c.capacity))) and \
        all((g == M.CANARY32).all() for g in got[3:])


def test_refusals_come_before_any_launch(device):
    c = M.refusal_case()
    state, neigh, outs = buffers(device, c)
    pageable = [c.bits.copy(), c.expiry.copy(), c.capacity.copy(), c.neighbors.copy()] + [M.prefilled(k) for k in c.out_sizes()]
    slots = [M.A_BITS, M.A_EXPIRY, M.A_CAPACITY, M.A_NEIGH] + [M.A_OUT + k for k in range(5)]
    ptrs = [b.ptr for b in state] + [neigh.ptr] + [o.ptr for o in outs]

    def call(change=None, **kw):
        a, dials = M.round_args(c, *(b.ptr for b in state), neigh.ptr, [o.ptr for o in outs])
        if change:
            change(a, dials)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.krk_conn_round_dev(*a, None)

    with D.KernelTimer():
        for label, change, rc in M.invalid_calls():  # every check runs on the host, before the launch
            assert call(change) == rc and b"conn_round_dev" in lib.krk_last_error(), label
        for slot, host in zip(slots, pageable):  # pageable memory where device memory belongs
            assert call(**{f"_{slot}": host.ctypes.data}) == _capi.KRK_EINVAL, slot
        for slot, p in zip(slots, ptrs):  # misaligned by half an element
            assert call(**{f"_{slot}": p + (4 if slot in (M.A_BITS, M.A_EXPIRY, M.A_NEIGH) else 2)}) == _capi.KRK_EINVAL, slot
            assert b"aligned" in lib.krk_last_error()
        D.synchronize()
        assert D.KernelTimer.stats("conn_round")[0] == 0
        assert untouched(c, read(c, state, outs))
        assert np.array_equal(pageable[0], c.bits) and all((p == M.CANARY32).all() for p in pageable[4:])
        # the accepted neighbour: one timed call, its work units the torrents
        assert call() == _capi.KRK_OK
        D.synchronize()
        assert D.KernelTimer.stats("conn_round")[0] == 1
        assert [u for _, u, _, _ in D.KernelTimer.timeline("conn_round")] == [len(c.torrents)]
    assert M.compare(c, read(c, state, outs)) == []


def test_sweep_refusals_come_before_any_launch(device):
    c = M.sweeps()[1]
    want = c.want()
    bits, times = device.upload(c.bits), [device.upload(a) for a in c.times]
    close, n_close = device.upload(np.full_like(want[0], M.CANARY64)), device.upload(np.full_like(want[1], M.CANARY32))
    ok = [bits.ptr, *(t.ptr for t in times), close.ptr, n_close.ptr]
    pageable = [c.bits, *c.times, want[0].copy(), want[1].copy()]

    def call(p=ok, now=c.now, tti=c.tti, ttl=c.ttl):
        return lib.krk_conn_preempt_dev(c.structs, len(c.torrents), *p[:4], now, tti, ttl, *p[4:], None)

    with D.KernelTimer():
        assert call(now=-1) == call(tti=-1) == call(ttl=-1) == _capi.KRK_EINVAL
        for k in range(6):
            assert call(ok[:k] + [None] + ok[k + 1:]) == _capi.KRK_EINVAL, k
            assert call(ok[:k] + [pageable[k].ctypes.data] + ok[k + 1:]) == _capi.KRK_EINVAL, k
            assert call(ok[:k] + [ok[k] + 2] + ok[k + 1:]) == _capi.KRK_EINVAL and b"aligned" in lib.krk_last_error(), k
        D.synchronize()
        assert D.KernelTimer.stats("conn_preempt")[0] == 0
        assert (close.to_host(np.uint64, want[0].size) == M.CANARY64).all()
        assert (n_close.to_host(np.uint32, want[1].size) == M.CANARY32).all()
        assert call() == _capi.KRK_OK
        D.synchronize()
        assert D.KernelTimer.stats("conn_preempt")[0] == 1
    assert M.compare(c, (close.to_host(np.uint64, want[0].size), n_close.to_host(np.uint32, want[1].size)),
                     names=("close", "n_close")) == []


def test_the_host_arrays_may_be_overwritten_when_the_call_returns(device):
    c = M.case("matrix P=65")
    state, neigh, outs = buffers(device, c)
    a, dials = M.round_args(c, *(b.ptr for b in state), neigh.ptr, [o.ptr for o in outs])
    check(lib.krk_conn_round_dev(*a, None))
    for t in a[M.A_TORRENTS]:  # the call has staged its copies
        t.n_peers, t.self_peer, t.flags, t.bits_off, t.peer_off = 1, 0, 1, 0, 0
    for l in a[M.A_LISTS]:
        l.trans_off = l.n_trans = l.in_off = l.n_in = l.dial_off = l.n_dial = 0
    for e in a[M.A_TRANS]:
        e.peer, e.kind = 0, 3
    for e in a[M.A_IN]:
        e.peer, e.neigh_off = 0, 0
    dials[:] = 0
    check(lib.krk_stream_sync(None))
    assert M.compare(c, read(c, state, outs)) == []


def two_rounds():
    """Two rounds over one torrent of 130 peers: the second frees and establishes what the first
    admitted, and dials into the capacity that frees."""
    tor = [(130, 129, 0)]
    row = np.zeros(3, dtype=np.uint64)
    row[0] = 0b1110
    first = D.ConnBatch(tor, [([], [(1, None), (2, row), (3, row), (4, row)], list(range(60, 130)))])
    second = D.ConnBatch(tor, [([(1, D.CN_ESTABLISHED), (2, D.CN_FAILED_IN), (60, D.CN_FAILED_OUT), (61, D.CN_ESTABLISHED)],
                               [(5, row)], [60, 62, 10, 11, 12, 13])])
    return first, second


def test_two_rounds_back_to_back_on_one_stream(device):
    """Both rounds queued before either has run, over ONE state: the second round sees the first's."""
    first, second = two_rounds()
    host = [np.zeros(first.total_words, np.uint64), np.zeros(130, np.int64), np.array([8], np.uint32)]
    want = [D.conn_round(b, *host, 500, 30, 2) for b in (first, second)]
    dev = [device.upload(a) for a in (np.zeros(first.total_words, np.uint64), np.zeros(130, np.int64), np.array([8], np.uint32))]
    neigh = [device.upload(b.neighbors) for b in (first, second)]
    outs = [D.ConnOutputs(first), D.ConnOutputs(second, pinned=True)]
    for b, n, o in zip((first, second), neigh, outs):
        o.fill(0xA5)
        assert D.conn_round_dev(b, *dev, n, 500, 30, 2, out=o) is o
    check(lib.krk_stream_sync(None))
    for o, w in zip(outs, want):
        assert all(np.array_equal(g, h) for g, h in zip(o.to_host(), w))
    for d, h in zip(dev, host):
        assert np.array_equal(d.to_host(h.dtype, h.size), h)
    # the first round: 1, 2, 3 admitted, 4 has three mutual conns; five dials take the rest
    assert want[0][1].tolist() == [D.CN_OK, D.CN_OK, D.CN_OK, D.CN_TOO_MANY_MUTUAL]
    assert want[0][3].tolist() == [[3, 5]] and want[1][4].tolist() == [2]
    assert want[1][2].tolist() == [D.CN_BLACKLISTED, D.CN_ALREADY_PENDING, D.CN_OK, D.CN_AT_CAPACITY, D.CN_AT_CAPACITY,
                                   D.CN_AT_CAPACITY]


def test_wrappers_without_an_output_holder(device):
    first, _ = two_rounds()
    host = [np.zeros(first.total_words, np.uint64), np.zeros(130, np.int64), np.array([8], np.uint32)]
    dev = [device.upload(a) for a in host]
    want = D.conn_round(first, *host, 500, 30, 2)
    got = D.conn_round_dev(first, *dev, None, 500, 30, 2)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    for d, h in zip(dev, host):
        assert np.array_equal(d.to_host(h.dtype, h.size), h)
    # the state in page-locked memory
    pinned = [D.PinnedArray(a.shape, a.dtype) for a in host]
    pinned[0].a[:], pinned[1].a[:], pinned[2].a[:] = 0, 0, 8
    got = D.conn_round_dev(first, *pinned, None, 500, 30, 2)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert all(np.array_equal(p.a, h) for p, h in zip(pinned, host))


@pytest.mark.parametrize("disable", [False, True])
def test_conn_round_gpu_equals_host(device, disable):
    got = {}
    for placement in ("host", "gpu"):
        s, conns = TC.seeded(MockClock(1000), MaxMutualConnections=3, DisableBlacklist=disable)
        r = TC.feed(CS.ConnRound(s, placement), TC.events(conns))
        got[placement] = ({h: {k: [x.PeerID() if isinstance(x, CS.Conn) else
                                   (x[0].PeerID(), x[1]) if isinstance(x, tuple) and isinstance(x[0], CS.Conn) else x
                                   for x in v] if isinstance(v, list) else v for k, v in t.__dict__.items()}
                           for h, t in r.items()}, TC.snapshot(s))
    assert got["gpu"] == got["host"]
    assert got["host"][0]["h0"]["dial"] and got["host"][0]["h1"]["capacity"] == 0


def test_drive_and_sweep_gpu_equal_host(device):
    a, _, dial_a = TC.drive("host")
    b, _, dial_b = TC.drive("gpu")
    assert dial_a == dial_b and TC.snapshot(a) == TC.snapshot(b)
    a.clock.Add(200)
    b.clock.Add(200)
    received = lambda h, p: 190 if p.endswith("3") else 0  # noqa: E731
    ha = CS.PreemptionSweep(a, 100, 215, received, None, "host")
    hb = CS.PreemptionSweep(b, 100, 215, received, None, "gpu")
    assert [(c.InfoHash(), c.PeerID()) for c in ha] == [(c.InfoHash(), c.PeerID()) for c in hb]
    assert 0 < len(ha) < a.NumActiveConns()
