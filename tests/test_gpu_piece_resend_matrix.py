"""GPU parity: the resend kernel (piece_resend.hip) at its pass, word and launch edges through
krk_piece_resend_round_dev -- target, quota_left and n_resent against tests/piece_resend_ref.py's
restatement and, bit for bit, against the host form krk_piece_resend_round (the cases and the
comparison live in tests/piece_resend_matrix.py; tests/test_piece_resend_matrix_cpu.py proves them
on the host form); outputs in device memory and in page-locked host memory; the refusals, the
host-side list checks among them, with no launch and no output touched; the staging of the
torrent, resend and failed arrays; and two calls back to back on one stream."""
import numpy as np
import pytest

from kraken_amd import _capi, device as D
from kraken_amd._capi import check, lib
from tests import piece_resend_matrix as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device(gpu):
    return M.DeviceBackend()


def test_matrix_in_device_memory(device):
    calls, bad = M.run_cases(device, M.cases())
    assert calls > 0 and bad == [], f"{len(bad)} mismatches of {calls} calls, first {bad[:5]}"


def test_matrix_in_page_locked_memory(device):
    calls, bad = M.run_cases(device, M.cases()[::3], pinned=True)
    assert calls > 0 and bad == [], f"{len(bad)} mismatches of {calls} calls, first {bad[:5]}"


def test_named_cases(device):
    for b, targets in M.named():
        for pinned in (False, True):
            tg, lf, nr = device.run(b, pinned=pinned)
            f0 = b.offs[0][2]
            assert tg[f0:f0 + len(targets)].tolist() == targets, b.label
            assert M.compare(b, (tg, lf, nr)) == []
        assert M.compare(b, device.run(b, left=False), left=False) == []


@pytest.mark.parametrize("k", [0, 1, 3, 70])
def test_batches(device, k):
    """0, 1, 3 and 70 torrents that mix the matrix's shapes, a torrent without failed entries and
    one without peers in the middle, no array starting at 0."""
    b = M.batch(k)
    for pinned in (False, True):
        calls, bad = M.run_cases(device, [b], pinned=pinned)
        assert calls == 2 and bad == [], bad[:5]


def test_device_equals_the_host_form_bit_for_bit(device):
    host = M.HostBackend()
    for b in M.cases()[::2] + [b for b, _ in M.named()] + [M.batch(3), M.batch(70)]:
        for left in (True, False):
            g, h = device.run(b, left=left), host.run(b, left=left)
            assert all(np.array_equal(x, y) for x, y in zip(g, h)), b.label


def test_two_calls_back_to_back_on_one_stream(device):
    """Both calls queued before either has run: each has its own staged arrays and its own
    scratch, and the second's outputs are not the first's."""
    a, b = M.batch(70), M.batch(3)
    oa, ob = device.outputs(a, False), device.outputs(b, True)
    device.upload(a), device.upload(b)
    device.launch(a, oa, left=False)  # quota left in scratch
    device.launch(b, ob)
    check(lib.krk_stream_sync(None))
    assert M.compare(a, device.read(a, oa, False), left=False) == [] and M.compare(b, device.read(b, ob, True)) == []


def test_the_host_arrays_may_be_overwritten_when_the_call_returns(device):
    b = M.batch(70)
    outs = device.outputs(b, False)
    bits, quota = device.upload(b)
    a = M.call_args(b, bits.ptr, quota.ptr, [o.ptr for o in outs])
    check(lib.krk_piece_resend_round_dev(*a, None))
    for s, r in zip(a[0], a[1]):  # the call has staged its copies
        s.n_pieces, s.n_peers, s.bits_off, r.failed_off, r.n_failed = 1, 1, 0, 0, 1
    for e in a[5]:
        e.piece, e.peer, e.status = 0, 0, 2
    check(lib.krk_stream_sync(None))
    assert M.compare(b, device.read(b, outs, False)) == []


def test_refusals_come_before_any_launch(device):
    label, b, _ = M.invalid_calls()[0]
    bits, quota = device.upload(b)
    outs = device.outputs(b, False)
    pageable = [M.prefilled(k) for k in b.sizes()]
    host_bits, host_quota = b.bits.copy(), b.quota.copy()

    def call(change=None, **kw):
        a = M.call_args(b, bits.ptr, quota.ptr, [o.ptr for o in outs])
        if change:
            change(a)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.krk_piece_resend_round_dev(*a, None)

    E = _capi.KRK_EINVAL
    with D.KernelTimer():
        for label, _, change in M.invalid_calls():  # the list checks run on the host, before the launch
            assert call(change) == E and b"piece_resend_round_dev" in lib.krk_last_error(), label
        assert call(_3=host_bits.ctypes.data) == E and call(_4=host_quota.ctypes.data) == E
        for k in range(3):
            assert call(**{f"_{6 + k}": pageable[k].ctypes.data}) == E
        assert call(_3=bits.ptr + 4) == E and b"aligned" in lib.krk_last_error()
        assert call(_4=quota.ptr + 2) == E
        for k in range(3):
            assert call(**{f"_{6 + k}": outs[k].ptr + 2}) == E
        D.synchronize()
        assert D.KernelTimer.stats("piece_resend")[0] == 0
        for o, k in zip(outs, b.sizes()):
            assert (o.to_host(np.uint32, k) == M.CANARY32).all()
        for p in pageable:
            assert (p == M.CANARY32).all()
        # the accepted neighbour: one timed call, its work units the torrents
        assert call() == _capi.KRK_OK
        D.synchronize()
        assert D.KernelTimer.stats("piece_resend")[0] == 1
        assert [u for _, u, _, _ in D.KernelTimer.timeline("piece_resend")] == [len(b.torrents)]
    assert M.compare(b, device.read(b, outs, False)) == []


def test_wrappers_and_output_holder(device):
    """device.piece_resend_round_dev over a RequestBatch and a ResendBatch with a ResendOutputs
    holder (device and pinned) and without one, against device.piece_resend_round."""
    rng = np.random.default_rng(M.SEED)
    batch = D.RequestBatch([1000, 65, 0, 1], [5, 2, 1, 3], [0, D.PR_SAMPLE, 0, D.PR_ALLOW_DUPLICATES])
    bits = rng.integers(0, 1 << 64, size=batch.total_words, dtype=np.uint64)
    for t in range(len(batch)):
        batch.rows(bits, t)[0] &= rng.integers(0, 1 << 64, size=int(batch.words[t]), dtype=np.uint64)
    quota = rng.integers(-1, 4, size=batch.total_peers).astype(np.int32)
    lists = [sorted((int(rng.integers(0, 1000)), int(rng.integers(0, 5)), int(rng.integers(1, 4))) for _ in range(40)),
             [(3, D.PR_NONE, D.PR_EXPIRED), (64, 1, D.PR_UNSENT)], [], [(0, 0, D.PR_INVALID)] * 3]
    resend = D.ResendBatch(batch, lists)
    want = D.piece_resend_round(batch, resend, bits, quota)
    assert want[2].sum() > 0
    bits_dev, quota_dev = D.DeviceBuffer(bits.nbytes), D.DeviceBuffer(quota.nbytes)
    bits_dev.from_host(bits)
    quota_dev.from_host(quota)
    for pinned in (False, True):
        out = D.ResendOutputs(batch, resend, pinned=pinned)
        out.fill(0xA5)
        assert D.piece_resend_round_dev(batch, resend, bits_dev, quota_dev, out=out) is out
        check(lib.krk_stream_sync(None))
        assert all(np.array_equal(g, w) for g, w in zip(out.to_host(), want))
    tg, lf, nr = D.piece_resend_round_dev(batch, resend, bits_dev, quota_dev, quota_left=False)
    assert lf is None and np.array_equal(tg, want[0]) and np.array_equal(nr, want[2])
