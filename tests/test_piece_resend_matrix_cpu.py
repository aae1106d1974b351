"""Resend rounds where no GPU is: the host form krk_piece_resend_round against
tests/piece_resend_ref.py's restatement over the whole matrix (tests/piece_resend_matrix.py), every
output stored into 0xA5-prefilled buffers; the named cases against the targets worked out by hand;
the refusals, with the outputs untouched; the device.py wrappers; and KRK_ENODEV from the device
form on a box without a device."""
import ctypes as C

import numpy as np
import pytest

from kraken_amd import _capi, device as D
from kraken_amd._capi import lib
from tests import piece_resend_matrix as M
from tests import piece_resend_ref as R

E = _capi.KRK_EINVAL


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_matrix_covers_what_it_claims():
    S = M.S
    assert S % 64 == 0 and S >= 128
    ts = [b.torrents[0] for b in M.cases()]
    assert {t.n_peers for t in ts} == {0, 1, 2, S - 1, S, S + 1, 2 * S + 1}
    assert {t.n for t in ts} == {1, 63, 64, 65, 4097} and {len(t.failed) for t in ts} == {0, 1, 2, 300}
    assert {t.flags for t in ts} == {0, M.DUP}
    assert {s for t in ts for _, _, s in t.failed} == {M.EXPIRED, M.UNSENT, M.INVALID}
    assert any(p == M.NONE for t in ts for _, p, _ in t.failed)
    assert {int(q) for t in ts for q in t.quota} >= {-1, 0, 1}
    # the random torrents reach every pass, hit and miss, and resend one piece to two peers only with duplicates
    got = np.concatenate([t.want()[0] for t in ts])
    assert (got == M.NONE).any() and (got < S).any() and ((got >= S) & (got < 2 * S)).any()
    for t in ts:
        tg = t.want()[0]
        hit = [(i, int(p)) for (i, _, _), p in zip(t.failed, tg) if p != M.NONE]
        assert len(set(hit)) == len(hit), t.label
        if not t.flags & M.DUP:
            assert len({i for i, _ in hit}) == len(hit), t.label
    assert any(len({i for i, _ in h}) < len(h) for h in
               ([(i, int(p)) for (i, _, _), p in zip(t.failed, t.want()[0]) if p != M.NONE] for t in ts if t.flags & M.DUP))
    # a quota that runs out inside a list
    assert any((t.want()[1] == 0).any() and (t.quota > 0)[t.want()[1] == 0].any() for t in ts)
    b = M.batch(70)
    assert len(b.torrents) == 70 and not b.torrents[35].failed and b.torrents[36].n_peers == 0 and b.torrents[36].failed
    assert all(o > 0 for offs in b.offs for o in offs)


@pytest.mark.parametrize("k", range(len(M.named())), ids=lambda k: M.named()[k][0].label.replace(" ", "_"))
def test_named_cases_by_hand(k):
    """The targets worked out by hand are the restatement's and the host form's."""
    b, targets = M.named()[k]
    t = b.torrents[0]
    assert t.want()[0].tolist() == targets, b.label
    assert t.want()[2] == sum(x != M.NONE for x in targets)
    for left in (True, False):
        assert M.compare(b, M.HostBackend().run(b, left=left), left) == []


def test_host_round_equals_the_restatement_over_the_matrix():
    calls, bad = M.run_cases(M.HostBackend(), M.cases())
    assert calls == 2 * len(M.cases()) and bad == [], f"{len(bad)} mismatches of {calls} calls, first {bad[:5]}"


@pytest.mark.parametrize("k", [0, 1, 3, 70])
def test_batches(k):
    b = M.batch(k)
    calls, bad = M.run_cases(M.HostBackend(), [b])
    assert calls == 2 and bad == [], bad[:5]


def test_zero_torrents_take_null_everywhere():
    assert lib.krk_piece_resend_round(None, None, 0, None, None, None, None, None, None) == _capi.KRK_OK


@pytest.mark.parametrize("k", range(len(M.invalid_calls())), ids=lambda k: M.invalid_calls()[k][0].replace(" ", "_"))
def test_refusals_touch_no_output(k):
    label, b, change = M.invalid_calls()[k]
    outs = [M.prefilled(n) for n in b.sizes()]
    good = M.call_args(b, b.bits.ctypes.data_as(M.u64p), b.quota.ctypes.data_as(M.i32p),
                       [outs[0].ctypes.data_as(M.u32p), outs[1].ctypes.data_as(M.i32p), outs[2].ctypes.data_as(M.u32p)])
    bad = list(good)
    change(bad)
    assert lib.krk_piece_resend_round(*bad) == E, label
    assert b"piece_resend_round" in lib.krk_last_error()
    assert all((o == M.CANARY32).all() for o in outs), label
    if not label.startswith("NULL"):  # the same call with the change undone is accepted
        good = M.call_args(b, *good[3:5], good[6:])
        assert lib.krk_piece_resend_round(*good) == _capi.KRK_OK
        assert M.compare(b, (outs[0], outs[1].view(np.int32), outs[2])) == []


def test_a_list_of_2_32_entries_is_out_of_range():
    b = M.invalid_calls()[0][1]
    outs = [M.prefilled(n) for n in b.sizes()]
    a = M.call_args(b, b.bits.ctypes.data_as(M.u64p), b.quota.ctypes.data_as(M.i32p),
                    [outs[0].ctypes.data_as(M.u32p), outs[1].ctypes.data_as(M.i32p), outs[2].ctypes.data_as(M.u32p)])
    a[1][0].n_failed = 1 << 32
    assert lib.krk_piece_resend_round(*a) == _capi.KRK_ERANGE
    assert all((o == M.CANARY32).all() for o in outs)


def test_wrappers():
    """device.piece_resend_round over a RequestBatch and a ResendBatch against the restatement."""
    rng = np.random.default_rng(M.SEED)
    batch = D.RequestBatch([1000, 65, 0, 1], [5, 2, 1, 3], [0, D.PR_SAMPLE, 0, D.PR_ALLOW_DUPLICATES])
    bits = rng.integers(0, 1 << 64, size=batch.total_words, dtype=np.uint64)
    for t in range(len(batch)):  # a sparse have, so that something is resent
        batch.rows(bits, t)[0] &= rng.integers(0, 1 << 64, size=int(batch.words[t]), dtype=np.uint64)
    quota = rng.integers(-1, 4, size=batch.total_peers).astype(np.int32)
    lists = [sorted((int(rng.integers(0, 1000)), int(rng.integers(0, 5)), int(rng.integers(1, 4))) for _ in range(40)),
             [(3, D.PR_NONE, D.PR_EXPIRED), (64, 1, D.PR_UNSENT)], [], [(0, 0, D.PR_INVALID)] * 3]
    resend = D.ResendBatch(batch, lists)
    assert resend.total_failed == 45 and resend.failed_off.tolist() == [0, 40, 42, 42, 45]
    target, left, n_resent = D.piece_resend_round(batch, resend, bits, quota)
    for t in range(len(batch)):
        n, P = int(batch.n_pieces[t]), int(batch.n_peers[t])
        p0 = int(batch.peer_off[t])
        tg, lf, nr = R.resend_torrent(batch.rows(bits, t), n, P, int(batch.flags[t]), quota[p0:p0 + P], lists[t])
        assert resend.split(target, t).tolist() == tg.tolist() and left[p0:p0 + P].tolist() == lf.tolist()
        assert int(n_resent[t]) == nr
    assert n_resent.sum() > 0
    t2, none, n2 = D.piece_resend_round(batch, resend, bits, quota, quota_left=False)
    assert none is None and np.array_equal(t2, target) and np.array_equal(n2, n_resent)
    assert D.piece_resend_geometry() == M.S
    with pytest.raises(ValueError):
        D.ResendBatch(batch, lists[:2])


def test_device_form_is_enodev_without_a_device():
    n = C.c_int(-1)
    _capi.check(lib.krk_device_count(C.byref(n)))
    if n.value > 0:
        pytest.skip("a GPU is visible")
    b = M.batch(3)
    outs = [M.prefilled(k) for k in b.sizes()]
    a = M.call_args(b, ptr(b.bits), ptr(b.quota), [ptr(o) for o in outs])
    assert lib.krk_piece_resend_round_dev(*a, None) == _capi.KRK_ENODEV
    assert b"no HIP device" in lib.krk_last_error()
    assert all((o == M.CANARY32).all() for o in outs)
    # the list checks come first, as in the host form
    a[5][b.offs[0][2]].status = 7
    assert lib.krk_piece_resend_round_dev(*a, None) == E
    assert lib.krk_piece_resend_round_dev(None, None, 0, None, None, None, None, None, None, None) == _capi.KRK_OK
