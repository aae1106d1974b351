"""Piece request rounds where no GPU is: the host forms (krk_piece_availability, krk_piece_select,
krk_piece_request_round) against tests/piece_request_ref.py's restatement over the whole matrix
(tests/piece_request_matrix.py), every output stored into 0xA5-prefilled buffers; the refusals;
KRK_ENODEV from the device form on a box without a device; the reference's manager_test.go
scenarios (tests/golden/piece_requests.json) replayed through piecerequest.Manager with a mock
clock; and KRK_PR_SAMPLE's uniformity."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from kraken_amd import _capi, device as D, piecerequest as PR
from kraken_amd._capi import lib
from tests import piece_request_matrix as M
from tests import piece_request_ref as R

u32p, u64p, i32p = M.u32p, M.u64p, M.i32p
E = _capi.KRK_EINVAL


# ------------------------------------------------------------------ the restatement itself
def test_the_restatements_vector_key_is_its_scalar_key():
    assert R.splitmix64(0) == 0xE220A8397B1DCDAF  # splitmix64's first output from state 0
    rng = np.random.default_rng(3)
    idx = rng.integers(0, 1 << 32, size=200, dtype=np.uint64)
    for seed, peer in ((0, 0), (0xFFFFFFFFFFFFFFFF, 299), (int(rng.integers(0, 1 << 63)), 7)):
        assert R.sample_keys_np(seed, peer, idx).tolist() == [R.sample_key(seed, peer, int(i)) for i in idx]


def test_matrix_covers_what_it_claims():
    G, S = M.G, M.S
    assert S % 64 == 0 and S >= 128 and G % S == 0 and M.LMAX >= 16
    assert set(M.NS) == {0, 1, 63, 64, 65, S - 1, S, S + 1, G - 1, G, G + 1, 2 * G + 1, 81920}
    cs = M.cases()
    ts = [b.torrents[0] for b in cs]
    assert {t.n for t in ts} == set(M.NS) and {t.n_peers for t in ts} >= set(M.PS) and {b.limit for b in cs} == set(M.LS)
    assert {int(q) for t in ts for q in t.quota} >= {-1, 0, 1, 3, M.LMAX}
    assert {t.kind for t in ts} == {"random", "equal", "ties", "first", "last", "ones", "have_full", "blocked_full", "twins"}
    # all counts equal: the picks are the lowest indices, peer after peer
    t = next(t for t in ts if t.kind == "equal" and t.n == 2 * G + 1 and t.n_peers == 3 and t.flags == M.RAREST)
    assert t.want(3)[1].tolist() == [[0, 1, 2], [3, 4, 5], [6, 7, 8]]
    # ties on both sides of the word / wave boundary, of the thread stride and of the pass, and the last piece
    t = next(t for t in ts if t.kind == "ties" and t.n == 2 * G + 1 and t.n_peers == 10)
    picked = t.want(M.LMAX)[1].reshape(-1)
    assert picked[picked != R.NONE].tolist() == sorted(set(M.TIES))
    assert {63, 64, S - 1, S, G - 1, G} <= set(M.TIES) and len(set(M.TIES)) < 10 * M.LMAX
    t = next(t for t in ts if t.kind == "ties" and t.n == 2 * G + 1 and t.n_peers == 3 and t.flags == M.RAREST)
    assert t.want(3)[1].tolist() == [[62, 63, 64], [65, S - 2, S - 1], [S, S + 1, 2 * S - 1]]
    for t in ts:
        c, pk, npk = t.want(next(b.limit for b in cs if b.torrents[0] is t))
        if t.kind == "first" and t.n:
            assert pk[0, 0] == 0 and npk.sum() == (1 if not t.flags & M.DUP else t.n_peers)
        if t.kind == "last":
            assert pk[0, 0] == t.n - 1
        if t.kind in ("ones", "have_full", "blocked_full"):
            assert npk.sum() == 0
        if t.kind == "ones":
            assert (c == t.n_peers).all()
    # counts no 8-bit counter holds
    assert any(t.n_peers == 300 and t.want(M.LMAX)[0].max() == 300 for t in ts if t.kind == "equal")
    # twins: with allow-duplicates both get the same pieces, without the second gets the next ones
    # (rarest first; a sampled key depends on the peer, so sampled twins only never share a piece)
    for flags in (M.RAREST, M.SAMPLE):
        a = next(t for t in ts if t.kind == "twins" and t.flags == flags and t.n == 2 * G + 1).want(3)[1]
        d = next(t for t in ts if t.kind == "twins" and t.flags == flags | M.DUP and t.n == 2 * G + 1).want(3)[1]
        assert not set(a[0]) & set(a[1]) and d[0].tolist() == a[0].tolist()
        if flags == M.RAREST:
            assert d[1].tolist() == d[0].tolist()
    b = M.batch(70)
    assert len(b.torrents) == 70 and b.torrents[35].n == 0 and b.torrents[36].n_peers == 0
    assert {t.n for t in b.torrents} >= set(M.NS) - {0} and sum((t.n + S - 1) // S for t in b.torrents) > M.MAX_WG


# ------------------------------------------------------------------ the host forms over the matrix
def test_host_round_equals_the_restatement_over_the_matrix():
    calls, bad = M.run_cases(M.HostBackend(), M.cases())
    assert calls == 2 * len(M.cases()) and bad == [], f"{len(bad)} mismatches of {calls} calls, first {bad[:5]}"


@pytest.mark.parametrize("k", [0, 1, 3, 70])
def test_host_round_batches(k):
    for limit in (3, M.LMAX) if k == 3 else (3,):
        calls, bad = M.run_cases(M.HostBackend(), [M.batch(k, limit)])
        assert calls == 2 and bad == [], bad[:5]


def test_availability_and_select_equal_the_restatement():
    checked = 0
    for b in M.cases():
        t = b.torrents[0]
        if t.n > 2 * M.S + 1 or t.n_peers > 10:
            continue
        W = M.words(t.n)
        peers = np.ascontiguousarray(t.rows[1::2])
        counts = np.full(t.n + M.SPARE, M.CANARY32, dtype=np.uint32)
        assert lib.krk_piece_availability(peers.ctypes.data_as(u64p) if peers.size else None, t.n_peers, t.n,
                                          counts.ctypes.data_as(u32p)) == 0
        want = R.availability(t.rows[1::2], t.n)
        assert np.array_equal(counts[:t.n], want) and (counts[t.n:] == M.CANARY32).all(), t.label
        have = R.bools(t.rows[0], t.n)
        for p in range(t.n_peers):
            for q in (-1, 0, 1, b.limit):
                cand = np.ascontiguousarray(t.rows[1 + 2 * p] & ~t.rows[0])  # tail bits still set
                blocked = np.ascontiguousarray(t.rows[2 + 2 * p])
                picks = np.full(max(q, 0) + M.SPARE, M.CANARY32, dtype=np.uint32)
                m = C.c_uint32(0xA5A5A5A5)
                assert lib.krk_piece_select(cand.ctypes.data_as(u64p) if W else None,
                                            blocked.ctypes.data_as(u64p) if W else None,
                                            want.ctypes.data_as(u32p) if t.n else None, t.n, q, t.flags & 0xFF, t.seed, p,
                                            picks.ctypes.data_as(u32p), C.byref(m)) == 0, lib.krk_last_error()
                w = R.select(R.bools(t.rows[1 + 2 * p], t.n) & ~have & ~R.bools(blocked, t.n), want, q, t.flags & 0xFF,
                             t.seed, p)
                k = max(q, 0)
                assert m.value == len(w) and picks[:len(w)].tolist() == w, (t.label, p, q)
                assert (picks[len(w):k] == R.NONE).all() and (picks[k:] == M.CANARY32).all(), (t.label, p, q)
                checked += 1
    assert checked > 500


def test_select_blocked_and_counts_are_nullable():
    cand = np.array([0b1011], dtype=np.uint64)
    picks = np.zeros(4, dtype=np.uint32)
    m = C.c_uint32()
    # rarest first, the reference's own example: candidates 1101, counts 2,3,1,0, limit 2 -> [3, 0]
    counts = np.array([2, 3, 1, 0], dtype=np.uint32)
    assert lib.krk_piece_select(cand.ctypes.data_as(u64p), None, counts.ctypes.data_as(u32p), 4, 2, M.RAREST, 0, 0,
                                picks.ctypes.data_as(u32p), C.byref(m)) == 0
    assert m.value == 2 and picks[:2].tolist() == [3, 0]
    assert lib.krk_piece_select(cand.ctypes.data_as(u64p), None, None, 4, 4, M.SAMPLE, 9, 1,
                                picks.ctypes.data_as(u32p), C.byref(m)) == 0
    assert m.value == 3 and picks[:3].tolist() == R.select(np.array([1, 1, 0, 1], bool), None, 4, M.SAMPLE, 9, 1)
    assert picks[3] == R.NONE


# ------------------------------------------------------------------ refusals
def _round_args(b):
    c, pk, npk = (M.prefilled(k) for k in b.sizes())
    return c, pk, npk, [b.structs, len(b.torrents), b.bits.ctypes.data_as(u64p), b.quota.ctypes.data_as(i32p), b.limit,
                        c.ctypes.data_as(u32p), pk.ctypes.data_as(u32p), npk.ctypes.data_as(u32p)]


def _refusals(b, call, extra=()):
    """Every refusal of the error table through `call` (the host round, or the device round with a
    trailing stream argument): KRK_EINVAL, and no output touched."""
    c, pk, npk, good = _round_args(b)
    outs = (c, pk, npk)

    def with_(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return call(*a, *extra)

    S = _capi.krk_request_torrent
    t = b.torrents[0]
    w, p, i = b.offs[0]
    one = lambda **kw: (S * 1)(S(**{**dict(n_pieces=t.n, n_peers=t.n_peers, flags=t.flags, seed=t.seed, bits_off=w,
                                             peer_off=p, piece_off=i), **kw}))
    assert with_(_0=one(n_pieces=1 << 32), _1=1) == E and b"2^32" in lib.krk_last_error()
    assert with_(_0=one(flags=2), _1=1) == E and b"invalid piece selection policy" in lib.krk_last_error()
    assert with_(_0=one(flags=M.RAREST | 0x200), _1=1) == E
    for limit in (0, M.LMAX + 1, 0xFFFFFFFF):
        assert with_(_4=limit) == E and b"limit" in lib.krk_last_error()
    assert with_(_0=None) == E
    assert with_(_2=None) == E
    assert with_(_3=None) == E
    assert with_(_6=None) == E
    assert with_(_7=None) == E
    for o in outs:
        assert (o == M.CANARY32).all()
    return with_, outs


def test_host_round_refusals_touch_no_output():
    b = M.single("random", 65, 2, M.RAREST, 3, quota=[3, 3])
    with_, outs = _refusals(b, lib.krk_piece_request_round)
    q = b.quota.copy()
    q[b.offs[0][1] + 1] = 4  # above the limit
    assert with_(_3=q.ctypes.data_as(i32p)) == E and b"quota 4 above the limit 3" in lib.krk_last_error()
    for o in outs:
        assert (o == M.CANARY32).all()
    assert with_() == 0 and M.compare(b, outs) == []  # the accepted neighbour
    # no torrents: nothing is read, nothing is written
    assert lib.krk_piece_request_round(None, 0, None, None, 3, None, None, None) == 0
    assert lib.krk_piece_request_round(None, 0, None, None, 0, None, None, None) == E


def test_availability_and_select_refusals():
    out = M.prefilled(8)
    op = out.ctypes.data_as(u32p)
    w = np.zeros(1, dtype=np.uint64)
    wp = w.ctypes.data_as(u64p)
    m = C.c_uint32(0xA5A5A5A5)
    assert lib.krk_piece_availability(wp, 1, 1 << 32, op) == E
    assert lib.krk_piece_availability(None, 1, 8, op) == E
    assert lib.krk_piece_availability(wp, 1, 8, None) == E
    assert lib.krk_piece_select(wp, None, op, 1 << 32, 1, M.RAREST, 0, 0, op, C.byref(m)) == E
    assert lib.krk_piece_select(wp, None, op, 8, 1, 2, 0, 0, op, C.byref(m)) == E
    assert lib.krk_piece_select(wp, None, op, 8, M.LMAX + 1, M.RAREST, 0, 0, op, C.byref(m)) == E
    assert lib.krk_piece_select(None, None, op, 8, 1, M.RAREST, 0, 0, op, C.byref(m)) == E
    assert lib.krk_piece_select(wp, None, None, 8, 1, M.RAREST, 0, 0, op, C.byref(m)) == E  # rarest first reads counts
    assert lib.krk_piece_select(wp, None, op, 8, 1, M.RAREST, 0, 0, None, C.byref(m)) == E
    assert lib.krk_piece_select(wp, None, op, 8, 1, M.RAREST, 0, 0, op, None) == E
    assert (out == M.CANARY32).all() and m.value == 0xA5A5A5A5
    assert lib.krk_piece_availability(None, 0, 0, None) == 0
    assert lib.krk_piece_select(None, None, None, 0, 3, M.RAREST, 0, 0, op, C.byref(m)) == 0 and m.value == 0
    assert out[:4].tolist() == [R.NONE] * 3 + [int(M.CANARY32)]


def test_round_dev_without_a_device():
    """The refusals need no device; a real call needs a gfx950 device (KRK_ENODEV here when there is
    none -- with one, tests/test_gpu_piece_request_matrix.py): there is no fall-back to the host form."""
    b = M.single("random", 65, 2, M.RAREST, 3, quota=[3, 3])
    with_, outs = _refusals(b, lib.krk_piece_request_round_dev, extra=(None,))
    assert lib.krk_piece_request_round_dev(None, 0, None, None, 3, None, None, None, None) == 0
    if D.device_count() == 0:
        assert with_() == _capi.KRK_ENODEV
        for o in outs:
            assert (o == M.CANARY32).all()
        with pytest.raises(_capi.KrakenError) as e:
            PR.ReserveRound([_dispatcher(65, 2, PR.RarestFirstPolicy, 3, 1)], placement="gpu")
        assert e.value.code == _capi.KRK_ENODEV


# ------------------------------------------------------------------ piecerequest.Manager
def _golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "piece_requests.json")) as f:
        return json.load(f)


GOLDEN = _golden()
STATUS = {"unsent": PR.StatusUnsent, "invalid": PR.StatusInvalid, "expired": PR.StatusExpired}


def test_new_manager_refuses_an_unknown_policy():
    with pytest.raises(ValueError, match="^invalid piece selection policy: rarest$"):
        PR.NewManager(PR.MockClock(), 5, "rarest", 3)
    assert PR.NewManager(PR.MockClock(), 5, PR.DefaultPolicy, 3).pipelineLimit == 3


@pytest.mark.parametrize("sc", GOLDEN["scenarios"], ids=lambda s: s["name"])
def test_manager_replays_the_references_scenarios(sc):
    clk = PR.MockClock()
    timeout = GOLDEN["timeout_seconds"] * 10**9  # nanoseconds, as time.Duration
    m = PR.NewManager(clk, timeout, sc["policy"], sc["limit"])
    for st in sc["steps"]:
        op = st["op"]
        if op == "reserve":
            got = m.ReservePieces(st["peer"], [c == "1" for c in st["candidates"]], st["counts"], st["allow_duplicates"])
            if "want" in st:
                want = st["want"]
                assert (got == want) if sc["policy"] == PR.RarestFirstPolicy else (sorted(got) == want), (st, got)
            if st.get("want_len") is not None:
                assert len(got) == st["want_len"] and len(set(got)) == len(got), (st, got)
        elif op in ("unsent", "invalid"):
            (m.MarkUnsent if op == "unsent" else m.MarkInvalid)(st["peer"], st["piece"])
        elif op == "clear":
            m.Clear(st["piece"])
        elif op == "clear_peer":
            m.ClearPeer(st["peer"])
        elif op == "advance_past_timeout":
            clk.Add(timeout + 1)
        elif op == "pending":
            assert m.PendingPieces(st["peer"]) == st["want"], st
        elif op == "pending_len":
            assert len(m.PendingPieces(st["peer"])) == st["want"], st
        elif op == "failed":
            failed = m.GetFailedRequests()
            assert len(failed) == len(st["want"])
            for piece, peer, status in st["want"]:
                assert PR.Request(piece, peer, STATUS[status]) in failed, (st, failed)
        else:
            raise AssertionError(op)


def test_an_expired_request_expires_strictly_after_its_timeout():
    clk = PR.MockClock()
    m = PR.NewManager(clk, 5, PR.RarestFirstPolicy, 1)
    assert m.ReservePieces("a", [True], [0], False) == [0]
    clk.Add(5)  # not AFTER sentAt + timeout yet
    assert m.ReservePieces("b", [True], [0], False) == [] and m.GetFailedRequests() == []
    clk.Add(1)
    assert m.GetFailedRequests() == [PR.Request(0, "a", PR.StatusExpired)]
    assert m.ReservePieces("b", [True], [0], False) == [0]


# ------------------------------------------------------------------ ReserveRound on the host
def _dispatcher(n, n_peers, policy, limit, seed):
    rng = np.random.default_rng([M.SEED, n, seed])
    d = PR.Dispatcher(n, PR.NewManager(PR.MockClock(), 5, policy, limit, seed=seed))
    for p in range(n_peers):
        d.AddPeer(f"peer-{p}", rng.random(n) < 0.5)
    return d


def test_reserve_round_is_reserve_pieces_peer_after_peer():
    """One round over a torrent equals ReservePieces called for its peers in order at one clock
    instant (rarest first: the picks are a function of the counts, so the two must agree exactly)."""
    for n in (65, 1000):
        a, b = (_dispatcher(n, 5, PR.RarestFirstPolicy, 3, 2) for _ in range(2))
        a.disable_endgame = b.disable_endgame = True
        got = PR.ReserveRound([a])[0]
        counts = b.numPeersByPiece()
        for peerID, bits in b.peers.items():
            assert got[peerID] == b.manager.ReservePieces(peerID, bits & ~b.have, counts, False), (n, peerID)
            assert a.manager.PendingPieces(peerID) == b.manager.PendingPieces(peerID) == sorted(got[peerID])
        assert sum(len(v) for v in got.values()) == 15
        assert PR.ReserveRound([a])[0] == {p: [] for p in a.peers}  # every quota is used up
    assert PR.ReserveRound([]) == []
    with pytest.raises(ValueError):
        PR.ReserveRound([a], placement="auto")


# ------------------------------------------------------------------ KRK_PR_SAMPLE's uniformity
def test_sample_policy_is_uniform_over_the_candidates():
    """16 candidates, L = 3, 20,000 rounds with seed = splitmix64(s), s = 0 .. 19,999: each
    candidate's hit count within 5 binomial standard deviations (sqrt(20000 * 3/16 * 13/16) ~ 55.2)
    of 3,750.  The restatement gives a worst deviation of 1.92 sigma; the run is deterministic.  Raw
    s as the seed would make every block of 16 consecutive seeds an exact permutation (the xor with
    the piece index), and the test would pass trivially."""
    rounds, n, limit = 20000, 16, 3
    batch = D.RequestBatch([n] * rounds, 1, D.PR_SAMPLE, [R.splitmix64(s) for s in range(rounds)])
    bits = np.zeros((rounds, 3), dtype=np.uint64)
    bits[:, 1] = 0xFFFF
    _, picks, n_picked = D.piece_request_round(batch, bits.reshape(-1), np.full(rounds, limit, np.int32), limit)
    assert (n_picked == limit).all()
    hits = np.bincount(picks.reshape(-1), minlength=n)
    assert hits.size == n and hits.sum() == rounds * limit
    sigma = math.sqrt(rounds * (limit / n) * (1 - limit / n))
    worst = float(np.abs(hits - rounds * limit / n).max() / sigma)
    print(f"worst deviation {worst:.2f} sigma, hits {hits.tolist()}")
    assert worst <= 5.0, (worst, hits.tolist())
    # and the library's picks are the restatement's, round for round
    for s in (0, 1, 19999):
        want = R.select(np.ones(n, bool), None, limit, R.SAMPLE, R.splitmix64(s), 0)
        assert picks[s].tolist() == want
