"""kraken_amd.connstate: State against the reference's own unit cases restated
(lib/torrent/scheduler/connstate/state_test.go), ConnRound against the same events applied one at a
time to a State in phase order, PreemptionSweep against the restatement, and one drive through the
existing classes: peerstore.AnnounceRound's handouts fed to ConnRound.announce_result, the admitted
peers established, the active sets exactly what tests/conn_ref.py's restatement gives."""
import numpy as np
import pytest

from kraken_amd import connstate as CS, device as D, peerstore as PS
from kraken_amd.piecerequest import MockClock
from tests import conn_ref as R

H = "hash-0"


def state(clock=None, **config):
    return CS.State(CS.Config(**config), clock or MockClock(1000), "local-peer")


def test_config_defaults_and_error_strings():
    c = CS.Config().applyDefaults()
    assert (c.MaxOpenConnectionsPerTorrent, c.MaxMutualConnections, c.BlacklistDuration, c.DisableBlacklist) == (10, 10, 30, False)
    assert CS.Config(MaxOpenConnectionsPerTorrent=20).applyDefaults().MaxMutualConnections == 20
    assert CS.Config(MaxMutualConnections=5, MaxOpenConnectionsPerTorrent=20).applyDefaults().MaxMutualConnections == 5
    assert [str(e) for e in (CS.ErrTorrentAtCapacity, CS.ErrConnAlreadyPending, CS.ErrConnAlreadyActive, CS.ErrConnClosed,
                             CS.ErrInvalidActiveTransition, CS.ErrTooManyMutualConns)] == [
        "torrent is at capacity", "conn is already pending", "conn is already active", "conn is closed",
        "conn must be pending to transition to active", "conn has too many mutual connections"]
    assert state().MaxConnsPerTorrent() == 10


def test_blacklist_expires_after_the_duration():
    """TestStateBlacklist."""
    clk = MockClock(1000)
    s = state(clk, BlacklistDuration=30)
    assert s.Blacklist("p", H) is None
    assert s.Blacklisted("p", H)
    assert str(s.Blacklist("p", H)) == "conn is already blacklisted"
    clk.Add(30)
    assert not s.Blacklisted("p", H)  # expiry == now: no time remains
    clk.Add(-1)
    assert s.Blacklisted("p", H)
    clk.Add(2)  # duration + 1
    assert not s.Blacklisted("p", H)
    assert s.Blacklist("p", H) is None


def test_blacklist_snapshot():
    """TestStateBlacklistSnapshot."""
    s = state(BlacklistDuration=30)
    assert s.Blacklist("p", H) is None
    assert s.BlacklistSnapshot() == [CS.BlacklistedConn("p", H, 30)]


def test_clear_blacklist():
    """TestStateClearBlacklist."""
    s = state()
    peers = [f"p{i}" for i in range(10)]
    for p in peers:
        assert s.Blacklist(p, H) is None and s.Blacklisted(p, H)
    assert s.Blacklist("q", "other") is None
    s.ClearBlacklist(H)
    assert not any(s.Blacklisted(p, H) for p in peers)
    assert s.Blacklisted("q", "other")
    assert not s.torrents[H].expiry.any()


def test_disable_blacklist():
    s = state(DisableBlacklist=True)
    assert s.Blacklist("p", H) is None and not s.Blacklisted("p", H)


def test_blacklist_frees_nothing():
    s = state(MaxOpenConnectionsPerTorrent=2)
    c = CS.Conn("a", H)
    assert s.AddPending("a", H) is None and s.MovePendingToActive(c) is None and s.AddPending("b", H) is None
    assert s.Blacklist("a", H) is None and s.Blacklist("b", H) is None  # an active and a pending conn
    assert s.NumActiveConns() == 1 and s.AddPending("c", H) is CS.ErrTorrentAtCapacity
    assert s.AddPending("a", H) is CS.ErrTorrentAtCapacity


def test_add_pending_prevents_duplicates():
    s = state()
    assert s.AddPending("p", H) is None
    assert s.AddPending("p", H) is CS.ErrConnAlreadyPending


def test_add_pending_reserves_capacity():
    s = state(MaxOpenConnectionsPerTorrent=10)
    for i in range(10):
        assert s.AddPending(f"p{i}", H) is None
    assert s.AddPending("one more", H) is CS.ErrTorrentAtCapacity
    assert s.AddPending("elsewhere", "other") is None  # capacity is a torrent's


def test_delete_pending_allows_future_add_pending_and_frees_capacity():
    s = state(MaxOpenConnectionsPerTorrent=1)
    assert s.AddPending("p1", H) is None
    assert s.AddPending("p2", H) is CS.ErrTorrentAtCapacity
    s.DeletePending("p1", H)
    s.DeletePending("p1", H)  # a no-op the second time: nothing more is freed
    assert s.AddPending("p2", H) is None
    assert s.AddPending("p1", H) is CS.ErrTorrentAtCapacity


def test_move_pending_to_active_rules():
    s = state()
    c = CS.Conn("p", H)
    assert s.MovePendingToActive(c) is CS.ErrInvalidActiveTransition
    assert s.AddPending("p", H) is None
    assert s.MovePendingToActive(c) is None
    assert s.MovePendingToActive(c) is CS.ErrInvalidActiveTransition
    assert s.AddPending("p", H) is CS.ErrConnAlreadyActive
    closed = CS.Conn("q", H)
    assert s.AddPending("q", H) is None
    closed.Close()
    assert s.MovePendingToActive(closed) is CS.ErrConnClosed


def test_delete_active_frees_capacity_and_noops_on_another_conn():
    s = state(MaxOpenConnectionsPerTorrent=1)
    c = CS.Conn("p", H)
    assert s.AddPending("p", H) is None and s.MovePendingToActive(c) is None
    assert s.AddPending("p2", H) is CS.ErrTorrentAtCapacity
    s.DeleteActive(CS.Conn("p", H))  # the same key, another conn
    s.DeleteActive(CS.Conn("never seen", H))
    assert s.AddPending("p2", H) is CS.ErrTorrentAtCapacity and s.ActiveConns() == [c]
    s.DeleteActive(c)
    assert s.AddPending("p2", H) is None and not s.Blacklisted("p", H)


def test_active_conns():
    s = state()
    conns = [CS.Conn(f"p{i}", H) for i in range(10)]
    for c in conns:
        assert s.AddPending(c.PeerID(), H) is None and s.MovePendingToActive(c) is None
    assert sorted(s.ActiveConns(), key=id) == sorted(conns, key=id) and s.NumActiveConns() == 10
    for c in conns:
        s.DeleteActive(c)
    assert s.ActiveConns() == []


def test_max_mutual_conns():
    """TestMaxMutualConns: 10, 6 and 5 mutual neighbours under a limit of 5."""
    s = state(MaxMutualConnections=5, MaxOpenConnectionsPerTorrent=20)
    neighbors = [f"n{i}" for i in range(10)]
    for n in neighbors:
        assert s.AddPending(n, H) is None
    assert s.AddPending("a", H, neighbors) is CS.ErrTooManyMutualConns
    assert s.AddPending("b", H, neighbors[:6]) is CS.ErrTooManyMutualConns
    assert s.AddPending("c", H, neighbors[:5] + ["a stranger"]) is None


def test_rows_grow_past_a_word():
    s = state(MaxOpenConnectionsPerTorrent=200, MaxMutualConnections=1000)
    for i in range(130):
        assert s.AddPending(f"p{i}", H) is None
    assert s.torrents[H].rows.shape[1] >= 3 and s.AddPending("p129", H) is CS.ErrConnAlreadyPending
    assert s.AddPending("x", H, [f"p{i}" for i in range(130)]) is None


# ------------------------------------------------------------------ ConnRound
def seeded(clock, **config):
    """A State with pending, active and blacklisted conns over two torrents, and its conns."""
    config.setdefault("MaxOpenConnectionsPerTorrent", 80)
    s = state(clock, **config)
    conns = {}
    for h, n in (("h0", 9), ("h1", 70)):
        for i in range(n):
            assert s.AddPending(f"p{i}", h) is None
        for i in range(0, n, 2):
            c = conns[(h, i)] = CS.Conn(f"p{i}", h, createdAt=900 + i)
            assert s.MovePendingToActive(c) is None
    assert s.Blacklist("gone", "h0") is None
    return s, conns


def snapshot(s):
    return {h: (T.peers[:], T.packed().tolist(), T.expiry[:len(T.peers)].tolist(), T.capacity, sorted(T.conns))
            for h, T in s.torrents.items()}


def events(conns):
    other = CS.Conn("p4", "h0")  # shares p4's key, is not the active conn
    dead = CS.Conn("p3", "h0")
    dead.Close()
    return [("closed", conns[("h0", 0)]), ("closed", other), ("outgoing_failed", "h0", "p1"), ("incoming_failed", "h0", "p5"),
            ("established", CS.Conn("p7", "h0")), ("established", dead), ("established", CS.Conn("fresh", "h0")),
            ("closed", conns[("h1", 64)]), ("outgoing_failed", "h1", "p69"),
            ("incoming_handshake", "h0", "in-a", ["p2", "p6", "nobody"]), ("incoming_handshake", "h0", "in-b", ["p2", "in-a"]),
            ("incoming_handshake", "h0", "p2", None), ("incoming_handshake", "h1", "in-c", [f"p{i}" for i in range(70)]),
            ("announce_result", "h0", ["local-peer", "gone", "p0", "d1", "d1", "p1", "d2", "d3", "d4"], False),
            ("announce_result", "h1", [f"e{i}" for i in range(72)], False),
            ("announce_result", "h2", ["a", "b"], True)]


def one_at_a_time(s, evs):
    """The events applied to State's own methods, in phase order: what ConnRound must equal."""
    out = {}

    def res(h):
        if h not in out:
            out[h] = CS.TorrentResult()
        return out[h]

    def blacklist(h, p):
        before = s.Blacklisted(p, h)
        if s.Blacklist(p, h) is None and not before and not s.config.DisableBlacklist:
            res(h).blacklisted.append(p)

    order = {"h0": [], "h1": [], "h2": []}
    for e in evs:  # a torrent's transitions run in its peers' index order
        if e[0] in ("closed", "established"):
            order[e[1].InfoHash()].append((s.torrent(e[1].InfoHash()).peer(e[1].PeerID()), e))
        elif e[0] in ("outgoing_failed", "incoming_failed"):
            order[e[1]].append((s.torrent(e[1]).peer(e[2]), e))
    for h in order:
        for _, e in sorted(order[h], key=lambda x: x[0]):
            T = s.torrents[h]
            cap = T.capacity
            if e[0] == "closed":
                s.DeleteActive(e[1])
                blacklist(h, e[1].PeerID())
            elif e[0] == "established":
                err = s.MovePendingToActive(e[1])
                if err is None:
                    res(h).established.append(e[1])
                elif err is not CS.ErrConnClosed:
                    res(h).invalid.append((e[1], err))
            else:
                s.DeletePending(e[2], h)
                if e[0] == "outgoing_failed":
                    blacklist(h, e[2])
            res(h).freed += T.capacity - cap
    for e in evs:
        if e[0] == "established" and e[1].IsClosed():
            res(e[1].InfoHash()).invalid.insert(0, (e[1], CS.ErrConnClosed))
    for e in evs:
        if e[0] == "incoming_handshake":
            err = s.AddPending(e[2], e[1], e[3])
            (res(e[1]).admitted.append(e[2]) if err is None else res(e[1]).rejected.append((e[2], err)))
    status = {CS.ErrTorrentAtCapacity: D.CN_AT_CAPACITY, CS.ErrConnAlreadyPending: D.CN_ALREADY_PENDING,
              CS.ErrConnAlreadyActive: D.CN_ALREADY_ACTIVE}
    for e in evs:
        if e[0] != "announce_result":
            continue
        _, h, peers, complete = e
        for p in peers:
            s.torrent(h).peer(p)
            if complete:
                res(h).skipped.append((p, D.CN_TORRENT_IS_COMPLETE))
            elif p == s.localPeerID:
                res(h).skipped.append((p, D.CN_SELF))
            elif s.Blacklisted(p, h):
                res(h).skipped.append((p, D.CN_BLACKLISTED))
            else:
                err = s.AddPending(p, h)
                (res(h).dial.append(p) if err is None else res(h).skipped.append((p, status[err])))
    for h, r in out.items():
        r.capacity = s.torrents[h].capacity
    return out


def feed(rnd, evs):
    for e in evs:
        getattr(rnd, e[0])(*e[1:])
    return rnd.run()


@pytest.mark.parametrize("disable", [False, True])
def test_conn_round_equals_the_events_one_at_a_time(disable):
    a, conns_a = seeded(MockClock(1000), MaxOpenConnectionsPerTorrent=80, MaxMutualConnections=3, DisableBlacklist=disable)
    b, conns_b = seeded(MockClock(1000), MaxOpenConnectionsPerTorrent=80, MaxMutualConnections=3, DisableBlacklist=disable)
    assert snapshot(a) == snapshot(b)
    ev_a, ev_b = events(conns_a), events(conns_b)
    got = feed(CS.ConnRound(a, "host"), ev_a)
    want = one_at_a_time(b, ev_b)
    assert snapshot(a) == snapshot(b)
    assert sorted(got) == sorted(want) == ["h0", "h1", "h2"]
    for h in got:
        g, w = got[h], want[h]
        assert (g.dial, g.skipped, g.admitted, g.rejected, g.freed, g.blacklisted, g.capacity) == \
            (w.dial, w.skipped, w.admitted, w.rejected, w.freed, w.blacklisted, w.capacity), h
        assert [c.PeerID() for c in g.established] == [c.PeerID() for c in w.established], h
        assert [(c.PeerID(), e) for c, e in g.invalid] == [(c.PeerID(), e) for c, e in w.invalid], h
    # what the round is for: some of everything happened
    r0 = got["h0"]
    assert r0.dial and r0.admitted and r0.rejected and r0.freed and r0.established and r0.invalid
    assert bool(r0.blacklisted) != disable
    assert ("local-peer", D.CN_SELF) in r0.skipped and ("d1", D.CN_ALREADY_PENDING) in r0.skipped
    assert (("gone", D.CN_BLACKLISTED) in r0.skipped) != disable
    assert got["h2"].skipped == [("a", D.CN_TORRENT_IS_COMPLETE), ("b", D.CN_TORRENT_IS_COMPLETE)]
    assert got["h1"].skipped and got["h1"].skipped[-1][1] == D.CN_AT_CAPACITY and got["h1"].capacity == 0


def test_conn_round_refuses_a_second_transition_or_handout():
    s, conns = seeded(MockClock(1000))
    rnd = CS.ConnRound(s)
    rnd.outgoing_failed("h0", "p1")
    with pytest.raises(ValueError):
        rnd.incoming_failed("h0", "p1")
    rnd.announce_result("h0", ["x"])
    with pytest.raises(ValueError):
        rnd.announce_result("h0", ["y"])
    with pytest.raises(ValueError):
        CS.ConnRound(s, "tpu")
    assert CS.ConnRound(s).run() == {}


def test_preemption_sweep_host():
    clk = MockClock(1000)
    s, conns = seeded(clk)
    received = {("h1", "p2"): 950, ("h0", "p2"): 899}
    sent = {("h1", "p4"): 901}
    clk.Add(1)  # now 1001, tti 100: created 900 + i, so conns with i < 1 are idle unless they made progress
    got = CS.PreemptionSweep(s, 100, 10_000, lambda h, p: received.get((h, p), 0), lambda h, p: sent.get((h, p), 0))
    want = []
    for (h, i), c in sorted(conns.items()):
        last = max(c.CreatedAt(), received.get((h, c.PeerID()), 0), sent.get((h, c.PeerID()), 0))
        if 1001 - last > 100:
            want.append(c)
    assert got == want and [c.PeerID() for c in got] == ["p0", "p0"]
    clk.Add(20)
    got = CS.PreemptionSweep(s, 100, 95)  # the ttl: created more than 95 ago, whatever the progress
    assert sorted(c.CreatedAt() for c in got) == sorted(c.CreatedAt() for c in conns.values() if 1021 - c.CreatedAt() > 95)
    assert CS.PreemptionSweep(state(), 1, 1) == []


# ------------------------------------------------------------------ announce -> connect
def drive(placement):
    """Three announce intervals through peerstore.AnnounceRound; our agent ("peer-000") announces
    too, takes its handout to ConnRound.announce_result and establishes whoever it may dial."""
    clk = MockClock(0)
    store = PS.LocalStore(clk, 10, 5, seed=7)
    s = CS.State(CS.Config(MaxOpenConnectionsPerTorrent=12), clk, "peer-000")
    model = {h: R.Torrent(0, capacity=12) for h in ("hash-0", "hash-1")}  # the restatement, peers by identity
    dialled = {h: [] for h in model}
    for k in range(3):
        anns = [(f"digest-{j % 2}", f"hash-{j % 2}", PS.PeerInfo(f"peer-{1 + (j * 5 + k) % 96:03d}", "10.0.0.1", 8000))
                for j in range(120)]
        anns += [("digest-0", "hash-0", PS.PeerInfo("peer-000", "10.0.0.9", 9000)),
                 ("digest-1", "hash-1", PS.PeerInfo("peer-000", "10.0.0.9", 9000))]
        handouts, _ = PS.AnnounceRound(store, {}, anns, 50)
        rnd = CS.ConnRound(s, placement)
        ours = {}
        for (d, h, p), handout in zip(anns, handouts):
            if p.PeerID == "peer-000":
                ours[h] = [q.PeerID for q in handout] + ["peer-000"]  # the tracker may return our own peer
                rnd.announce_result(h, ours[h])
        got = rnd.run()
        for h, peers in ours.items():
            T = model[h]
            index = s.torrents[h].index  # the restatement works on indices: the order of first sight, as State's
            T.n_peers = len(index)
            T.self_peer = index["peer-000"]
            _, _, ds, _, n_dial, _ = R.conn_round(T, [], [], [index[p] for p in peers], clk.Now(), 30, 12, 0)
            assert got[h].dial == [p for p, st in zip(peers, ds) if st == R.OK] and len(got[h].dial) == n_dial
            dialled[h] += got[h].dial
        rnd = CS.ConnRound(s, placement)
        last = {h: got[h].dial for h in ours}
        for h in ours:
            for j, p in enumerate(last[h]):  # every other handshake fails
                if j % 2:
                    rnd.outgoing_failed(h, p)
                else:
                    rnd.established(CS.Conn(p, h, createdAt=clk.Now()))
        got = rnd.run()
        for h in ours:
            T, index = model[h], s.torrents[h].index
            trans = sorted((index[p], R.FAILED_OUT if j % 2 else R.ESTABLISHED) for j, p in enumerate(last[h]))
            R.conn_round(T, trans, [], [], clk.Now(), 30, 12, 0)
        clk.Add(10)
    return s, model, dialled


def test_announce_handouts_drive_the_connection_state():
    s, model, dialled = drive("host")
    for h, T in model.items():
        S = s.torrents[h]
        active = {i for i in range(len(S.peers)) if S.has(0, i)}
        pending = {i for i in range(len(S.peers)) if S.has(1, i)}
        assert active == T.active == set(S.conns) and pending == T.pending == set()
        assert S.capacity == T.capacity == 12 - len(active)
        assert {i: int(e) for i, e in enumerate(S.expiry[:len(S.peers)]) if e} == T.expiry
        assert active and T.expiry and "peer-000" not in dialled[h]
        assert len(set(dialled[h])) == len(dialled[h])  # nobody is dialled twice: active, pending or blacklisted
