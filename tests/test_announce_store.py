"""kraken_amd/peerstore.py on the host: LocalStore's peer-set windows (rotation, expiry after
MaxPeerSetWindows windows, complete bits collapsing across windows, GetPeers' bound),
PriorityPolicy.SortPeers with the reference's unit cases, and AnnounceRound through
krk_announce_round.  No device."""
import pytest

from kraken_amd import peerstore as PS
from kraken_amd.piecerequest import MockClock

H = "infohash-a"


def peer(k, complete=False, origin=False):
    return PS.PeerInfo(f"peer-{k:03d}", f"10.0.0.{k}", 8000 + k, Origin=origin, Complete=complete)


def ids(peers):
    return sorted(p.PeerID for p in peers)


def test_update_then_get():
    s = PS.LocalStore(MockClock(1000), 10, 5, seed=1)
    assert s.GetPeers(H, 50) == []
    for k in range(7):
        s.UpdatePeer(H, peer(k, complete=k == 3))
    got = s.GetPeers(H, 50)
    assert ids(got) == ids(peer(k) for k in range(7))
    assert [p.PeerID for p in got if p.Complete] == ["peer-003"] and not any(p.Origin for p in got)
    assert s.GetPeers("another", 50) == []


def test_get_peers_never_returns_more_than_n():
    clk = MockClock(0)
    s = PS.LocalStore(clk, 10, 3, seed=2)
    for w in range(3):
        for k in range(100 * w, 100 * w + 100):
            s.UpdatePeer(H, peer(k % 256))
        clk.Add(10)
    for n in (1, 2, 50, 64):
        for _ in range(5):  # every call draws afresh
            got = s.GetPeers(H, n)
            assert 0 < len(got) <= n and len(set(ids(got))) == len(got)
    assert len({p.PeerID for _ in range(20) for p in s.GetPeers(H, 1)}) > 1  # a seeded draw a call
    with pytest.raises(ValueError):
        s.GetPeers(H, 65)
    with pytest.raises(ValueError):
        s.GetPeers(H, 0)


def test_windows_rotate_and_expire_after_max_windows():
    clk = MockClock(50)
    s = PS.LocalStore(clk, 10, 3, seed=3)
    s.UpdatePeer(H, peer(1))
    clk.Add(10)
    s.UpdatePeer(H, peer(2))
    T = s.torrent(H)
    assert T.cur_row == 2 and s.curPeerSetWindow() == 60
    clk.Add(10)
    assert ids(s.GetPeers(H, 50)) == ["peer-001", "peer-002"]  # windows 70, 60, 50 are live
    clk.Add(9)
    assert ids(s.GetPeers(H, 50)) == ["peer-001", "peer-002"]  # still window 70
    clk.Add(1)
    assert ids(s.GetPeers(H, 50)) == ["peer-002"]  # window 50 has expired
    s.UpdatePeer(H, peer(1, complete=True))  # ... and its row, zeroed, is the current one
    assert ids(s.GetPeers(H, 50)) == ["peer-001", "peer-002"]
    clk.Add(10)
    assert ids(s.GetPeers(H, 50)) == ["peer-001"]
    clk.Add(1000)  # more than the ring in one step: every row zeroed, none twice
    assert s.GetPeers(H, 50) == [] and not s.torrent(H).rows.any()
    s.UpdatePeer(H, peer(2))
    assert ids(s.GetPeers(H, 50)) == ["peer-002"] and s.torrent(H).index[peer(1).identity()] == 0


def test_complete_bits_collapse_across_windows():
    clk = MockClock(0)
    s = PS.LocalStore(clk, 10, 5, seed=4)
    s.UpdatePeer(H, peer(1))
    s.UpdatePeer(H, peer(2))
    clk.Add(10)
    s.UpdatePeer(H, peer(1, complete=True))  # incomplete in the older window, complete in the newer
    clk.Add(10)
    s.UpdatePeer(H, peer(3))
    for _ in range(8):  # whatever order the windows are visited in
        got = {p.PeerID: p.Complete for p in s.GetPeers(H, 50)}
        assert got == {"peer-001": True, "peer-002": False, "peer-003": False}


def test_the_store_grows_past_a_word_of_peers():
    s = PS.LocalStore(MockClock(0), 10, 2, seed=5)
    for k in range(200):
        s.UpdatePeer(H, peer(k % 250, complete=k % 3 == 0))
    T = s.torrent(H)
    assert len(T.peers) == 200 and T.rows.shape == (4, 4)
    got = s.GetPeers(H, 64)
    assert len(got) == 64 and all(p.Complete == (int(p.PeerID[-3:]) % 3 == 0) for p in got)


def test_sort_peers_removes_the_source():
    """TestPriorityPolicyRemoveSource."""
    policy = PS.PriorityPolicy(PS.DefaultPolicy)
    src = peer(99)
    peers = [peer(k) for k in range(10)] + [src]
    got = policy.SortPeers(src, peers)
    assert len(got) == len(peers) - 1 and src not in got and ids(got) == ids(peers[:-1])
    assert policy.counts == {"default": 10}
    assert ids(policy.SortPeers(peer(99), peers)) == ids(peers[:-1])  # by identity, not by object


def test_sort_peers_by_completeness():
    """TestCompletenessPriorityPolicy: 10 seeders, 3 origins, 20 incomplete peers, shuffled."""
    policy = PS.PriorityPolicy(PS.CompletenessPolicy, seed=7)
    peers = [peer(k, complete=True) for k in range(10)] + [peer(k, complete=True, origin=True) for k in range(10, 13)] + \
        [peer(k) for k in range(13, 33)]
    shuffled = peers[::3] + peers[1::3] + peers[2::3]
    got = policy.SortPeers(peer(200), shuffled)
    assert len(got) == 33 and ids(got) == ids(peers)
    assert all(p.Complete and not p.Origin for p in got[:10])
    assert all(p.Complete and p.Origin for p in got[10:13])
    assert all(not p.Complete and not p.Origin for p in got[13:])
    assert policy.counts == {"peer_seeder": 10, "origin": 3, "peer_incomplete": 20}
    assert PS.PriorityPolicy(PS.CompletenessPolicy).SortPeers(None, []) == []
    with pytest.raises(ValueError):
        PS.PriorityPolicy("nearest")


def announces(n, n_torrents=3):
    return [(f"digest-{k % n_torrents}", f"hash-{k % n_torrents}", peer(k % 40, complete=k % 5 == 0)) for k in range(n)]


def test_announce_round_on_the_host():
    origins = {"digest-0": [peer(240 + k, complete=True, origin=True) for k in range(3)], "digest-2": []}
    clk = MockClock(0)
    s = PS.LocalStore(clk, 10, 5, seed=6)
    handouts, labels = PS.AnnounceRound(s, origins, announces(60), 50, PS.CompletenessPolicy)
    assert len(handouts) == 60 and labels.shape == (60, 3)
    for (d, h, p), got, lab in zip(announces(60), handouts, labels):
        if p.Complete:
            assert got == [] and lab.tolist() == [0, 0, 0]
            continue
        assert p.identity() not in [g.identity() for g in got]
        assert ids(g for g in got if g.Origin) == ids(origins.get(d, []))
        # every announcer of the round is in the window already
        want = {q.identity() for dd, hh, q in announces(60) if hh == h} - {p.identity()}
        assert {g.identity() for g in got if not g.Origin} == want
        prio = [1 if g.Origin else 0 if g.Complete else 2 for g in got]
        assert prio == sorted(prio) and lab.tolist() == [prio.count(k) for k in range(3)]
    # the store was updated: a later GetPeers sees the round's announcers
    assert len(s.GetPeers("hash-1", 64)) == len({p.identity() for d, h, p in announces(60) if h == "hash-1"})
    assert PS.AnnounceRound(s, origins, [], 50)[0] == []
    with pytest.raises(ValueError):
        PS.AnnounceRound(s, origins, announces(3), 50, placement="tpu")
