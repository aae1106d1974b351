"""Host-side mirror of the tracker's announce path, with the handout behind the C ABI.

``LocalStore`` keeps the reference's peer store (tracker/peerstore/redis.go) in process memory as
the bit matrix ``krk_announce_round`` works on: a torrent's known peers in the order they first
announced (identity -> index), and a ring of ``MaxPeerSetWindows`` peer-set windows of
``PeerSetWindowSize`` clock units, (member, complete) a window.  Where Redis expires a window's key
(``EXPIREAT``, redis.go:131-141), advancing the clock zeroes the ring row that becomes current and
moves ``cur_row``: a peer that has not announced for ``MaxPeerSetWindows`` windows is gone.
``UpdatePeer`` and ``GetPeers`` keep the reference's names; ``GetPeers`` is ``krk_announce_handout``
with no origins and no source, its SRANDMEMBER draws seeded from the store's seed.

``PriorityPolicy.SortPeers`` (tracker/peerhandoutpolicy/peerhandoutpolicy.go:65-99) orders a list
of PeerInfos through the same entry point.  The source is dropped by identity -- the reference
compares pointers, which never match what its store returns.

``AnnounceRound`` is the batched form the reference lacks: ``Server.announce``
(tracker/trackerserver/announce.go:75-115) for every announce of an interval at one clock instant,
in one ``krk_announce_round`` call (placement "host") or one ``krk_announce_round_dev`` call
(placement "gpu": one wave an announce).  HTTP and the origin cluster stay with the caller.
"""
from __future__ import annotations

import numpy as np

from . import device as D
from .piecerequest import splitmix64

DefaultPolicy = "default"
CompletenessPolicy = "completeness"
_POLICY = {DefaultPolicy: D.AN_DEFAULT, CompletenessPolicy: D.AN_COMPLETENESS}
_LABELS = {DefaultPolicy: ("default",), CompletenessPolicy: ("peer_seeder", "origin", "peer_incomplete")}


class PeerInfo:
    """core.PeerInfo."""

    def __init__(self, PeerID, IP="", Port=0, Origin=False, Complete=False):
        self.PeerID, self.IP, self.Port, self.Origin, self.Complete = PeerID, IP, Port, bool(Origin), bool(Complete)

    def identity(self):
        return (self.PeerID, self.IP, self.Port)

    def __eq__(self, o):
        return isinstance(o, PeerInfo) and (self.identity(), self.Origin, self.Complete) == (o.identity(), o.Origin, o.Complete)

    def __hash__(self):
        return hash(self.identity())

    def __repr__(self):
        return f"PeerInfo({self.PeerID!r}, {self.IP!r}, {self.Port}, Origin={self.Origin}, Complete={self.Complete})"


def _words(p: int) -> int:
    return (p + 63) // 64


class _Torrent:
    def __init__(self, n_windows: int, window: int):
        self.index, self.peers = {}, []  # identity -> index, index -> identity
        self.rows = np.zeros((2 * n_windows, 1), dtype=np.uint64)  # ring row r: rows[2r] member, rows[2r + 1] complete
        self.cur_row, self.window = 0, window

    def peer(self, identity) -> int:
        i = self.index.get(identity)
        if i is None:
            i = self.index[identity] = len(self.peers)
            self.peers.append(identity)
            if _words(i + 1) > self.rows.shape[1]:
                grown = np.zeros((self.rows.shape[0], 2 * self.rows.shape[1]), dtype=np.uint64)
                grown[:, :self.rows.shape[1]] = self.rows
                self.rows = grown
        return i

    def packed(self) -> np.ndarray:
        return np.ascontiguousarray(self.rows[:, :_words(len(self.peers))]).reshape(-1)

    def unpack(self, words: np.ndarray):
        self.rows[:, :_words(len(self.peers))] = words.reshape(self.rows.shape[0], -1)


class LocalStore:
    """peerstore.Store over bit matrices.  clock: anything with Now() in the unit of
    PeerSetWindowSize (piecerequest.MockClock serves)."""

    def __init__(self, clock, PeerSetWindowSize: int, MaxPeerSetWindows: int, seed: int = 0):
        if PeerSetWindowSize <= 0 or not 1 <= MaxPeerSetWindows <= D.AN_MAX_WINDOWS:
            raise ValueError(f"LocalStore: window size {PeerSetWindowSize}, {MaxPeerSetWindows} windows "
                             f"(1 .. {D.AN_MAX_WINDOWS})")
        self.clock, self.size, self.W, self.seed = clock, int(PeerSetWindowSize), int(MaxPeerSetWindows), int(seed)
        self.torrents, self._draws = {}, 0

    def curPeerSetWindow(self) -> int:
        t = int(self.clock.Now())
        return t - t % self.size

    def next_seed(self) -> int:
        self._draws += 1
        return splitmix64(self.seed ^ self._draws)

    def torrent(self, h, create: bool = False):
        """The torrent's store with its windows moved to the clock, or None."""
        T = self.torrents.get(h)
        if T is None:
            if not create:
                return None
            T = self.torrents[h] = _Torrent(self.W, self.curPeerSetWindow())
        steps = (self.curPeerSetWindow() - T.window) // self.size
        for _ in range(min(max(steps, 0), self.W)):  # the oldest window's row becomes the current one, empty
            T.cur_row = (T.cur_row - 1) % self.W
            T.rows[2 * T.cur_row:2 * T.cur_row + 2] = 0
        T.window += max(steps, 0) * self.size
        return T

    def UpdatePeer(self, h, p: PeerInfo):
        T = self.torrent(h, create=True)
        i = T.peer(p.identity())
        T.rows[2 * T.cur_row, i >> 6] |= np.uint64(1 << (i & 63))
        if p.Complete:
            T.rows[2 * T.cur_row + 1, i >> 6] |= np.uint64(1 << (i & 63))

    def GetPeers(self, h, n: int):
        """At most n PeerInfos of h: up to n sampled from each window in shuffled order until n
        distinct ones are collected, complete bits collapsed (redis.go:155-196)."""
        if not 1 <= n <= D.AN_MAX_LIMIT:
            raise ValueError(f"GetPeers: n = {n} is outside [1, {D.AN_MAX_LIMIT}]")
        T = self.torrent(h)
        if T is None or not T.peers:
            return []
        batch = D.AnnounceBatch([(len(T.peers), self.W, T.cur_row, 0)], [(0, 0, 0, D.AN_NONE, self.next_seed())])
        handout, k, _ = D.announce_handout(batch, T.packed(), 0, n, D.AN_DEFAULT)
        return [_peer_info(T, int(c), ()) for c in handout[:k]]


def _peer_info(T: _Torrent, c: int, origins) -> PeerInfo:
    if c & D.AN_ORIGIN:
        return origins[c & ~D.AN_ORIGIN]
    return PeerInfo(*T.peers[c & ~D.AN_COMPLETE_BIT], Origin=False, Complete=bool(c & D.AN_COMPLETE_BIT))


class PriorityPolicy:
    """peerhandoutpolicy.PriorityPolicy; .counts holds the last call's gauges by label."""

    def __init__(self, policy: str, seed: int = 0):
        if policy not in _POLICY:
            raise ValueError(f"priority policy {policy!r} not found")
        self.policy, self.seed, self.counts = policy, int(seed), {}

    def SortPeers(self, source: PeerInfo, peers):
        """The peers but the source, ordered by the policy's priority: at most AN_MAX_LIMIT peers and
        AN_MAX_ORIGINS origins."""
        peers = [p for p in peers if source is None or p.identity() != source.identity()]
        plain, origins = [p for p in peers if not p.Origin], [p for p in peers if p.Origin]
        if len(plain) > D.AN_MAX_LIMIT or len(origins) > D.AN_MAX_ORIGINS:
            raise ValueError(f"SortPeers: {len(plain)} peers and {len(origins)} origins (at most {D.AN_MAX_LIMIT} and "
                             f"{D.AN_MAX_ORIGINS})")
        n = max(len(plain), 1)
        batch = D.AnnounceBatch([(n + 1, 1, 0, len(origins))], [(0, n, 0, D.AN_NONE, self.seed)])  # peer n: nobody
        rows = np.zeros((2, _words(n + 1)), dtype=np.uint64)
        for i, p in enumerate(plain):
            rows[0, i >> 6] |= np.uint64(1 << (i & 63))
            if p.Complete:
                rows[1, i >> 6] |= np.uint64(1 << (i & 63))
        handout, k, counts = D.announce_handout(batch, rows.reshape(-1), 0, D.AN_MAX_LIMIT, _POLICY[self.policy])
        self.counts = {label: int(c) for label, c in zip(_LABELS[self.policy], counts) if c}
        return [origins[c & ~D.AN_ORIGIN] if c & D.AN_ORIGIN else plain[c & ~D.AN_COMPLETE_BIT] for c in map(int, handout[:k])]


def AnnounceRound(store: LocalStore, origins_by_digest, announces, limit: int, policy: str = DefaultPolicy,
                  placement: str = "host"):
    """Server.announce for every (digest, infohash, PeerInfo) of `announces` at one clock instant, in
    one call: every announcer written into the current window of its torrent, then every handout
    sampled from the updated windows, the digest's origins appended, the announcer left out and the
    rest ordered by `policy`.  Returns ([PeerInfo list an announce], label counts (A, 3)).
    placement "host": krk_announce_round; "gpu": krk_announce_round_dev (an error without a
    device)."""
    if placement not in ("host", "gpu"):
        raise ValueError(f"AnnounceRound: placement {placement!r} is neither \"host\" nor \"gpu\"")
    if policy not in _POLICY:
        raise ValueError(f"priority policy {policy!r} not found")
    order, origins, anns = {}, [], []  # infohash -> torrent index of the batch
    for d, h, p in announces:
        T = store.torrent(h, create=True)
        if h not in order:
            order[h] = len(order)
            origins.append(list(origins_by_digest.get(d, ())))
        i = T.peer(p.identity())
        anns.append((order[h], i, D.AN_COMPLETE if p.Complete else 0, i, store.next_seed()))
    if not anns:
        return [], np.zeros((0, 3), dtype=np.uint32)
    tors = [store.torrents[h] for h in order]
    batch = D.AnnounceBatch([(len(T.peers), store.W, T.cur_row, len(o)) for T, o in zip(tors, origins)], anns)
    bits = np.concatenate([T.packed() for T in tors])
    if placement == "host":
        handout, n_out, labels = D.announce_round(batch, bits, limit, _POLICY[policy])
    else:
        bits_dev = D.DeviceBuffer(bits.nbytes)
        bits_dev.from_host(bits)
        handout, n_out, labels = D.announce_round_dev(batch, bits_dev, limit, _POLICY[policy])
        bits = bits_dev.to_host(np.uint64, bits.size)
    for t, T in enumerate(tors):
        T.unpack(bits[int(batch.bits_off[t]):int(batch.bits_off[t + 1])])
    return [[_peer_info(tors[a[0]], int(c), origins[a[0]]) for c in handout[k, :int(n_out[k])]]
            for k, a in enumerate(anns)], labels
