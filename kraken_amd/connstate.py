"""Host-side mirror of the scheduler's connection bookkeeping, with every decision behind the C ABI.

``State`` keeps the reference's connstate.State (lib/torrent/scheduler/connstate/state.go) in
process memory as the bit rows ``krk_conn_round`` works on: a torrent's known peers in the order they
were first seen (identity -> index, the index space of the torrent's request rounds), an active and a
pending row, one blacklist expiry a peer and the remaining capacity.  Its methods keep the
reference's names and return its errors (``None`` for Go's nil); every single operation is a
one-entry round of the host call, so the class and the batch are the same code.

``ConnRound`` is the batched form the reference's event loop lacks: one instant's events --
announce results, incoming handshakes, failed handshakes, established and closed conns -- for every
torrent in one ``krk_conn_round`` call (placement "host") or one ``krk_conn_round_dev`` launch
(placement "gpu": one wave a torrent).  A round applies the frees first, then the incoming
handshakes, then the dials; the reference applies events in arrival order.  ``PreemptionSweep`` is
preemptionTickEvent's connection half (events.go:370-392) the same way.  Dialling, handshaking and
closing stay with the caller.
"""
from __future__ import annotations

import numpy as np

from . import device as D


class ConnError(Exception):
    """A connstate error; compare with the Err* constants."""


ErrTorrentAtCapacity = ConnError("torrent is at capacity")
ErrConnAlreadyPending = ConnError("conn is already pending")
ErrConnAlreadyActive = ConnError("conn is already active")
ErrConnClosed = ConnError("conn is closed")
ErrInvalidActiveTransition = ConnError("conn must be pending to transition to active")
ErrTooManyMutualConns = ConnError("conn has too many mutual connections")
ErrAlreadyBlacklisted = ConnError("conn is already blacklisted")  # errors.New at state.go:129

_ADD_PENDING_ERR = {D.CN_AT_CAPACITY: ErrTorrentAtCapacity, D.CN_ALREADY_PENDING: ErrConnAlreadyPending,
                    D.CN_ALREADY_ACTIVE: ErrConnAlreadyActive, D.CN_TOO_MANY_MUTUAL: ErrTooManyMutualConns}


class Config:
    """connstate.Config; durations in the clock's units (the default 30 is the reference's 30 s)."""

    def __init__(self, MaxOpenConnectionsPerTorrent=0, MaxMutualConnections=0, DisableBlacklist=False, BlacklistDuration=0):
        self.MaxOpenConnectionsPerTorrent, self.MaxMutualConnections = int(MaxOpenConnectionsPerTorrent), int(MaxMutualConnections)
        self.DisableBlacklist, self.BlacklistDuration = bool(DisableBlacklist), int(BlacklistDuration)

    def applyDefaults(self) -> "Config":
        c = Config(self.MaxOpenConnectionsPerTorrent or 10, self.MaxMutualConnections, self.DisableBlacklist,
                   self.BlacklistDuration or 30)
        if c.MaxMutualConnections == 0:  # defaults to no mutual connection limit
            c.MaxMutualConnections = c.MaxOpenConnectionsPerTorrent
        return c


class Conn:
    """What the bookkeeping reads of a conn.Conn: its peer, its torrent, when it was created and
    whether it is closed."""

    def __init__(self, peerID, infoHash, createdAt=0):
        self.peerID, self.infoHash, self.createdAt, self.closed = peerID, infoHash, int(createdAt), False

    def PeerID(self):
        return self.peerID

    def InfoHash(self):
        return self.infoHash

    def CreatedAt(self):
        return self.createdAt

    def IsClosed(self):
        return self.closed

    def Close(self):
        self.closed = True

    def __repr__(self):
        return f"Conn({self.peerID!r}, {self.infoHash!r})"


class BlacklistedConn:
    """connstate.BlacklistedConn."""

    def __init__(self, PeerID, InfoHash, Remaining):
        self.PeerID, self.InfoHash, self.Remaining = PeerID, InfoHash, Remaining

    def __eq__(self, o):
        return isinstance(o, BlacklistedConn) and (self.PeerID, self.InfoHash, self.Remaining) == (o.PeerID, o.InfoHash, o.Remaining)

    def __repr__(self):
        return f"BlacklistedConn({self.PeerID!r}, {self.InfoHash!r}, {self.Remaining})"


def _words(p: int) -> int:
    return (p + 63) // 64


class _Torrent:
    def __init__(self, capacity: int):
        self.index, self.peers = {}, []  # identity -> index, index -> identity
        self.rows = np.zeros((2, 1), dtype=np.uint64)  # active, pending
        self.expiry = np.zeros(64, dtype=np.int64)
        self.capacity = capacity
        self.conns = {}  # index -> the active Conn

    def peer(self, identity) -> int:
        i = self.index.get(identity)
        if i is None:
            i = self.index[identity] = len(self.peers)
            self.peers.append(identity)
            if _words(i + 1) > self.rows.shape[1]:
                grown = np.zeros((2, 2 * self.rows.shape[1]), dtype=np.uint64)
                grown[:, :self.rows.shape[1]] = self.rows
                self.rows = grown
                self.expiry = np.concatenate([self.expiry, np.zeros(self.expiry.size, dtype=np.int64)])
        return i

    def has(self, row: int, i: int) -> bool:
        return bool((int(self.rows[row, i >> 6]) >> (i & 63)) & 1)

    def packed(self) -> np.ndarray:
        return np.ascontiguousarray(self.rows[:, :_words(len(self.peers))]).reshape(-1)

    def unpack(self, words: np.ndarray):
        self.rows[:, :_words(len(self.peers))] = words.reshape(2, -1)

    def neighbor_row(self, neighbors):
        """The neighbours this torrent knows as a bit row, or None: a peer it has never seen is
        neither active nor pending."""
        known = [self.index[n] for n in neighbors or () if n in self.index]
        if not known:
            return None
        row = np.zeros(_words(len(self.peers)), dtype=np.uint64)
        for i in known:
            row[i >> 6] |= np.uint64(1 << (i & 63))
        return row


class State:
    """connstate.State over bit rows.  clock: anything with Now() in the unit of BlacklistDuration
    (piecerequest.MockClock serves).  Not thread-safe, as the reference's."""

    def __init__(self, config: Config | None, clock, localPeerID=None):
        self.config, self.clock, self.localPeerID = (config or Config()).applyDefaults(), clock, localPeerID
        self.torrents = {}

    def torrent(self, h) -> _Torrent:
        T = self.torrents.get(h)
        if T is None:
            T = self.torrents[h] = _Torrent(self.config.MaxOpenConnectionsPerTorrent)
        return T

    # ------------------------------------------------------------ one-entry rounds
    def _round(self, T: _Torrent, transitions=(), incoming=(), disable_blacklist=None):
        """One torrent's one-entry round on the host: the entry's status."""
        batch = D.ConnBatch([(len(T.peers), D.CN_NONE, 0)], [(transitions, incoming, ())])
        n = len(T.peers)
        bits, expiry, cap = T.packed(), T.expiry[:n].copy(), np.array([T.capacity], dtype=np.uint32)
        off = self.config.DisableBlacklist if disable_blacklist is None else disable_blacklist
        ts, ins, _, _, _ = D.conn_round(batch, bits, expiry, cap, int(self.clock.Now()), self.config.BlacklistDuration,
                                        self.config.MaxMutualConnections, D.CN_DISABLE_BLACKLIST if off else 0)
        T.unpack(bits)
        T.expiry[:n] = expiry
        T.capacity = int(cap[0])
        return int(ts[0]) if len(ts) else int(ins[0])

    def _blacklist_kind(self, T: _Torrent, i: int) -> int:
        """The transition that blacklists peer i and frees nothing: a failed outgoing handshake of
        a conn that is not pending, or a close of one that is not active."""
        return D.CN_FAILED_OUT if not T.has(1, i) else D.CN_CLOSED

    # ------------------------------------------------------------ the reference's methods
    def MaxConnsPerTorrent(self) -> int:
        return self.config.MaxOpenConnectionsPerTorrent

    def ActiveConns(self):
        return [c for T in self.torrents.values() for c in T.conns.values()]

    def NumActiveConns(self) -> int:
        return sum(len(T.conns) for T in self.torrents.values())

    def Blacklist(self, peerID, h):
        if self.config.DisableBlacklist:
            return None
        T = self.torrent(h)
        i = T.peer(peerID)
        st = self._round(T, transitions=[(i, self._blacklist_kind(T, i))])
        return ErrAlreadyBlacklisted if st & D.CN_STILL_BLACKLISTED else None

    def Blacklisted(self, peerID, h) -> bool:
        T = self.torrents.get(h)
        i = T.index.get(peerID) if T is not None else None
        return i is not None and int(T.expiry[i]) > int(self.clock.Now())

    def ClearBlacklist(self, h):
        T = self.torrents.get(h)
        if T is not None:
            T.expiry[:] = 0

    def BlacklistSnapshot(self):
        now = int(self.clock.Now())
        return [BlacklistedConn(T.peers[i], h, int(T.expiry[i]) - now)
                for h, T in self.torrents.items() for i in np.flatnonzero(T.expiry[:len(T.peers)]).tolist()]

    def AddPending(self, peerID, h, neighbors=None):
        T = self.torrent(h)
        i = T.peer(peerID)
        return _ADD_PENDING_ERR.get(self._round(T, incoming=[(i, T.neighbor_row(neighbors))]))

    def DeletePending(self, peerID, h):
        T = self.torrent(h)
        self._round(T, transitions=[(T.peer(peerID), D.CN_FAILED_IN)])

    def MovePendingToActive(self, c: Conn):
        if c.IsClosed():
            return ErrConnClosed
        T = self.torrent(c.InfoHash())
        i = T.peer(c.PeerID())
        if self._round(T, transitions=[(i, D.CN_ESTABLISHED)]) & D.CN_NOT_PENDING:
            return ErrInvalidActiveTransition
        T.conns[i] = c
        return None

    def DeleteActive(self, c: Conn):
        T = self.torrent(c.InfoHash())
        i = T.peer(c.PeerID())
        if T.conns.get(i) is not c:  # some new conn may share the key: delete the right one only
            return
        self._round(T, transitions=[(i, D.CN_CLOSED)], disable_blacklist=True)  # DeleteActive alone blacklists nobody
        del T.conns[i]


class TorrentResult:
    """What a round did to one torrent.  dial: the peers to open outgoing handshakes to, in handout
    order; skipped: [(peer, status)] of the handout's other entries; admitted: the incoming
    handshakes to establish; rejected: [(peer, error)]; established: the conns now active;
    invalid: [(conn, error)] of those that were not pending or closed; freed: the capacity given
    back; blacklisted: the peers blacklisted by this round; capacity: what remains."""

    def __init__(self):
        self.dial, self.skipped, self.admitted, self.rejected = [], [], [], []
        self.established, self.invalid, self.blacklisted = [], [], []
        self.freed, self.capacity = 0, 0

    def __eq__(self, o):
        return isinstance(o, TorrentResult) and self.__dict__ == o.__dict__

    def __repr__(self):
        return f"TorrentResult({self.__dict__})"


class ConnRound:
    """One instant's events for every torrent, applied by run() in one call."""

    def __init__(self, state: State, placement: str = "host"):
        if placement not in ("host", "gpu"):
            raise ValueError(f"ConnRound: placement {placement!r} is neither \"host\" nor \"gpu\"")
        self.state, self.placement = state, placement
        self.events = {}  # h -> {"trans": {index: (kind, conn)}, "in": [(index, neighbors)], "dial": [index] or None, ...}

    def _of(self, h):
        e = self.events.get(h)
        if e is None:
            e = self.events[h] = {"T": self.state.torrent(h), "trans": {}, "in": [], "dial": None, "complete": False,
                                  "closed": []}
        return e

    def _transition(self, h, peerID, kind, conn=None):
        e = self._of(h)
        i = e["T"].peer(peerID)
        if i in e["trans"]:
            raise ValueError(f"ConnRound: a second transition of {peerID!r} in one round")
        e["trans"][i] = (kind, conn)

    def announce_result(self, h, peers, complete: bool = False):
        """announceResultEvent: one handout a torrent a round; peers: identities in handout order."""
        e = self._of(h)
        if e["dial"] is not None:
            raise ValueError(f"ConnRound: a second announce result for {h!r} in one round")
        e["dial"], e["complete"] = [e["T"].peer(p) for p in peers], bool(complete)

    def incoming_handshake(self, h, peerID, neighbors=None):
        e = self._of(h)
        e["in"].append((e["T"].peer(peerID), list(neighbors or ())))

    def incoming_failed(self, h, peerID):
        self._transition(h, peerID, D.CN_FAILED_IN)

    def outgoing_failed(self, h, peerID):
        self._transition(h, peerID, D.CN_FAILED_OUT)

    def established(self, c: Conn):
        if c.IsClosed():  # a closed conn is the caller's to filter: it never enters the list
            self._of(c.InfoHash())["closed"].append(c)
            return
        self._transition(c.InfoHash(), c.PeerID(), D.CN_ESTABLISHED, c)

    def closed(self, c: Conn):
        e = self._of(c.InfoHash())
        T = e["T"]
        i = T.peer(c.PeerID())
        # DeleteActive deletes only the very conn; Blacklist follows in both cases
        self._transition(c.InfoHash(), c.PeerID(), D.CN_CLOSED if T.conns.get(i) is c else self.state._blacklist_kind(T, i), c)

    def run(self):
        """{infohash: TorrentResult} of every torrent that had an event."""
        S = self.state
        hs = list(self.events)
        if not hs:
            return {}
        me, torrents, lists = S.localPeerID, [], []
        for h in hs:
            e = self.events[h]
            T = e["T"]
            torrents.append((len(T.peers), T.index.get(me, D.CN_NONE), D.CN_TORRENT_COMPLETE if e["complete"] else 0))
            lists.append(([(i, k) for i, (k, _) in sorted(e["trans"].items())],
                          [(i, T.neighbor_row(nbs)) for i, nbs in e["in"]], e["dial"] or []))
        batch = D.ConnBatch(torrents, lists)
        bits = np.concatenate([e["T"].packed() for e in self.events.values()] + [np.zeros(0, dtype=np.uint64)])
        expiry = np.concatenate([e["T"].expiry[:len(e["T"].peers)] for e in self.events.values()] + [np.zeros(0, dtype=np.int64)])
        cap = np.array([e["T"].capacity for e in self.events.values()], dtype=np.uint32)
        now, cfg = int(S.clock.Now()), S.config
        flags = D.CN_DISABLE_BLACKLIST if cfg.DisableBlacklist else 0
        if self.placement == "host":
            out = D.conn_round(batch, bits, expiry, cap, now, cfg.BlacklistDuration, cfg.MaxMutualConnections, flags)
        else:
            dev = []
            for a in (bits, expiry, cap):
                b = D.DeviceBuffer(a.nbytes)
                b.from_host(a)
                dev.append(b)
            out = D.conn_round_dev(batch, *dev, None, now, cfg.BlacklistDuration, cfg.MaxMutualConnections, flags)
            bits, expiry, cap = (b.to_host(a.dtype, a.size) for b, a in zip(dev, (bits, expiry, cap)))
        ts, ins, ds, n_adm, n_freed = out
        results = {}
        for t, h in enumerate(hs):
            e = self.events[h]
            T = e["T"]
            T.unpack(bits[int(batch.bits_off[t]):int(batch.bits_off[t + 1])])
            T.expiry[:len(T.peers)] = expiry[int(batch.peer_off[t]):int(batch.peer_off[t + 1])]
            T.capacity = int(cap[t])
            r = results[h] = TorrentResult()
            r.freed, r.capacity = int(n_freed[t]), T.capacity
            r.invalid = [(c, ErrConnClosed) for c in e["closed"]]
            for (i, (kind, c)), st in zip(sorted(e["trans"].items()), batch.split(ts, t, 0).tolist()):
                if kind == D.CN_ESTABLISHED:
                    if st & D.CN_OK:
                        T.conns[i] = c
                        r.established.append(c)
                    else:
                        r.invalid.append((c, ErrInvalidActiveTransition))
                elif kind == D.CN_CLOSED and st & D.CN_FREED:
                    del T.conns[i]
                if st & D.CN_BLACKLISTED_NOW:
                    r.blacklisted.append(T.peers[i])
            for (i, _), st in zip(e["in"], batch.split(ins, t, 1).tolist()):
                if st == D.CN_OK:
                    r.admitted.append(T.peers[i])
                else:
                    r.rejected.append((T.peers[i], _ADD_PENDING_ERR[st]))
            for i, st in zip(e["dial"] or [], batch.split(ds, t, 2).tolist()):
                if st == D.CN_OK:
                    r.dial.append(T.peers[i])
                else:
                    r.skipped.append((T.peers[i], st))
            assert (len(r.admitted), len(r.dial)) == tuple(int(x) for x in n_adm[t])
        self.events = {}
        return results


def PreemptionSweep(state: State, ConnTTI: int, ConnTTL: int, last_good_piece_received=None, last_piece_sent=None,
                    placement: str = "host"):
    """preemptionTickEvent's connection half for every active conn in one call: the conns to close
    (idle longer than ConnTTI or older than ConnTTL).  last_good_piece_received / last_piece_sent:
    callables (infohash, peerID) -> time, 0 for never (the dispatcher's); None: never."""
    if placement not in ("host", "gpu"):
        raise ValueError(f"PreemptionSweep: placement {placement!r} is neither \"host\" nor \"gpu\"")
    hs = [h for h, T in state.torrents.items() if T.conns]
    if not hs:
        return []
    tors = [state.torrents[h] for h in hs]
    batch = D.ConnBatch([(len(T.peers), D.CN_NONE, 0) for T in tors])
    bits = np.concatenate([T.packed() for T in tors])
    times = np.zeros((3, batch.total_peers), dtype=np.int64)
    for t, (h, T) in enumerate(zip(hs, tors)):
        base = int(batch.peer_off[t])
        for i, c in T.conns.items():
            times[0, base + i] = c.CreatedAt()
            times[1, base + i] = last_good_piece_received(h, c.PeerID()) if last_good_piece_received else 0
            times[2, base + i] = last_piece_sent(h, c.PeerID()) if last_piece_sent else 0
    now = int(state.clock.Now())
    if placement == "host":
        close, _ = D.conn_preempt(batch, bits, times[0], times[1], times[2], now, ConnTTI, ConnTTL)
    else:
        dev = []
        for a in (bits, times[0], times[1], times[2]):
            b = D.DeviceBuffer(a.nbytes)
            b.from_host(np.ascontiguousarray(a))
            dev.append(b)
        close, _ = D.conn_preempt_dev(batch, *dev, now, ConnTTI, ConnTTL)
    out = []
    for t, T in enumerate(tors):
        row = close[int(batch.close_off[t]):int(batch.close_off[t + 1])]
        out += [c for i, c in sorted(T.conns.items()) if (int(row[i >> 6]) >> (i & 63)) & 1]
    return out
