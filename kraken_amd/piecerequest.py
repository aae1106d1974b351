"""Host-side mirror of the agent's piece request bookkeeping, with the selection behind the C ABI.

``Manager`` follows lib/torrent/scheduler/dispatch/piecerequest/manager.go: the request table
(``requests`` by piece, ``requestsByPeer``), the statuses, the expiry rule (a pending request is
expired once the clock is AFTER sentAt + timeout), ``requestQuota`` and ``validRequest``.  What it
does not do itself is choose: ``ReservePieces`` hands ``validRequest`` over as a bitset (`blocked`)
and lets ``krk_piece_select`` pick -- rarest first (rarest_first_policy.go:38-44; ties go to the
lower piece index where the reference's heap leaves them to its sift order) or the default policy's
uniform sample (default_policy.go:33-66), drawn from a seed instead of Go's global math/rand.

``ReserveRound`` is the batched form the reference lacks: ``Dispatcher.maybeRequestMorePieces``
(dispatch/dispatcher.go:374-399) runs ReservePieces for one peer after every piece that arrives;
a round runs it for every peer of every torrent at one clock instant, in one
``krk_piece_request_round`` call (placement "host") or one ``krk_piece_request_round_dev`` call
(placement "gpu": one workgroup a torrent), and records the picks as pending.

``ResendRound`` is ``Dispatcher.resendFailedPieceRequests`` (dispatch/dispatcher.go:401-434) batched
the same way: every expired, unsent and invalid request of every torrent placed on the first peer
that holds the piece, has quota left and may be asked (``krk_piece_resend_round`` /
``krk_piece_resend_round_dev``, over the rows a reserve round uses), and recorded as pending there.
Connections and the wire protocol stay with the caller.
"""
from __future__ import annotations

import numpy as np

from . import device as D

DefaultPolicy = "default"
RarestFirstPolicy = "rarest_first"

StatusPending, StatusExpired, StatusUnsent, StatusInvalid = range(4)

_MASK64 = (1 << 64) - 1


def splitmix64(x: int) -> int:
    z = (x + 0x9E3779B97F4A7C15) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def bitset_words(bools) -> np.ndarray:
    """A willf/bitset of len(bools) bits as uint64 words (piece i = bit i & 63 of word i >> 6)."""
    b = np.packbits(np.asarray(bools, dtype=bool), bitorder="little")
    return np.concatenate([b, np.zeros(-b.size % 8, dtype=np.uint8)]).view(np.uint64)


class MockClock:
    """clock.NewMock(): stands still until Add."""

    def __init__(self, now=0):
        self.now = now

    def Now(self):
        return self.now

    def Add(self, d):
        self.now += d


class Request:
    """piecerequest.Request."""

    def __init__(self, Piece: int, PeerID, Status: int, sentAt=None):
        self.Piece, self.PeerID, self.Status, self.sentAt = Piece, PeerID, Status, sentAt

    def __eq__(self, o):
        return (self.Piece, self.PeerID, self.Status) == (o.Piece, o.PeerID, o.Status)

    def __repr__(self):
        return f"Request(Piece={self.Piece}, PeerID={self.PeerID!r}, Status={self.Status})"


class Manager:
    """piecerequest.Manager: piece request bookkeeping.  It sends and receives nothing."""

    def __init__(self, clock, timeout, policy: str, pipelineLimit: int, seed: int = 0):
        if policy == DefaultPolicy:
            self.policy = D.PR_SAMPLE
        elif policy == RarestFirstPolicy:
            self.policy = D.PR_RAREST_FIRST
        else:
            raise ValueError(f"invalid piece selection policy: {policy}")
        if not 1 <= pipelineLimit <= D.PR_MAX_LIMIT:
            raise ValueError(f"pipeline limit {pipelineLimit} outside [1, {D.PR_MAX_LIMIT}]")
        self.requests: dict[int, list[Request]] = {}
        self.requestsByPeer: dict[object, dict[int, Request]] = {}
        self.clock, self.timeout, self.pipelineLimit = clock, timeout, pipelineLimit
        self._seed, self._draws = seed, 0

    # -- the reference's private helpers
    def expired(self, r: Request) -> bool:
        return self.clock.Now() > r.sentAt + self.timeout

    def _live(self, r: Request) -> bool:
        return r.Status == StatusPending and not self.expired(r)

    def requestQuota(self, peerID) -> int:
        quota = self.pipelineLimit
        for r in self.requestsByPeer.get(peerID, {}).values():
            if self._live(r):
                quota -= 1
                if quota == 0:
                    break
        return quota

    def validRequest(self, peerID, i: int, allowDuplicates: bool) -> bool:
        return not any(self._live(r) and (r.PeerID == peerID or not allowDuplicates) for r in self.requests.get(i, ()))

    def blocked(self, peerID, n_pieces: int, allowDuplicates: bool) -> np.ndarray:
        """validRequest's complement over the pieces as a bitset: the pieces with a pending,
        unexpired request to peerID itself or, without allowDuplicates, to any peer."""
        b = np.zeros(n_pieces, dtype=bool)
        for i in self.requests:
            if i < n_pieces and not self.validRequest(peerID, i, allowDuplicates):
                b[i] = True
        return bitset_words(b)

    def next_seed(self) -> int:
        """The seed of the next sampled selection: splitmix64 of the manager's seed plus the draws so far."""
        s = splitmix64((self._seed + self._draws) & _MASK64)
        self._draws += 1
        return s

    def record(self, peerID, pieces):
        """Set as pending in the request maps (ReservePieces' tail)."""
        now = self.clock.Now()
        for i in pieces:
            r = Request(int(i), peerID, StatusPending, now)
            self.requests.setdefault(int(i), []).append(r)
            self.requestsByPeer.setdefault(peerID, {})[int(i)] = r

    # -- the reference's surface
    def ReservePieces(self, peerID, candidates, numPeersByPiece, allowDuplicates: bool) -> list[int]:
        """The next piece(s) to request from peerID.  candidates: one bool a piece;
        numPeersByPiece: one count a piece (read under the rarest-first policy)."""
        quota = self.requestQuota(peerID)
        if quota <= 0:
            return []
        cand = np.asarray(candidates, dtype=bool)
        n = cand.size
        counts = np.asarray(numPeersByPiece, dtype=np.uint32)[:n] if self.policy == D.PR_RAREST_FIRST else None
        seed = self.next_seed() if self.policy == D.PR_SAMPLE else 0
        pieces = D.piece_select(bitset_words(cand), self.blocked(peerID, n, allowDuplicates), counts, n, quota,
                                self.policy, seed).tolist()
        self.record(peerID, pieces)
        return pieces

    def MarkUnsent(self, peerID, i: int):
        self._mark(peerID, i, StatusUnsent)

    def MarkInvalid(self, peerID, i: int):
        self._mark(peerID, i, StatusInvalid)

    def _mark(self, peerID, i: int, s: int):
        for r in self.requests.get(i, ()):
            if r.PeerID == peerID:
                r.Status = s

    def Clear(self, i: int):
        self.requests.pop(i, None)
        for peerID in list(self.requestsByPeer):
            pm = self.requestsByPeer[peerID]
            pm.pop(i, None)
            if not pm:
                del self.requestsByPeer[peerID]

    def PendingPieces(self, peerID) -> list[int]:
        return sorted(i for i, r in self.requestsByPeer.get(peerID, {}).items() if r.Status == StatusPending)

    def ClearPeer(self, peerID):
        self.requestsByPeer.pop(peerID, None)
        for i, rs in self.requests.items():
            for j, r in enumerate(rs):
                if r.PeerID == peerID:
                    rs[j] = rs[-1]
                    rs.pop()
                    break

    def GetFailedRequests(self) -> list[Request]:
        failed = []
        for rs in self.requests.values():
            for r in rs:
                status = StatusExpired if r.Status == StatusPending and self.expired(r) else r.Status
                if status != StatusPending:
                    failed.append(Request(r.Piece, r.PeerID, status))
        return failed


def NewManager(clock, timeout, policy: str, pipelineLimit: int, seed: int = 0) -> Manager:
    """piecerequest.NewManager; an unknown policy is "invalid piece selection policy: <policy>"."""
    return Manager(clock, timeout, policy, pipelineLimit, seed)


class Dispatcher:
    """What a round needs of dispatch.Dispatcher: the torrent's Bitfield(), the peers' bitfields in
    a fixed order, its piece request Manager and the endgame rule (dispatcher.go:366-372)."""

    def __init__(self, n_pieces: int, manager: Manager, endgame_threshold: int | None = None,
                 disable_endgame: bool = False):
        self.n_pieces, self.manager = int(n_pieces), manager
        self.have = np.zeros(self.n_pieces, dtype=bool)
        self.peers: dict[object, np.ndarray] = {}
        self.endgame_threshold = manager.pipelineLimit if endgame_threshold is None else endgame_threshold
        self.disable_endgame = disable_endgame

    def AddPeer(self, peerID, bitfield):
        if peerID in self.peers:
            raise ValueError("peer already exists")
        b = np.asarray(bitfield, dtype=bool)
        if b.size != self.n_pieces:
            raise ValueError(f"peer bitfield of {b.size} pieces for a torrent of {self.n_pieces}")
        self.peers[peerID] = b.copy()

    def RemovePeer(self, peerID):
        del self.peers[peerID]
        self.manager.ClearPeer(peerID)

    def endgame(self) -> bool:
        return not self.disable_endgame and self.n_pieces - int(self.have.sum()) <= self.endgame_threshold

    def numPeersByPiece(self) -> np.ndarray:
        rows = [bitset_words(b) for b in self.peers.values()]
        return D.piece_availability(np.stack(rows) if rows else np.zeros((0, (self.n_pieces + 63) // 64), np.uint64),
                                    self.n_pieces)


def _round_inputs(ds, dups, flags, seeds):
    """(RequestBatch, bits, quota) of one round over the dispatchers ds: a torrent's rows are have,
    then (bitfield, blocked) a peer in the dispatcher's peer order; quota is requestQuota a peer."""
    batch = D.RequestBatch([d.n_pieces for d in ds], [len(d.peers) for d in ds], flags, seeds)
    bits = np.zeros(batch.total_words, dtype=np.uint64)
    quota = np.zeros(batch.total_peers, dtype=np.int32)
    for t, (d, dup) in enumerate(zip(ds, dups)):
        rows = batch.rows(bits, t)
        rows[0] = bitset_words(d.have)
        for p, (peerID, b) in enumerate(d.peers.items()):
            rows[1 + 2 * p] = bitset_words(b)
            rows[2 + 2 * p] = d.manager.blocked(peerID, d.n_pieces, dup)
            quota[int(batch.peer_off[t]) + p] = d.manager.requestQuota(peerID)
    return batch, bits, quota


def ReserveRound(dispatchers, placement: str = "host"):
    """ReservePieces for every peer of every dispatcher at one clock instant, in one call: the
    peers of a torrent in their order, each seeing the reservations of those before it (in endgame:
    only its own).  Returns one {peerID: [pieces]} a dispatcher; the picks are pending in the
    dispatchers' managers afterwards.  placement "host": krk_piece_request_round; "gpu":
    krk_piece_request_round_dev (an error without a device)."""
    if placement not in ("host", "gpu"):
        raise ValueError(f"ReserveRound: placement {placement!r} is neither \"host\" nor \"gpu\"")
    ds = list(dispatchers)
    limits = {d.manager.pipelineLimit for d in ds}
    if len(limits) > 1:
        raise ValueError(f"ReserveRound: one pipeline limit a round, got {sorted(limits)}")
    if not ds:
        return []
    limit = limits.pop()
    dups = [d.endgame() for d in ds]
    flags = [d.manager.policy | (D.PR_ALLOW_DUPLICATES if dup else 0) for d, dup in zip(ds, dups)]
    seeds = [d.manager.next_seed() if d.manager.policy == D.PR_SAMPLE else 0 for d in ds]
    batch, bits, quota = _round_inputs(ds, dups, flags, seeds)
    if placement == "host":
        _, picks, n_picked = D.piece_request_round(batch, bits, quota, limit)
    else:
        bits_dev, quota_dev = D.DeviceBuffer(bits.nbytes), D.DeviceBuffer(quota.nbytes)
        bits_dev.from_host(bits)
        quota_dev.from_host(quota)
        _, picks, n_picked = D.piece_request_round_dev(batch, bits_dev, quota_dev, limit)
    out = []
    for t, d in enumerate(ds):
        got = {}
        for p, peerID in enumerate(d.peers):
            k = int(batch.peer_off[t]) + p
            got[peerID] = picks[k, :int(n_picked[k])].tolist()
            d.manager.record(peerID, got[peerID])
        out.append(got)
    return out


def ResendRound(dispatchers, placement: str = "host"):
    """resendFailedPieceRequests for every dispatcher at one clock instant, in one call: a
    dispatcher's failed requests (expired, unsent, invalid) by piece and then by their position in
    requests[piece], each to the first peer, in the dispatcher's peer order, that holds the piece,
    has quota left and may be asked for it; an expired or invalid request never goes back to its
    own peer.  Returns one [(Request, target peerID or None)] a dispatcher; the resent pieces are
    pending on their targets in the dispatchers' managers afterwards.  No seed is drawn.  The
    dispatchers need not share a pipeline limit.  placement "host": krk_piece_resend_round; "gpu":
    krk_piece_resend_round_dev (an error without a device)."""
    if placement not in ("host", "gpu"):
        raise ValueError(f"ResendRound: placement {placement!r} is neither \"host\" nor \"gpu\"")
    ds = list(dispatchers)
    if not ds:
        return []
    failed = [sorted(d.manager.GetFailedRequests(), key=lambda r: r.Piece) for d in ds]  # stable: positions kept
    dups = [d.endgame() for d in ds]
    flags = [d.manager.policy | (D.PR_ALLOW_DUPLICATES if dup else 0) for d, dup in zip(ds, dups)]
    batch, bits, quota = _round_inputs(ds, dups, flags, 0)
    lists = []
    for d, rs in zip(ds, failed):
        index = {peerID: p for p, peerID in enumerate(d.peers)}
        lists.append([(r.Piece, index.get(r.PeerID, D.PR_NONE), r.Status) for r in rs])
    resend = D.ResendBatch(batch, lists)
    if placement == "host":
        target, _, _ = D.piece_resend_round(batch, resend, bits, quota, quota_left=False)
    else:
        bits_dev, quota_dev = D.DeviceBuffer(bits.nbytes), D.DeviceBuffer(quota.nbytes)
        bits_dev.from_host(bits)
        quota_dev.from_host(quota)
        target, _, _ = D.piece_resend_round_dev(batch, resend, bits_dev, quota_dev, quota_left=False)
    out = []
    for t, (d, rs) in enumerate(zip(ds, failed)):
        peers = list(d.peers)
        got = []
        for r, p in zip(rs, resend.split(target, t).tolist()):
            peerID = None if p == D.PR_NONE else peers[p]
            if peerID is not None:
                d.manager.record(peerID, [r.Piece])
            got.append((r, peerID))
        out.append(got)
    return out
