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


def marshal_bitfield(bools) -> bytes:
    """The wire form of a peer's bitfield, as the handshake's BitfieldMessage carries it: a
    willf/bitset MarshalBinary -- the bit length as a big-endian uint64, then the words, each a
    big-endian uint64."""
    b = np.asarray(bools, dtype=bool)
    return int(b.size).to_bytes(8, "big") + bitset_words(b).astype(">u8").tobytes()


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


class RequestTable:
    """The request tables of a set of dispatchers kept where the rounds read them
    (``krk_request_table_round`` / ``krk_request_table_round_dev``): the rows (have, then
    (bitfield, blocked) a peer) and one table of up to `cap` requests a torrent are uploaded once --
    placement "gpu": into device memory; "host": numpy arrays and the host forms -- and after that
    only a round's event lists cross the link.  The dispatchers give the shapes, the peers' order
    and bitfields, and their managers the clock, the timeout, the policy, the pipeline limit and
    the seeds (drawn exactly as ``ReserveRound`` draws them); the managers' own request maps are
    not used.  Events are queued on the host and applied by the next round.  A removed peer keeps
    its index: its row is zeroed and its requests dropped -- all of them, where the reference's
    ClearPeer leaves all but the first a piece behind (manager.go:188-196).

    The peer set changes where the rows lie (``krk_peer_round`` / ``krk_peer_round_dev``): every
    torrent's layout has `spare_peers` empty slots after its peers, ``AddPeer`` queues a join from
    the handshake's wire bytes into the lowest free slot, ``PeerComplete`` queues a Complete
    message, and ``Progress`` reads what the dispatcher derives from the rows.  A removed peer's
    slot is free again once a round has applied the removal.

    The torrents' own rows are loaded, checked, persisted and advertised where they lie
    (``krk_have_round`` / ``krk_have_round_dev``): ``Restore``, ``Verified``, ``Handshake``,
    ``Status`` and ``MissingPieces`` each run one have round at once; ``self.have``, the host's
    mirror, follows from the round's changed list or emitted status.

    The upload side runs on the same rows (``krk_serve_round`` / ``krk_serve_round_dev``):
    ``Requested`` queues a peer's PieceRequestMessage, ``Serve`` answers everything queued in one
    round, and ``LastPieceSent`` reads the resident array the round keeps.

    So does the download side's arrival step (``krk_receive_round`` / ``krk_receive_round_dev``):
    ``Received`` queues a peer's PiecePayloadMessage, ``Receive`` judges everything queued against
    the dispatchers' ``piece_sums`` in one round and queues the arrived pieces and the MarkInvalid
    pairs for the next table round, and ``LastGoodPieceReceived`` reads the resident array."""

    def __init__(self, dispatchers, placement: str = "host", cap: int = D.RT_MAX_ENTRIES, spare_peers: int = 0):
        if placement not in ("host", "gpu"):
            raise ValueError(f"RequestTable: placement {placement!r} is neither \"host\" nor \"gpu\"")
        self.ds, self.gpu = list(dispatchers), placement == "gpu"
        limits = {d.manager.pipelineLimit for d in self.ds}
        if len(limits) != 1:
            raise ValueError(f"RequestTable: one pipeline limit a table, got {sorted(limits)}")
        self.limit = limits.pop()
        self.peers = [list(d.peers) + [None] * int(spare_peers) for d in self.ds]  # a slot's peerID, None while free
        self.index = [{peerID: p for p, peerID in enumerate(d.peers)} for d in self.ds]
        self.have = [d.have.copy() for d in self.ds]  # the host's count of the arrived pieces: the endgame rule
        self._layout([d.manager.policy for d in self.ds], 0)
        self.table = D.TableBatch(self.batch, cap)
        bits = np.zeros(max(self.batch.total_words, 1), dtype=np.uint64)
        for t, d in enumerate(self.ds):
            rows = self.batch.rows(bits, t)
            rows[0] = bitset_words(d.have)
            for p, b in enumerate(d.peers.values()):
                rows[1 + 2 * p] = bitset_words(b)
        entries = np.zeros(max(self.table.total_entries, 1), dtype=D.RT_ENTRY)
        n_entries = np.zeros(len(self.ds), dtype=np.uint32)
        if self.gpu:
            self.bits, self.entries, self.n_entries = (D.DeviceBuffer(a.nbytes) for a in (bits, entries, n_entries))
            for buf, a in ((self.bits, bits), (self.entries, entries), (self.n_entries, n_entries)):
                buf.from_host(a)
            self.out = D.TableOutputs(self.batch, self.table, failed=True, pinned=False)
            self.failed = D.TableOutputs(self.batch, self.table, failed=True, pinned=True)  # Resend's list, page-locked
            self.picks = D.RequestOutputs(self.batch, self.limit)  # in HBM: recorded there, copied down once
        else:
            self.bits, self.entries, self.n_entries = bits, entries, n_entries
        self._events = {name: {} for name in ("arrived", "gone", "marks", "holds")}
        self.slots = D.PeerBatch(self.batch, [d.endgame_threshold for d in self.ds],
                                 [D.PE_DISABLE_ENDGAME if d.disable_endgame else 0 for d in self.ds],
                                 live=[range(len(d.peers)) for d in self.ds])
        self._joins, self._fulls = {}, {}  # {torrent: {slot: wire}}, {torrent: {slot}}
        self._refused = [[] for _ in self.ds]
        if self.gpu:
            self.progress = D.PeerOutputs(self.batch, pinned=True)  # read after one synchronise
            self._wire = D.DeviceBuffer(1 << 12)
        self._requests = [[] for _ in self.ds]  # (slot, peerID, index, offset, length), in arrival order
        self._serve, self._serve_out = None, None  # the ServeBatch, and on "gpu" its page-locked outputs, kept between rounds
        sent = np.zeros(max(self.batch.total_peers, 1), dtype=np.int64)  # LastPieceSent a slot, 0: never
        if self.gpu:
            self.sent = D.DeviceBuffer(sent.nbytes)
            self.sent.from_host(sent)
        else:
            self.sent = sent
        self._payloads = [[] for _ in self.ds]  # (slot, peerID, index, offset, length, sum), in arrival order
        self._receive, self._receive_out = None, None  # the ReceiveBatch, and on "gpu" its page-locked outputs
        self._expected_of = set()  # the torrents whose piece_sums lie in self.expected
        expected = np.zeros(max(self.batch.total_pieces, 1), dtype=np.uint32)
        if self.gpu:
            self.received, self.expected = D.DeviceBuffer(sent.nbytes), D.DeviceBuffer(expected.nbytes)
            self.received.from_host(sent)  # LastGoodPieceReceived a slot, 0: never
            self.expected.from_host(expected)
        else:
            self.received, self.expected = sent.copy(), expected

    def _layout(self, flags, seeds):
        self.batch = D.RequestBatch([d.n_pieces for d in self.ds], [len(ps) for ps in self.peers], flags, seeds)

    # -- events, queued until the next round
    def Arrived(self, t: int, pieces):
        """The pieces have arrived: set in have, their requests cleared (Manager.Clear)."""
        new = [int(i) for i in pieces if not self.have[t][int(i)]]
        self.have[t][new] = True
        self._events["arrived"].setdefault(t, set()).update(new)

    def Announced(self, t: int, peerID, pieces):
        """The peer announced the pieces (handleAnnouncePiece)."""
        p = self.index[t][peerID]
        self._events["holds"].setdefault(t, set()).update((int(i), p) for i in pieces)

    def MarkUnsent(self, t: int, peerID, i: int):
        self._events["marks"].setdefault(t, []).append((int(i), self.index[t][peerID], StatusUnsent))

    def MarkInvalid(self, t: int, peerID, i: int):
        self._events["marks"].setdefault(t, []).append((int(i), self.index[t][peerID], StatusInvalid))

    def RemovePeer(self, t: int, peerID):
        p = self.index[t].pop(peerID)
        self.slots.set_live(t, p, False)
        self._fulls.get(t, set()).discard(p)
        if self._joins.get(t, {}).pop(p, None) is not None:
            self.peers[t][p] = None  # never joined: nothing to drop, the slot is free at once
        else:
            self._events["gone"].setdefault(t, set()).add(p)  # peers[t][p] stays until a round has applied it

    def AddPeer(self, t: int, peerID, wire: bytes):
        """Dispatcher.AddPeer from the handshake: the peer takes the lowest free slot, its bitfield
        decoded from `wire` (``marshal_bitfield``'s form) by the next peer round."""
        if peerID in self.index[t]:
            raise ValueError("peer already exists")
        free = [p for p, x in enumerate(self.peers[t]) if x is None]
        if not free:
            raise ValueError("no free peer slot")
        self.peers[t][free[0]], self.index[t][peerID] = peerID, free[0]
        self.slots.set_live(t, free[0])
        self._joins.setdefault(t, {})[free[0]] = bytes(wire)

    def PeerComplete(self, t: int, peerID):
        """The peer sent Complete (handleComplete): it holds every piece."""
        self._fulls.setdefault(t, set()).add(self.index[t][peerID])

    def endgame(self, t: int) -> bool:
        d = self.ds[t]
        return not d.disable_endgame and d.n_pieces - int(self.have[t].sum()) <= d.endgame_threshold

    # -- the torrents' own rows: restored, checked, persisted and advertised where they lie
    def _have_round(self, flags, status=None, ok=None):
        """One have round (``krk_have_round`` / ``krk_have_round_dev``) now, and one synchronise:
        (the HaveBatch, its outputs by name as numpy arrays)."""
        have = D.HaveBatch(self.batch, [getattr(d, "piece_length", 0) for d in self.ds], [getattr(d, "length", 0) for d in self.ds])
        have.plan(flags, status)
        if self.gpu:
            side = None
            if have.sidecar.size:
                side = D.DeviceBuffer(have.sidecar.nbytes)
                side.from_host(have.sidecar)
            out = D.have_round_dev(self.batch, have, self.bits, side, ok, D.HaveOutputs(have, pinned=True))
            D.check(D.lib.krk_stream_sync(None))
            out = out.to_host()
        else:
            out = D.have_round(self.batch, have, self.bits, ok)
        return have, dict(zip(D.HaveOutputs.NAMES, out))

    def _every(self, flags):
        return [flags] * len(self.ds)

    def Restore(self, t: int, status_bytes=None, in_cache: bool = False):
        """restorePieces for torrent t: its row from the `_status` sidecar's bytes (one a piece), or
        every piece set for a torrent found in the cache.  Returns {"bad_status", "unexpected",
        "complete", "bytes"}; a sidecar of the wrong length is bad_status and changes nothing."""
        if (status_bytes is None) == (not in_cache):
            raise ValueError("Restore: either the sidecar's bytes or in_cache")
        flags = [0] * len(self.ds)
        flags[t] = D.HV_EMIT_STATUS | (D.HV_IN_CACHE if in_cache else D.HV_RESTORE)
        have, o = self._have_round(flags, None if in_cache else {t: status_bytes})
        self.have[t][:] = np.frombuffer(have.status_span(o["status_out"], t), dtype=np.uint8).astype(bool)
        return {"bad_status": bool(o["flags"][t] & D.HV_BAD_STATUS), "unexpected": int(o["n_unexpected"][t]),
                "complete": int(o["n_complete"][t]), "bytes": int(o["bytes"][t])}

    def Verified(self, ok, mode: str = "or"):
        """A verify result folded into every torrent's row where it lies.  ok: the bitfields
        ``krk_verify_batch_dev`` leaves in device memory (placement "gpu": a DeviceBuffer) or their
        uint64 words ("host"), torrent t's words from the sum of the word counts before it.  mode
        "or": the set pieces have arrived (their requests are cleared by the next table round);
        "and": a recheck, the pieces it does not confirm are lost.  Returns the changed pieces a
        torrent."""
        if mode not in ("or", "and"):
            raise ValueError(f"Verified: mode {mode!r} is neither \"or\" nor \"and\"")
        have, o = self._have_round(self._every(D.HV_MERGE_OR if mode == "or" else D.HV_MERGE_AND), ok=ok)
        out = []
        for t in range(len(self.ds)):
            out.append(o["changed"][have.changed_off[t]:have.changed_off[t] + int(o["n_changed"][t])].tolist())
            self.have[t][out[t]] = mode == "or"
            if mode == "or" and out[t]:
                self._events["arrived"].setdefault(t, set()).update(out[t])
        return out

    def Handshake(self):
        """info.Bitfield() as every handshake sends it: the wire bytes a torrent (``AddPeer``'s form)."""
        have, o = self._have_round(self._every(D.HV_EMIT_WIRE))
        return [have.wire_span(o["wire_out"], t) for t in range(len(self.ds))]

    def Status(self):
        """pieceStatusMetadata.Serialize: the `_status` sidecar's bytes a torrent."""
        have, o = self._have_round(self._every(D.HV_EMIT_STATUS))
        return [have.status_span(o["status_out"], t) for t in range(len(self.ds))]

    def MissingPieces(self):
        """Torrent.MissingPieces(): the pieces not yet held, ascending, a torrent."""
        have, o = self._have_round(self._every(D.HV_EMIT_MISSING))
        return [o["missing"][have.missing_off[t]:have.missing_off[t] + d.n_pieces - int(o["n_complete"][t])].tolist()
                for t, d in enumerate(self.ds)]

    # -- the upload side: the peers' piece requests answered on the resident rows
    def Requested(self, t: int, peerID, index: int, offset: int, length: int):
        """The peer's PieceRequestMessage (handlePieceRequest), queued in arrival order for the next
        ``Serve``.  The peer may be removed before then: its send fails and nothing is touched."""
        self._requests[t].append((self.index[t][peerID], peerID, int(index), int(offset), int(length)))

    def LastPieceSent(self, t: int, peerID) -> int:
        """The clock reading of the peer's last served piece, 0 for none: the resident array."""
        p = self.index[t][peerID]
        if p in self._joins.get(t, {}):  # joined since the last round: the slot's element is the peer before it
            return 0
        at = int(self.batch.peer_off[t]) + p
        return int(self.sent.to_host(np.int64, 1, offset=8 * at)[0] if self.gpu else self.sent[at])

    def Serve(self, token_size: int = 0):
        """One serve round over everything ``Requested`` queued, at the managers' clock, and one
        synchronise -- two on "gpu" when joins are queued: the peer round that applies them first
        reads their statuses back.  One dict a torrent: "sends", (peerID, piece, file_off, length,
        send_off) in arrival order -- the payloads lie end to end at send_off; "refusals", (peerID,
        index, error) with the reference's error texts; "gone", (peerID, index) in arrival order, the
        requests whose peer has left -- among them those whose slot another peer has taken since,
        which never enter the round and are in no count; "bytes" and "tokens", the totals (tokens:
        max(length * 8 // token_size, 1) a send, 0 when token_size is 0)."""
        if not self.ds:
            return []
        queued, self._requests = self._requests, [[] for _ in self.ds]
        for t, d in enumerate(self.ds):
            if queued[t] and not (hasattr(d, "length") and hasattr(d, "piece_length")):
                raise ValueError(f"Serve: torrent {t} has queued requests and no length / piece_length")
        self._peer_round()
        # A torrent without the attributes takes no request: any consistent pair will do.
        shape = [(getattr(d, "length", d.n_pieces), getattr(d, "piece_length", 1)) for d in self.ds]
        if self._serve is None or shape != list(zip(self._serve.length.tolist(), self._serve.piece_length.tolist())):
            self._serve = D.ServeBatch(self.batch, [s[0] for s in shape], [s[1] for s in shape], self.slots.live_off[:-1])
        serve = self._serve.plan({t: [(p, i, off, ln) for p, peerID, i, off, ln in qs if self.peers[t][p] == peerID]
                                  for t, qs in enumerate(queued) if qs})
        clocks = {d.manager.clock.Now() for d in self.ds}
        if len(clocks) != 1:
            raise ValueError("RequestTable: the dispatchers of a round share one clock reading")
        now = clocks.pop()
        if self.gpu:
            if self._serve_out is None or self._serve_out.sizes[0] < serve.sizes[0]:  # grown on demand, as _wire
                self._serve_out = D.ServeOutputs(serve, pinned=True, margin=serve.sizes[0])
            D.serve_round_dev(self.batch, serve, self.bits, self.slots.live, self.sent, now, self._serve_out, token_size)
            D.check(D.lib.krk_stream_sync(None))
            out = [getattr(self._serve_out, n).a for n in D.ServeOutputs.NAMES]
        else:
            out = D.serve_round(self.batch, serve, self.bits, self.slots.live, self.sent, now, token_size)
        o = {n: a.tolist() for n, a in zip(D.ServeOutputs.NAMES, out) if n in ("status", "file_off", "len", "send_off")}
        errors = {D.SV_CHUNK: lambda i, n: "reading / writing chunk of piece not supported",
                  D.SV_INDEX: lambda i, n: f"invalid piece index {i}: num pieces = {n}",
                  D.SV_INCOMPLETE: lambda i, n: "piece not complete"}
        res = []
        for t, qs in enumerate(queued):
            got = {"sends": [], "refusals": [], "gone": [], "bytes": int(out[8][t]), "tokens": int(out[9][t]) if token_size else 0}
            r = serve.req_off[t]
            for p, peerID, index, _, _ in qs:
                if self.peers[t][p] != peerID:  # the slot is another peer's by now: this one has left
                    got["gone"].append((peerID, index))
                    continue
                st = o["status"][r]
                if st == D.SV_OK:
                    got["sends"].append((peerID, index, o["file_off"][r], o["len"][r], o["send_off"][r]))
                elif st == D.SV_GONE:
                    got["gone"].append((peerID, index))
                else:
                    got["refusals"].append((peerID, index, errors[st](index, self.ds[t].n_pieces)))
                r += 1
            res.append(got)
        return res

    # -- the download side: the peers' piece payloads judged on the resident rows
    def Received(self, t: int, peerID, index: int, offset: int, length: int, sum=None):
        """The peer's PiecePayloadMessage (handlePiecePayload), queued in arrival order for the next
        ``Receive``; `sum`: the CRC-32 of its bytes, or None when ``Receive`` is given the sums."""
        self._payloads[t].append((self.index[t][peerID], peerID, int(index), int(offset), int(length), sum))

    def LastGoodPieceReceived(self, t: int, peerID) -> int:
        """The clock reading of the peer's last good piece, 0 for none: the resident array."""
        p = self.index[t][peerID]
        if p in self._joins.get(t, {}):  # joined since the last round: the slot's element is the peer before it
            return 0
        at = int(self.batch.peer_off[t]) + p
        return int(self.received.to_host(np.int64, 1, offset=8 * at)[0] if self.gpu else self.received[at])

    def Receive(self, sums=None):
        """One receive round over everything ``Received`` queued, at the managers' clock, and one
        synchronise -- two on "gpu" when joins are queued, as in ``Serve``.  sums: None for the
        per-message sums, else one uint32 a queued payload, torrent after torrent and each
        torrent's in arrival order: a DeviceBuffer on "gpu" (where ``krk_piece_sums_dev`` left
        them), an array on "host".  The expected sums are the `piece_sums` of every dispatcher with
        queued payloads, uploaded once and kept.  A payload whose slot another peer has taken since
        is judged and written all the same, attributed to nobody.  The arrived pieces and the
        MarkInvalid pairs are queued for the next table round and ``self.have`` follows.  One dict a
        torrent: "writes", (peerID or None, piece, file_off) in arrival order; "duplicates",
        (peerID, index); "invalid", (peerID, index, error) with the reference's error texts;
        "announce", (piece, from peerID or None) ascending by piece -- AnnouncePiece goes to every
        live peer but that one; "complete", "completed_now" and "bytes" (BytesDownloaded)."""
        if not self.ds:
            return []
        for t, d in enumerate(self.ds):
            if self._payloads[t] and not all(hasattr(d, a) for a in ("length", "piece_length", "piece_sums")):
                raise ValueError(f"Receive: torrent {t} has queued payloads and no length / piece_length / piece_sums")
        if sums is None and any(q[5] is None for qs in self._payloads for q in qs):
            raise ValueError("Receive: a queued payload has no sum and none were given")
        queued, self._payloads = self._payloads, [[] for _ in self.ds]
        self._peer_round()
        for t, d in enumerate(self.ds):  # the MetaInfo's sums, once a torrent
            if queued[t] and t not in self._expected_of:
                mine = np.ascontiguousarray(d.piece_sums, dtype=np.uint32)
                if mine.size != d.n_pieces:
                    raise ValueError(f"Receive: torrent {t}: {mine.size} piece sums for {d.n_pieces} pieces")
                at = int(self.batch.piece_off[t])
                if self.gpu:
                    self.expected.from_host(mine, offset=4 * at)
                else:
                    self.expected[at:at + mine.size] = mine
                self._expected_of.add(t)
        # A torrent without the attributes takes no payload: any consistent pair will do.
        shape = [(getattr(d, "length", d.n_pieces), getattr(d, "piece_length", 1)) for d in self.ds]
        if self._receive is None or shape != list(zip(self._receive.length.tolist(), self._receive.piece_length.tolist())):
            self._receive = D.ReceiveBatch(self.batch, [s[0] for s in shape], [s[1] for s in shape])
        rec = self._receive.plan({t: [(p if self.peers[t][p] == peerID else D.PR_NONE, i, off, ln) for p, peerID, i, off, ln, _ in qs]
                                  for t, qs in enumerate(queued) if qs})
        if sums is None:
            sums = np.array([q[5] for qs in queued for q in qs], dtype=np.uint32)
            if self.gpu:
                host, sums = sums, D.DeviceBuffer(max(sums.nbytes, 4))
                sums.from_host(host)
        clocks = {d.manager.clock.Now() for d in self.ds}
        if len(clocks) != 1:
            raise ValueError("RequestTable: the dispatchers of a round share one clock reading")
        now = clocks.pop()
        if self.gpu:
            if self._receive_out is None or self._receive_out.sizes[0] < rec.sizes[0]:  # grown on demand, as _wire
                self._receive_out = D.ReceiveOutputs(rec, pinned=True, margin=rec.sizes[0])
            D.receive_round_dev(self.batch, rec, self.bits, sums, self.expected, self.received, now, self._receive_out)
            D.check(D.lib.krk_stream_sync(None))
            out = [getattr(self._receive_out, n).a for n in D.ReceiveOutputs.NAMES]
        else:
            out = D.receive_round(self.batch, rec, self.bits, sums, self.expected, self.received, now)
        o = dict(zip(D.ReceiveOutputs.NAMES, out))
        errors = {D.RV_CHUNK: lambda i, n: "reading / writing chunk of piece not supported",
                  D.RV_INDEX: lambda i, n: f"invalid piece index {i}: num pieces = {n}", D.RV_BAD_SUM: lambda i, n: "invalid piece sum"}
        res = []
        for t, qs in enumerate(queued):
            r, k, m, flags = rec.pay_off[t], int(o["n_arrived"][t]), int(o["n_marks"][t]), int(o["flags"][t])
            got = {"writes": [], "duplicates": [], "invalid": [], "complete": bool(flags & D.RV_COMPLETE),
                   "completed_now": bool(flags & D.RV_COMPLETED_NOW), "bytes": int(o["bytes"][t])}
            name = lambda p: None if p == D.PR_NONE else self.peers[t][p]  # noqa: E731
            for (p, peerID, index, _, _, _), st, off in zip(qs, o["status"][r:r + len(qs)].tolist(), o["file_off"][r:r + len(qs)].tolist()):
                if st == D.RV_OK:
                    got["writes"].append((peerID if self.peers[t][p] == peerID else None, index, off))
                elif st == D.RV_DUPLICATE:
                    got["duplicates"].append((peerID, index))
                else:
                    got["invalid"].append((peerID, index, errors[st](index, self.ds[t].n_pieces)))
            pieces = o["arrived"][r:r + k].tolist()
            got["announce"] = [(i, name(p)) for i, p in zip(pieces, o["arrived_from"][r:r + k].tolist())]
            if pieces:
                self.have[t][pieces] = True
                self._events["arrived"].setdefault(t, set()).update(pieces)
            if m:
                self._events["marks"].setdefault(t, []).extend(tuple(int(x) for x in mk) for mk in o["marks"][r:r + m].tolist())
            res.append(got)
        return res

    # -- rounds
    def _peer_round(self, always=False):
        """One peer round over the queued joins and fulls (none queued: only when `always`).  The
        joins' statuses are read back: a peer whose bitfield was malformed leaves the index again.
        Returns the five outputs when they were read (after one synchronise), else None."""
        if not (self._joins or self._fulls or always):
            return None
        joins, self._joins = self._joins, {}
        fulls, self._fulls = self._fulls, {}
        self.slots.events({t: sorted(j.items()) for t, j in joins.items()}, {t: sorted(f) for t, f in fulls.items()})
        for t, j in joins.items():  # a new connection has sent and received nothing: its slot's LastPieceSent and
            for p in j:             # LastGoodPieceReceived, with the joins' upload
                at = int(self.batch.peer_off[t]) + p
                if self.gpu:
                    self.sent.from_host(np.zeros(1, dtype=np.int64), offset=8 * at)
                    self.received.from_host(np.zeros(1, dtype=np.int64), offset=8 * at)
                else:
                    self.sent[at] = self.received[at] = 0
        if self.gpu:
            if self.slots.wire.size > self._wire.nbytes:
                self._wire = D.DeviceBuffer(2 * self.slots.wire.size)
            self._wire.from_host(self.slots.wire)
            D.peer_round_dev(self.batch, self.slots, self.bits, self._wire, self.progress)
            if not (joins or always):
                return None
            D.check(D.lib.krk_stream_sync(None))
            out = self.progress.to_host()
        else:
            out = D.peer_round(self.batch, self.slots, self.bits)
        for t, j in joins.items():
            for p in j:
                if out[4][int(self.batch.peer_off[t]) + p] & D.PE_BAD_BITFIELD:
                    self._refused[t].append(self.peers[t][p])
                    del self.index[t][self.peers[t][p]]
                    self.peers[t][p] = None
                    self.slots.set_live(t, p, False)
        return out

    def Progress(self):
        """What the dispatchers derive from the rows, after a peer round over whatever is queued
        and one synchronise.  One dict a torrent: remaining, complete, endgame; held and wanted by
        peerID; close and notify, the peerIDs complete() would close and send Complete to; refused,
        the peers whose join was malformed since the last call.  Pieces queued by ``Arrived`` count
        once a table round has applied them."""
        if not self.ds:
            return []
        remaining, tflags, held, wanted, status = self._peer_round(always=True)
        out = []
        for t, ps in enumerate(self.peers):
            at = int(self.batch.peer_off[t])
            named = [(p, peerID) for p, peerID in enumerate(ps) if peerID in self.index[t]]
            out.append({"remaining": int(remaining[t]), "complete": bool(tflags[t] & D.PE_TORRENT_COMPLETE),
                        "endgame": bool(tflags[t] & D.PE_ENDGAME),
                        "held": {peerID: int(held[at + p]) for p, peerID in named},
                        "wanted": {peerID: int(wanted[at + p]) for p, peerID in named},
                        "close": [peerID for p, peerID in named if status[at + p] & D.PE_CLOSE],
                        "notify": [peerID for p, peerID in named if status[at + p] & D.PE_NOTIFY],
                        "refused": self._refused[t]})
            self._refused[t] = []
        return out

    def _round(self, out=None, records=None, picks=None):
        """One table round at the dispatchers' clock: the queued events, `records`, the picks."""
        ev, self._events = self._events, {name: {} for name in self._events}
        for t, gone in ev["gone"].items():  # applied by this round: the slots are free after it
            for p in gone:
                self.peers[t][p] = None
        self.table.events(arrived={t: sorted(s) for t, s in ev["arrived"].items()},
                          gone={t: sorted(s) for t, s in ev["gone"].items()}, marks=ev["marks"],
                          holds={t: sorted(s, key=lambda h: h[::-1]) for t, s in ev["holds"].items()}, records=records)
        clocks = {(d.manager.clock.Now(), d.manager.timeout) for d in self.ds}
        if len(clocks) != 1:
            raise ValueError("RequestTable: the dispatchers of a round share one clock reading and one timeout")
        now, timeout = clocks.pop()
        if self.gpu:
            D.request_table_round_dev(self.batch, self.table, self.bits, self.entries, self.n_entries, now, timeout,
                                      self.limit, out or self.out, picks_dev=picks.picks if picks else None,
                                      n_picked_dev=picks.n_picked if picks else None)
            return None
        return D.request_table_round(self.batch, self.table, self.bits, self.entries, self.n_entries, now, timeout,
                                     self.limit, picks=picks[0] if picks else None, n_picked=picks[1] if picks else None)

    def Reserve(self):
        """ReserveRound over the resident tables: a table round (the events, then quotas and blocked
        rows derived where they lie), the request round on them, and a table round that records its
        picks from where the request round left them.  Returns one {peerID: [pieces]} a torrent."""
        if not self.ds:
            return []
        dups = [self.endgame(t) for t in range(len(self.ds))]
        flags = [d.manager.policy | (D.PR_ALLOW_DUPLICATES if dup else 0) for d, dup in zip(self.ds, dups)]
        self._layout(flags, [d.manager.next_seed() if d.manager.policy == D.PR_SAMPLE else 0 for d in self.ds])
        self._peer_round()
        if self.gpu:
            self._round()
            D.piece_request_round_dev(self.batch, self.bits, self.out.quota, self.limit, out=self.picks)
            self._round(picks=self.picks)
            D.check(D.lib.krk_stream_sync(None))
            _, picks, n_picked = self.picks.to_host()
        else:
            quota = self._round()[0]
            _, picks, n_picked = D.piece_request_round(self.batch, self.bits, quota, self.limit)
            self._round(picks=(picks, n_picked))
        return [{peerID: picks[int(self.batch.peer_off[t]) + p, :int(n_picked[int(self.batch.peer_off[t]) + p])].tolist()
                 for p, peerID in enumerate(ps) if peerID is not None} for t, ps in enumerate(self.peers)]

    def Resend(self):
        """ResendRound over the resident tables: a table round that leaves the failed list in
        page-locked memory (one stream synchronise), the resend round on the resident rows, and a
        table round that records the targets.  Returns one [(Request, target peerID or None)] a
        torrent; the Request's PeerID is the peer the request failed on."""
        if not self.ds:
            return []
        dups = [self.endgame(t) for t in range(len(self.ds))]
        self._layout([d.manager.policy | (D.PR_ALLOW_DUPLICATES if dup else 0) for d, dup in zip(self.ds, dups)], 0)
        self._peer_round()
        if self.gpu:
            self._round(out=self.failed)
            D.check(D.lib.krk_stream_sync(None))
            quota, failed, n_failed, _ = self.failed.quota, *self.failed.to_host()[1:]
        else:
            quota, failed, n_failed, _ = self._round()
        lists = [[tuple(int(x) for x in f) for f in self.table.split(failed, t, n_failed[t])] for t in range(len(self.ds))]
        resend = D.ResendBatch(self.batch, lists)
        if self.gpu:
            target, _, _ = D.piece_resend_round_dev(self.batch, resend, self.bits, quota, quota_left=False)
        else:
            target, _, _ = D.piece_resend_round(self.batch, resend, self.bits, quota, quota_left=False)
        out, records = [], {}
        for t, fl in enumerate(lists):
            got = []
            for (piece, peer, status), p in zip(fl, resend.split(target, t).tolist()):
                if p != D.PR_NONE:
                    records.setdefault(t, []).append((piece, p))
                got.append((Request(piece, self.peers[t][peer], status), None if p == D.PR_NONE else self.peers[t][p]))
            out.append(got)
        self._round(records=records)
        return out
