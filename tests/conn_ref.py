"""A plain-Python restatement of one connection round and one preemption sweep
(include/kraken_hip.h, "connection rounds"): connstate.State's rules over sets and dicts, one loop
an entry, no bit tricks, nothing shared with the library.  A helper module, not a test file."""

NONE = 0xFFFFFFFF
TORRENT_COMPLETE = 1
DISABLE_BLACKLIST = 1
ESTABLISHED, FAILED_IN, FAILED_OUT, CLOSED = 0, 1, 2, 3
(OK, FREED, NOOP, NOT_PENDING, BLACKLISTED_NOW, STILL_BLACKLISTED, AT_CAPACITY, ALREADY_PENDING, ALREADY_ACTIVE,
 TOO_MANY_MUTUAL, SELF, BLACKLISTED, TORRENT_IS_COMPLETE) = (0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40, 0x80, 0x100, 0x200,
                                                             0x400, 0x800, 0x1000)


class Torrent:
    """One torrent's connection state: sets of peer indices, expiry by peer (absent: 0)."""

    def __init__(self, n_peers, self_peer=NONE, flags=0, active=(), pending=(), expiry=None, capacity=0):
        self.n_peers, self.self_peer, self.flags = n_peers, self_peer, flags
        self.active, self.pending = set(active), set(pending)
        self.expiry = dict(expiry or {})
        self.capacity = capacity

    def blacklisted(self, p, now):
        return self.expiry.get(p, 0) > now

    def blacklist(self, p, now, duration, flags):
        if flags & DISABLE_BLACKLIST:
            return 0
        if self.blacklisted(p, now):
            return STILL_BLACKLISTED
        self.expiry[p] = now + duration
        return BLACKLISTED_NOW

    def add_pending(self, p, neighbours, max_mutual):
        if self.capacity == 0:
            return AT_CAPACITY
        if p in self.pending:
            return ALREADY_PENDING
        if p in self.active:
            return ALREADY_ACTIVE
        if neighbours is not None:
            mutual = 0
            for q in neighbours:
                if q < self.n_peers and (q in self.active or q in self.pending):
                    mutual += 1
            if mutual > max_mutual:
                return TOO_MANY_MUTUAL
        self.pending.add(p)
        self.capacity -= 1
        return OK


def conn_round(T, transitions, incoming, dials, now, duration, max_mutual, flags):
    """One torrent's round, T changed in place.  transitions: [(peer, kind)]; incoming: [(peer,
    iterable of neighbour indices or None)]; dials: [peer].  Returns (transition statuses, incoming
    statuses, dial statuses, incoming admitted, dials admitted, freed)."""
    ts, freed = [], 0
    for p, kind in transitions:
        if kind == ESTABLISHED:
            if p in T.pending:
                T.pending.remove(p)
                T.active.add(p)
                st = OK
            else:
                st = NOT_PENDING
        else:
            held = T.active if kind == CLOSED else T.pending
            if p in held:
                held.remove(p)
                T.capacity += 1
                freed += 1
                st = OK | FREED
            else:
                st = NOOP
            if kind in (FAILED_OUT, CLOSED):
                st |= T.blacklist(p, now, duration, flags)
        ts.append(st)
    ins = [T.add_pending(p, () if nb is None else nb, max_mutual) for p, nb in incoming]
    ds = []
    for p in dials:
        if T.flags & TORRENT_COMPLETE:
            ds.append(TORRENT_IS_COMPLETE)
        elif p == T.self_peer:
            ds.append(SELF)
        elif T.blacklisted(p, now):
            ds.append(BLACKLISTED)
        else:
            ds.append(T.add_pending(p, None, 0))
    return ts, ins, ds, ins.count(OK), ds.count(OK), freed


def preempt(n_peers, active, created, received, sent, now, tti, ttl):
    """The peers the tick closes, ascending: active and idle or expired (both strict)."""
    out = []
    for p in range(n_peers):
        if p not in active:
            continue
        c = max(created[p], 0)
        last = max(c, received[p], sent[p], 0)
        if now - last > tti or now - c > ttl:
            out.append(p)
    return out
