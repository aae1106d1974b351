"""Connection rounds and preemption sweeps (conn_round.hip, conn_math.hpp) at the kernel's word,
step and one-register-a-lane edges: the cases, their expectations and the comparison, shared by
tests/test_gpu_conn_matrix.py and tests/test_gpu_conn_round.py (krk_conn_round_dev,
krk_conn_preempt_dev on the production library) and tests/test_conn_matrix_cpu.py (krk_conn_round,
krk_conn_preempt, the host forms the kernels are documented to equal).  A helper module, not a test
file.

A case is one ROUND over one or more torrents.  Its inputs come from a splitmix64 stream written out
here (no library, no numpy generator), its expectation is tests/conn_ref.py's restatement, never the
library, and tests/golden/conn_rounds.json records that expectation (`python -m tests.conn_matrix
--write` regenerates it).  Every array starts with BASE canary elements, every torrent's region in
every array is followed by GAP canaries, and the outputs are prefilled with canaries, so a case's
expected output is the whole buffers: every owned element stored, nothing else touched.

 matrix   P in {1, 63, 64, 65, 4096, 4097}, six torrents a case whose three lists cycle through the
          lengths 0, 1, 63, 64, 65 and 129 (transitions are capped at P: they are distinct); random
          active, pending and blacklist state, garbage in the tail bits of every row
 named    one property each (see named())
 sweeps   the preemption tick at its thresholds (see sweeps())"""
import ctypes as C
import hashlib
import json
import os

import numpy as np

from kraken_amd import _capi
from kraken_amd._capi import check, lib
from tests import conn_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conn_rounds.json")
SEED = 20261021
BASE, GAP = 3, 2
CANARY32 = 0xA5A5A5A5
CANARY64 = 0x5A5A5A5A5A5A5A5A
CANARY_I64 = 0x5A5A5A5A5A5A5A5A  # as int64: positive
M64 = (1 << 64) - 1
PS = (1, 63, 64, 65, 4096, 4097)
LENGTHS = (0, 1, 63, 64, 65, 129)
NOW, DURATION = 1000, 30

assert (R.NONE, R.TORRENT_COMPLETE, R.DISABLE_BLACKLIST) == (_capi.KRK_CN_NONE, _capi.KRK_CN_TORRENT_COMPLETE,
                                                             _capi.KRK_CN_DISABLE_BLACKLIST)
assert (R.ESTABLISHED, R.FAILED_IN, R.FAILED_OUT, R.CLOSED) == (_capi.KRK_CN_ESTABLISHED, _capi.KRK_CN_FAILED_IN,
                                                                _capi.KRK_CN_FAILED_OUT, _capi.KRK_CN_CLOSED)
assert (R.OK, R.FREED, R.NOOP, R.NOT_PENDING, R.BLACKLISTED_NOW, R.STILL_BLACKLISTED, R.AT_CAPACITY, R.ALREADY_PENDING,
        R.ALREADY_ACTIVE, R.TOO_MANY_MUTUAL, R.SELF, R.BLACKLISTED, R.TORRENT_IS_COMPLETE) == (
    _capi.KRK_CN_OK, _capi.KRK_CN_FREED, _capi.KRK_CN_NOOP, _capi.KRK_CN_NOT_PENDING, _capi.KRK_CN_BLACKLISTED_NOW,
    _capi.KRK_CN_STILL_BLACKLISTED, _capi.KRK_CN_AT_CAPACITY, _capi.KRK_CN_ALREADY_PENDING, _capi.KRK_CN_ALREADY_ACTIVE,
    _capi.KRK_CN_TOO_MANY_MUTUAL, _capi.KRK_CN_SELF, _capi.KRK_CN_BLACKLISTED, _capi.KRK_CN_TORRENT_IS_COMPLETE)


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


class Stream:
    """A splitmix64 stream: the cases' only source of inputs."""

    def __init__(self, *salt):
        self.s = SEED
        for v in salt:
            self.s = splitmix64(self.s ^ (int(v) & M64))

    def word(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & M64
        return splitmix64(self.s)

    def below(self, n):
        return self.word() % n

    def subset(self, n, one_in):
        return {i for i in range(n) if self.below(one_in) == 0}


def words(p):
    return (p + 63) // 64


def tail(p):
    """The bits of the last word past peer p - 1 (0 when p is a multiple of 64)."""
    return (M64 << (p % 64)) & M64 if p % 64 else 0


def row_of(members, p, garbage=0):
    """words(p) words with the members' bits, the tail bits taken from `garbage`."""
    row = [0] * words(p)
    for i in members:
        row[i // 64] |= 1 << (i % 64)
    if row:
        row[-1] |= garbage & tail(p)
    return row


class Tor:
    """One torrent of a case: its state before the round and its three lists."""

    def __init__(self, P, capacity, self_peer=R.NONE, flags=0, active=(), pending=(), expiry=None, transitions=(),
                 incoming=(), dials=(), garbage=0):
        self.P, self.capacity, self.self_peer, self.flags = P, capacity, self_peer, flags
        self.active, self.pending, self.expiry = set(active), set(pending), dict(expiry or {})
        self.transitions, self.dials = list(transitions), list(dials)
        self.incoming = [(p, None if nb is None else set(nb)) for p, nb in incoming]
        self.garbage = garbage  # tail bits of the active, pending and neighbour rows

    def ref(self):
        return R.Torrent(self.P, self.self_peer, self.flags, self.active, self.pending, self.expiry, self.capacity)


class Case:
    def __init__(self, label, torrents, now=NOW, duration=DURATION, max_mutual=10, flags=0):
        self.label, self.torrents = label, torrents
        self.now, self.duration, self.max_mutual, self.flags = now, duration, max_mutual, flags
        k = len(torrents)
        bits, expiry, neigh = [CANARY64] * BASE, [CANARY_I64] * BASE, [CANARY64] * BASE
        at = [BASE, BASE, BASE]  # next element of the transition, incoming and dial arrays
        self.structs = (_capi.krk_conn_torrent * max(k, 1))()
        self.lists = (_capi.krk_conn_lists * max(k, 1))()
        trans, inc, dials = [], [], []
        self.regions = []  # (bits_off, peer_off, (trans_off, in_off, dial_off)) a torrent
        for t, T in enumerate(torrents):
            self.structs[t] = _capi.krk_conn_torrent(T.P, T.self_peer, T.flags, 0, len(bits), len(expiry), 0)
            self.regions.append((len(bits), len(expiry), tuple(at)))
            bits += row_of(T.active, T.P, T.garbage) + row_of(T.pending, T.P, T.garbage >> 7) + [CANARY64] * GAP
            expiry += [T.expiry.get(p, 0) for p in range(T.P)] + [CANARY_I64] * GAP
            self.lists[t] = _capi.krk_conn_lists(at[0], len(T.transitions), at[1], len(T.incoming), at[2], len(T.dials))
            trans += [(at[0] + j, e) for j, e in enumerate(T.transitions)]
            for j, (p, nb) in enumerate(T.incoming):
                if nb is None:
                    inc.append((at[1] + j, p, _capi.KRK_CN_NO_ROW))
                else:
                    inc.append((at[1] + j, p, len(neigh)))
                    neigh += row_of(nb, T.P, splitmix64(T.garbage ^ (j + 1))) + [CANARY64] * GAP
            dials += [(at[2] + j, p) for j, p in enumerate(T.dials)]
            at = [at[0] + len(T.transitions) + GAP, at[1] + len(T.incoming) + GAP, at[2] + len(T.dials) + GAP]
        self.sizes = tuple(at)  # elements of the three status arrays
        self.bits = np.array(bits, dtype=np.uint64)
        self.expiry = np.array(expiry, dtype=np.int64)
        self.capacity = np.array([T.capacity for T in torrents] + [CANARY32] * GAP, dtype=np.uint32)
        self.neighbors = np.array(neigh, dtype=np.uint64)
        for a in (self.bits, self.expiry, self.capacity, self.neighbors):
            a.setflags(write=False)
        self.transitions = (_capi.krk_conn_transition * at[0])()
        for j, (p, kind) in trans:
            self.transitions[j] = _capi.krk_conn_transition(p, kind)
        self.incoming = (_capi.krk_conn_incoming * at[1])()
        for j, p, off in inc:
            self.incoming[j] = _capi.krk_conn_incoming(p, 0, off)
        self.dials = np.full(at[2], CANARY32, dtype=np.uint32)
        for j, p in dials:
            self.dials[j] = p
        self._ref = None

    def ref(self):
        """The restatement's [(torrent after the round, its conn_round result)]."""
        if self._ref is None:
            self._ref = []
            for T in self.torrents:
                S = T.ref()
                self._ref.append((S, R.conn_round(S, T.transitions, T.incoming, T.dials, self.now, self.duration,
                                                  self.max_mutual, self.flags)))
        return self._ref

    def want(self):
        """The whole buffers after the call: (bits, expiry, capacity, trans, in, dial statuses,
        n_admitted, n_freed), canaries where nobody owns.  n_admitted and n_freed are indexed from 0
        by the torrent: their canaries follow."""
        bits, expiry, cap = self.bits.copy(), self.expiry.copy(), self.capacity.copy()
        outs = [np.full(k, CANARY32, dtype=np.uint32) for k in self.sizes]
        k = len(self.torrents)
        n_adm = np.full(2 * k + BASE + GAP, CANARY32, dtype=np.uint32)
        n_freed = np.full(k + BASE + GAP, CANARY32, dtype=np.uint32)
        for t, (T, (S, (ts, ins, ds, a_in, a_dial, freed))) in enumerate(zip(self.torrents, self.ref())):
            b_off, p_off, l_off = self.regions[t]
            wp = words(T.P)
            for r, members in enumerate((S.active, S.pending)):
                for w in range(wp):
                    keep = int(bits[b_off + r * wp + w]) & (tail(T.P) if w == wp - 1 else 0)
                    bits[b_off + r * wp + w] = keep
                for p in members:
                    bits[b_off + r * wp + p // 64] |= np.uint64(1 << (p % 64))
            for p in range(T.P):
                expiry[p_off + p] = S.expiry.get(p, 0)
            cap[t] = S.capacity
            for o, off, st in zip(outs, l_off, (ts, ins, ds)):
                o[off:off + len(st)] = st
            n_adm[2 * t:2 * t + 2] = (a_in, a_dial)
            n_freed[t] = freed
        return (bits, expiry, cap, *outs, n_adm, n_freed)

    def out_sizes(self):
        """Elements of the five output arrays."""
        k = len(self.torrents)
        return (*self.sizes, 2 * k + BASE + GAP, k + BASE + GAP)


# ------------------------------------------------------------------ the cases
def _matrix():
    out = []
    for p in PS:
        tors = []
        for k, n in enumerate(LENGTHS):
            rng = Stream(p, n)
            active = rng.subset(p, 5)
            pending = rng.subset(p, 4) - active
            expiry = {i: NOW + (rng.below(3) - 1) for i in rng.subset(p, 6)}  # now - 1, now, now + 1
            n_tr = min(n, p)
            tr_peers = sorted(range(p) if n_tr == p else {rng.below(p) for _ in range(4 * n_tr)})[:n_tr]
            while len(tr_peers) < n_tr:
                tr_peers = sorted(set(tr_peers) | {rng.below(p)})
            n_in, n_dial = LENGTHS[(k + 2) % 6], LENGTHS[(k + 4) % 6]
            incoming = [(rng.below(p), None if j % 5 == 4 else rng.subset(p, 2 + rng.below(60))) for j in range(n_in)]
            dials = [rng.below(p) for _ in range(n_dial)]
            tors.append(Tor(p, capacity=(0, 3, 40, 200, 64, 7)[k], self_peer=(R.NONE, 0, p - 1)[k % 3], active=active,
                            pending=pending, expiry=expiry, transitions=[(q, rng.below(4)) for q in tr_peers],
                            incoming=incoming, dials=dials, garbage=rng.word()))
        out.append(Case(f"matrix P={p}", tors, max_mutual=(3, 10, 40)[len(out) % 3]))
    return out


def named():
    """One property a case."""
    out = []

    def add(label, *tors, **kw):
        out.append(Case(label, list(tors), **kw))

    fresh = list(range(100, 180))  # 80 dials nobody holds
    for label, cap in (("capacity 0", 0), ("capacity 1", 1), ("capacity exactly the admissible dials", 80),
                       ("capacity one fewer than the admissible dials", 79), ("capacity runs out at dial entry 63", 64),
                       ("capacity runs out at dial entry 64", 65)):
        add(label, Tor(200, cap, active={3}, pending={4}, dials=fresh))
    # entries that are not admissible do not use capacity: the last slot goes to a later entry
    add("capacity counts admissions only", Tor(200, 3, active={100, 102}, pending={101}, self_peer=103,
                                               expiry={104: NOW + 1}, dials=list(range(100, 112))))
    add("duplicate dials inside one step", Tor(130, 10, dials=[5, 7, 5, 129, 7, 5, 64, 129, 64]))
    add("a duplicate of a dial the capacity cut", Tor(130, 1, dials=[3, 4, 4, 3]))
    add("a duplicate after the last slot went to its first occurrence", Tor(130, 2, dials=[3, 4, 4, 3, 5]))
    add("duplicate dials at entries 63 and 64", Tor(300, 100, dials=list(range(63)) + [200, 200] + list(range(70, 100))))
    add("duplicate dials across steps, the capacity gone in between", Tor(300, 64, dials=list(range(64)) + [0, 200]))
    add("self_peer present", Tor(65, 5, self_peer=64, dials=[1, 64, 2]))
    add("self_peer absent", Tor(65, 5, self_peer=63, dials=[1, 64, 2]))
    add("self_peer NONE", Tor(65, 5, dials=[1, 64, 2]))
    add("expiry == now is not blacklisted, now + 1 is", Tor(70, 9, expiry={1: NOW, 2: NOW + 1, 69: NOW - 1}, dials=[1, 2, 69]))
    add("a dial of a peer blacklisted by this round's phase 1",
        Tor(70, 0, active={9}, pending={65}, transitions=[(9, R.CLOSED), (65, R.FAILED_OUT)], dials=[9, 65, 10, 11, 12]))
    add("mutual count equal to max_mutual admits, one more rejects",
        Tor(130, 9, active={1, 64}, pending={2}, incoming=[(10, {1, 2, 64, 99}), (11, {1, 2, 64, 10})]), max_mutual=3)
    add("a mutual count pushed over the limit by the entry before",
        Tor(130, 9, active={1}, pending={2}, incoming=[(12, {1, 2, 50}), (13, {1, 2, 12}), (14, {1, 13, 12})]), max_mutual=2)
    add("max_mutual 0", Tor(64, 9, active={1}, incoming=[(5, set()), (6, {1}), (7, None), (8, {9})]), max_mutual=0)
    add("NO_ROW", Tor(4097, 4, active=set(range(0, 4097, 3)), incoming=[(1, None), (4096, None)]), max_mutual=0)
    add("incoming: the check order", Tor(70, 2, active={1}, pending={2},
                                         incoming=[(1, {1, 2}), (2, {1, 2}), (3, {1, 2}), (4, None), (1, None), (5, None), (6, None)]),
        max_mutual=1)
    add("the blacklist is not consulted for incoming handshakes", Tor(70, 2, expiry={5: NOW + 9}, incoming=[(5, None)]))
    kinds = (R.ESTABLISHED, R.FAILED_IN, R.FAILED_OUT, R.CLOSED)
    add("every transition kind from every state",
        Tor(20, 1, pending={0, 1, 2, 3}, active={4, 5, 6, 7}, transitions=[(p, kinds[p % 4]) for p in range(12)]))
    add("two transitions in one word and one in the next", Tor(130, 0, pending={62, 63, 64}, active={129},
                                                              transitions=[(62, R.ESTABLISHED), (63, R.FAILED_IN),
                                                                           (64, R.ESTABLISHED), (129, R.CLOSED)]))
    add("STILL_BLACKLISTED", Tor(10, 0, active={1, 2}, pending={3}, expiry={1: NOW + 5, 2: NOW, 3: NOW + 1, 4: NOW + 2},
                                 transitions=[(1, R.CLOSED), (2, R.CLOSED), (3, R.FAILED_OUT), (4, R.CLOSED)]))
    add("DISABLE_BLACKLIST", Tor(10, 0, active={1, 2}, expiry={5: NOW + 5}, transitions=[(1, R.CLOSED), (3, R.FAILED_OUT)],
                                 dials=[1, 5, 6]), flags=R.DISABLE_BLACKLIST)
    add("TORRENT_COMPLETE", Tor(70, 5, flags=R.TORRENT_COMPLETE, self_peer=1, pending={4}, expiry={2: NOW + 1},
                                transitions=[(4, R.ESTABLISHED)], incoming=[(9, None)], dials=[1, 2, 3, 4, 69]))
    add("freed capacity is used by the same round", Tor(70, 0, pending={1}, active={2},
                                                        transitions=[(1, R.FAILED_IN), (2, R.CLOSED)],
                                                        incoming=[(10, None)], dials=[11, 12]))
    add("three torrents at non-adjacent offsets",
        Tor(65, 2, active={64}, transitions=[(64, R.CLOSED)], incoming=[(0, {64})], dials=[1, 2, 3], garbage=M64),
        Tor(1, 1, dials=[0, 0]),
        Tor(130, 70, self_peer=129, pending={5}, transitions=[(5, R.ESTABLISHED)], incoming=[(6, {5, 129}), (7, None)],
            dials=list(range(129, 59, -1)), garbage=M64))
    add("no peers and no lists", Tor(0, 5), Tor(3, 1, dials=[2]))
    add("the longest blacklist", Tor(3, 0, active={1}, transitions=[(1, R.CLOSED)]), now=(1 << 62), duration=(1 << 62) - 1)
    return out


_cases = None


def cases():
    """Every case (built once a process)."""
    global _cases
    if _cases is None:
        _cases = _matrix() + named()
    return _cases


def case(label):
    return next(c for c in cases() if c.label == label)


# ------------------------------------------------------------------ the sweep
TTI, TTL = 100, 500


class SweepCase:
    """torrents: [(P, active set, created, received, sent)], three lists of P times each."""

    def __init__(self, label, torrents, now=NOW, tti=TTI, ttl=TTL):
        self.label, self.torrents, self.now, self.tti, self.ttl = label, torrents, now, tti, ttl
        k = len(torrents)
        bits, times, close_at = [CANARY64] * BASE, [[CANARY_I64] * BASE for _ in range(3)], BASE
        self.structs = (_capi.krk_conn_torrent * max(k, 1))()
        self.regions = []
        for t, (P, active, created, received, sent) in enumerate(torrents):
            self.structs[t] = _capi.krk_conn_torrent(P, R.NONE, 0, 0, len(bits), len(times[0]), close_at)
            self.regions.append((len(bits), close_at))
            bits += row_of(active, P, M64) + [CANARY64] * GAP  # a sweep reads the active row only
            for a, src in zip(times, (created, received, sent)):
                a += list(src) + [CANARY_I64] * GAP
            close_at += words(P) + GAP
        self.close_words = close_at
        self.bits = np.array(bits, dtype=np.uint64)
        self.times = [np.array(a, dtype=np.int64) for a in times]

    def want(self):
        """(close, n_close) whole buffers."""
        close = np.full(self.close_words, CANARY64, dtype=np.uint64)
        n_close = np.full(len(self.torrents) + GAP, CANARY32, dtype=np.uint32)
        for t, (P, active, created, received, sent) in enumerate(self.torrents):
            gone = R.preempt(P, active, created, received, sent, self.now, self.tti, self.ttl)
            at = self.regions[t][1]
            close[at:at + words(P)] = row_of(gone, P)
            n_close[t] = len(gone)
        return close, n_close

    def closed(self, t=0):
        P, active, created, received, sent = self.torrents[t]
        return R.preempt(P, active, created, received, sent, self.now, self.tti, self.ttl)


def sweeps():
    out = []
    # peer: (active, created, received, sent) at now = 1000, tti = 100, ttl = 500
    rows = [(1, 900, 0, 0),     # idle exactly tti: stays
            (1, 899, 0, 0),     # one past: closes
            (1, 500, 900, 0),   # the last good piece received is the most recent, at the threshold: stays
            (1, 500, 899, 0),   # ... one past: closes
            (1, 500, 0, 900),   # the last piece sent is the most recent: stays
            (1, 500, 10, 899),  # ... one past: closes
            (1, 500, 1000, 1000),  # created exactly ttl ago, busy: stays
            (1, 499, 1000, 1000),  # one past ttl, busy: closes
            (0, 1, 0, 0),       # inactive and ancient: never closed
            (0, 0, 0, 0),
            (1, 0, 0, 0),       # never anything: idle since 0
            (1, 1000, 0, 0),    # just created
            (1, 1001, -5, 2000)]  # the future and a negative time
    P = len(rows)
    out.append(SweepCase("the thresholds", [(P, {p for p, r in enumerate(rows) if r[0]}, [r[1] for r in rows],
                                             [r[2] for r in rows], [r[3] for r in rows])]))
    tors = []
    for P in (1, 63, 64, 65, 257, 4097):
        rng = Stream(77, P)
        tors.append((P, rng.subset(P, 2), [rng.below(1100) for _ in range(P)], [rng.below(1100) for _ in range(P)],
                     [rng.below(1100) for _ in range(P)]))
    out.append(SweepCase("six torrents at the word edges", tors))
    out.append(SweepCase("no peers", [(0, set(), [], [], []), (2, {0, 1}, [1, 950], [0, 0], [0, 0])]))
    return out


# ------------------------------------------------------------------ golden
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _sha(a, dtype):
    return hashlib.sha256(np.asarray(a, dtype=dtype).tobytes()).hexdigest()


def entry_of(c, got):
    """What the golden file records of a round's whole buffers: the bits and expiry as SHA-256 (little
    endian), the capacities, the statuses and the counts -- spelled out for the named cases, one
    SHA-256 of their JSON for the matrix."""
    bits, expiry, cap, ts, ins, ds, n_adm, n_freed = got
    k = len(c.torrents)
    e = {"bits": _sha(bits, "<u8"), "expiry": _sha(expiry, "<i8"), "capacity": [int(x) for x in cap[:k]],
         "transitions": [], "incoming": [], "dials": [], "admitted": [int(x) for x in n_adm[:2 * k]],
         "freed": [int(x) for x in n_freed[:k]]}
    for t, T in enumerate(c.torrents):
        off = c.regions[t][2]
        for name, a, o, n in (("transitions", ts, off[0], len(T.transitions)), ("incoming", ins, off[1], len(T.incoming)),
                              ("dials", ds, off[2], len(T.dials))):
            e[name].append([int(x) for x in a[o:o + n]])
    if c.label.startswith("matrix"):
        return hashlib.sha256(json.dumps(e, separators=(",", ":"), sort_keys=True).encode()).hexdigest()
    return e


def sweep_entry(c, got):
    close, n_close = got
    return {"close": [int(x) for x in close] if close.size < 40 else _sha(close, "<u8"),
            "n_close": [int(x) for x in n_close[:len(c.torrents)]]}


def golden_entry(c):
    return sweep_entry(c, c.want()) if isinstance(c, SweepCase) else entry_of(c, c.want())


# ------------------------------------------------------------------ backends
def prefilled(k):
    return np.full(k, CANARY32, dtype=np.uint32)


def round_args(c, bits, expiry, capacity, neighbors, outs):
    """The argument list of a round call over c (without the stream), the struct arrays copied so
    that a change leaves c alone.  bits ... outs: addresses."""
    structs = (_capi.krk_conn_torrent * len(c.structs))()
    lists = (_capi.krk_conn_lists * len(c.lists))()
    trans = (_capi.krk_conn_transition * len(c.transitions))()
    inc = (_capi.krk_conn_incoming * len(c.incoming))()
    for dst, src in ((structs, c.structs), (lists, c.lists), (trans, c.transitions), (inc, c.incoming)):
        C.memmove(dst, src, C.sizeof(src))
    dials = c.dials.copy()
    return [structs, lists, len(c.torrents), bits, expiry, capacity, trans, inc, dials.ctypes.data, neighbors,
            c.neighbors.size, c.now, c.duration, c.max_mutual, c.flags, *outs], dials


class HostBackend:
    """krk_conn_round and krk_conn_preempt: no device."""

    def run(self, c):
        state = [c.bits.copy(), c.expiry.copy(), c.capacity.copy()]
        outs = [prefilled(k) for k in c.out_sizes()]
        args, keep = round_args(c, *(a.ctypes.data for a in state), c.neighbors.ctypes.data, [o.ctypes.data for o in outs])
        check(lib.krk_conn_round(*args))
        return (*state, *outs)

    def sweep(self, c):
        close, n_close = c.want()
        close[:], n_close[:] = CANARY64, CANARY32
        check(lib.krk_conn_preempt(c.structs, len(c.torrents), c.bits.ctypes.data, *(a.ctypes.data for a in c.times), c.now,
                                   c.tti, c.ttl, close.ctypes.data, n_close.ctypes.data))
        return close, n_close


class DeviceBackend:
    """krk_conn_round_dev and krk_conn_preempt_dev: the state uploaded a call, the outputs in device
    memory or, with pinned, in krk_host_alloc memory."""

    def __init__(self):
        from kraken_amd import device as D
        self.D = D

    def upload(self, a):
        b = self.D.DeviceBuffer(a.nbytes)
        b.from_host(a)
        return b

    def run(self, c, pinned=False, stream=None):
        D = self.D
        state = [self.upload(a) for a in (c.bits, c.expiry, c.capacity)]
        neigh = self.upload(c.neighbors)
        sizes = c.out_sizes()
        outs = [D.PinnedArray((k,), np.uint32) if pinned else D.DeviceBuffer(4 * k) for k in sizes]
        for o, k in zip(outs, sizes):
            if pinned:
                o.a[:] = CANARY32
            else:
                o.from_host(prefilled(k))
        args, keep = round_args(c, *(b.ptr for b in state), neigh.ptr, [o.ptr for o in outs])
        check(lib.krk_conn_round_dev(*args, stream))
        check(lib.krk_stream_sync(stream))
        got = [o.a.copy() if pinned else o.to_host(np.uint32, k) for o, k in zip(outs, sizes)]
        return (state[0].to_host(np.uint64, c.bits.size), state[1].to_host(np.int64, c.expiry.size),
                state[2].to_host(np.uint32, c.capacity.size), *got)

    def sweep(self, c, stream=None):
        want = c.want()
        bits = self.upload(c.bits)
        times = [self.upload(a) for a in c.times]
        close, n_close = self.upload(np.full_like(want[0], CANARY64)), self.upload(np.full_like(want[1], CANARY32))
        check(lib.krk_conn_preempt_dev(c.structs, len(c.torrents), bits.ptr, *(a.ptr for a in times), c.now, c.tti, c.ttl,
                                       close.ptr, n_close.ptr, stream))
        check(lib.krk_stream_sync(stream))
        return close.to_host(np.uint64, want[0].size), n_close.to_host(np.uint32, want[1].size)


# ------------------------------------------------------------------ comparison
NAMES = ("bits", "expiry", "capacity", "trans_status", "in_status", "dial_status", "n_admitted", "n_freed")


def compare(c, got, want=None, names=NAMES):
    """Mismatches of one call's whole buffers against the restatement's (or `want`), as text."""
    bad = []
    for name, g, w in zip(names, got, want or c.want()):
        if not np.array_equal(g, w):
            k = int(np.flatnonzero(g != w)[0])
            bad.append(f"{c.label}: {name}[{k}] is {int(g[k]):#x}, want {int(w[k]):#x} ({int((g != w).sum())} differ)")
    return bad


def run_cases(backend, some, **kw):
    bad = []
    for c in some:
        bad += compare(c, backend.run(c, **kw))
    return len(some), bad


def run_sweeps(backend, some, **kw):
    bad = []
    for c in some:
        bad += compare(c, backend.sweep(c, **kw), names=("close", "n_close"))
    return len(some), bad


# ------------------------------------------------------------------ refusals
# round_args' positions
A_TORRENTS, A_LISTS, A_N, A_BITS, A_EXPIRY, A_CAPACITY, A_TRANS, A_IN, A_DIALS, A_NEIGH, A_NWORDS, A_NOW, A_DUR, A_MM, \
    A_FLAGS, A_OUT = range(16)


def refusal_case():
    return Case("refusals", [Tor(65, 3, self_peer=64, active={1}, pending={2}, expiry={3: NOW + 1},
                                 transitions=[(1, R.CLOSED), (2, R.ESTABLISHED)], incoming=[(5, {1, 2}), (6, None)],
                                 dials=[7, 8, 3]),
                             Tor(130, 1, pending={129}, transitions=[(129, R.FAILED_OUT)], incoming=[(0, {129})], dials=[64])])


def invalid_calls():
    """[(label, change, rc)]: change(args, dials) edits the argument list of a valid round call over
    refusal_case() into one that is refused with rc."""
    E, ER = _capi.KRK_EINVAL, _capi.KRK_ERANGE

    def field(arr, j, name, v):
        def change(a, dials):
            setattr(a[arr][j], name, v)
        return change

    def arg(k, v):
        def change(a, dials):
            a[k] = v
        return change

    def dial(j, v):
        def change(a, dials):
            dials[j] = v
        return change

    first_tr, first_in, first_dial = BASE, BASE, BASE  # torrent 0's first entries
    out = [("P = 2^30", field(A_TORRENTS, 1, "n_peers", 1 << 30), E),
           ("self_peer = P", field(A_TORRENTS, 0, "self_peer", 65), E),
           ("self_peer = NONE - 1", field(A_TORRENTS, 1, "self_peer", R.NONE - 1), E),
           ("unknown torrent flag", field(A_TORRENTS, 0, "flags", 2), E),
           ("torrent reserved set", field(A_TORRENTS, 1, "reserved", 1), E),
           ("bits_off = 2^48", field(A_TORRENTS, 0, "bits_off", 1 << 48), E),
           ("peer_off = 2^48", field(A_TORRENTS, 1, "peer_off", 1 << 48), E),
           ("trans_off = 2^48", field(A_LISTS, 0, "trans_off", 1 << 48), E),
           ("in_off = 2^48", field(A_LISTS, 0, "in_off", 1 << 48), E),
           ("dial_off = 2^48", field(A_LISTS, 1, "dial_off", 1 << 48), E),
           ("2^32 transitions", field(A_LISTS, 0, "n_trans", 1 << 32), ER),
           ("2^32 incoming", field(A_LISTS, 1, "n_in", 1 << 32), ER),
           ("2^32 dials", field(A_LISTS, 0, "n_dial", 1 << 32), ER),
           ("transition peer = P", field(A_TRANS, first_tr + 1, "peer", 65), E),
           ("unknown kind", field(A_TRANS, first_tr, "kind", 4), E),
           ("transitions descend", field(A_TRANS, first_tr + 1, "peer", 0), E),
           ("transitions repeat", field(A_TRANS, first_tr + 1, "peer", 1), E),
           ("incoming peer = P", field(A_IN, first_in, "peer", 65), E),
           ("incoming reserved set", field(A_IN, first_in + 1, "reserved", 7), E),
           ("a neighbour row past the end", arg(A_NWORDS, BASE + 1), E),
           ("neigh_off = 2^48", field(A_IN, first_in, "neigh_off", 1 << 48), E),
           ("dial peer = P", dial(first_dial + 2, 65), E),
           ("now < 0", arg(A_NOW, -1), E), ("blacklist_duration < 0", arg(A_DUR, -1), E),
           ("now + blacklist_duration past INT64_MAX", arg(A_NOW, (1 << 63) - DURATION), E),
           ("unknown round flag", arg(A_FLAGS, 2), E)]
    out += [(f"NULL argument {k}", arg(k, None), E) for k in (A_TORRENTS, A_LISTS, A_BITS, A_EXPIRY, A_CAPACITY, A_TRANS, A_IN,
                                                                A_DIALS, A_NEIGH, A_OUT, A_OUT + 1, A_OUT + 2, A_OUT + 3,
                                                                A_OUT + 4)]
    return out


if __name__ == "__main__":
    import sys
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python -m tests.conn_matrix --write")
    every = cases() + sweeps()
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(c.label)}:{json.dumps(golden_entry(c), separators=(',', ':'))}"
                                   for c in every) + "\n}\n")
    print(f"{GOLDEN}: {len(every)} cases, {os.path.getsize(GOLDEN)} bytes")
