"""Announce rounds (announce_round.hip, announce_math.hpp) at the kernel's word, lane-stride, window
and limit edges: the cases, their expectations and the comparison, shared by
tests/test_gpu_announce_matrix.py and tests/test_gpu_announce_round.py (krk_announce_round_dev on
the production library) and tests/test_announce_matrix_cpu.py (krk_announce_round and
krk_announce_handout, the host forms the kernel is documented to equal).  A helper module, not a
test file.

A case is one ROUND: torrents, their peer stores, announces, a limit and a policy.  Its inputs come
from a splitmix64 stream written out here (no library, no numpy generator), its expectation is
tests/announce_ref.py's restatement, never the library, and tests/golden/announce_rounds.json
records that expectation (`python -m tests.announce_matrix --write` regenerates it).  The bits
array starts at a non-zero offset (BASE) and carries SPARE words past its end; the outputs are
prefilled with 0xA5 bytes, so a case's expected output is the whole buffers: every owned element
stored, nothing else touched.

 matrix   P in {1, 63, 64, 65, 4097} x limit in {1, 50, 64} x W in {1, 5, 8}, a non-zero cur_row
          wherever W > 1, O cycling through {0, 3, 8}, the policy alternating; the windows cycle
          through empty, sparse, half, all ones (tail bits and complete rows garbage included);
          announces with the source KRK_AN_NONE, a sampled peer and an unsampled one, one complete
          announcer, and one (torrent, peer) announced twice
 named    one property each (see named())
 batches  A = 1 and A = 257 over three torrents"""
import ctypes as C
import hashlib
import json
import os

import numpy as np

from kraken_amd import _capi
from kraken_amd._capi import check, lib
from tests import announce_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "announce_rounds.json")
SEED = 20261021
BASE, SPARE = 3, 4
CANARY32 = np.uint32(0xA5A5A5A5)
CANARY64 = 0x5A5A5A5A5A5A5A5A
u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
NONE, ORIGIN, CBIT = R.NONE, R.ORIGIN, R.COMPLETE_BIT
DEFAULT, COMPLETENESS, COMPLETE = R.DEFAULT, R.COMPLETENESS, R.COMPLETE
assert (NONE, ORIGIN, CBIT, DEFAULT, COMPLETENESS, COMPLETE) == (
    _capi.KRK_AN_NONE, _capi.KRK_AN_ORIGIN, _capi.KRK_AN_COMPLETE_BIT, _capi.KRK_AN_DEFAULT, _capi.KRK_AN_COMPLETENESS,
    _capi.KRK_AN_COMPLETE)
assert (R.MAX_WINDOWS, R.MAX_ORIGINS, R.MAX_LIMIT) == (_capi.KRK_AN_MAX_WINDOWS, _capi.KRK_AN_MAX_ORIGINS,
                                                       _capi.KRK_AN_MAX_LIMIT)
PS = (1, 63, 64, 65, 4097)
LIMITS = (1, 50, 64)
WS = (1, 5, 8)
OS = (0, 3, 8)
M64 = (1 << 64) - 1


class Stream:
    """A splitmix64 stream: the cases' only source of inputs."""

    def __init__(self, *salt):
        self.s = SEED
        for v in salt:
            self.s = R.splitmix64(self.s ^ (int(v) & M64))

    def word(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & M64
        return R.splitmix64(self.s)

    def below(self, n):
        return self.word() % n


def row_words(rng, p, mode):
    """One row of words(p) words: "empty", "sparse" (1 bit in 16), "half", "ones" (every bit, the
    tail past p included)."""
    n = R.words(p)
    if mode == "empty":
        return [0] * n
    if mode == "ones":
        return [M64] * n
    if mode == "sparse":
        return [rng.word() & rng.word() & rng.word() & rng.word() for _ in range(n)]
    return [rng.word() for _ in range(n)]


class Case:
    """torrents: [(P, W, cur_row, O, [mode a window] or [(member set, complete set) a window])];
    announces: [(torrent, peer, flags, source, seed)] with source an index, NONE, "sampled" or
    "unsampled" (resolved with the restatement: the first store peer of the handout the announce gets
    with no source / the lowest index it does not get)."""

    def __init__(self, label, torrents, announces, limit, policy):
        self.label, self.limit, self.policy = label, int(limit), int(policy)
        rng = Stream(*label.encode())
        self.torrents, off, words = [], BASE, [CANARY64] * BASE
        for p, w, cur, o, windows in torrents:
            self.torrents.append((p, w, cur, o, off))
            rows = [None] * (2 * w)
            for k, win in enumerate(windows):  # window k is ring row (cur + k) % w
                r = (cur + k) % w
                if isinstance(win, str):
                    rows[2 * r] = row_words(rng, p, win)
                    rows[2 * r + 1] = row_words(rng, p, "ones" if win == "ones" else "half")  # garbage where no member is
                else:
                    rows[2 * r] = [sum(1 << (i % 64) for i in win[0] if i // 64 == x) for x in range(R.words(p))]
                    rows[2 * r + 1] = [sum(1 << (i % 64) for i in win[1] if i // 64 == x) for x in range(R.words(p))]
            for row in rows:
                words += row
            off += 2 * w * R.words(p)
        words += [CANARY64] * SPARE
        self.bits = np.array(words, dtype=np.uint64)
        self.bits.setflags(write=False)
        plain = [(t, peer, flags, NONE if isinstance(src, str) else src, seed) for t, peer, flags, src, seed in announces]
        if any(isinstance(a[3], str) for a in announces):
            _, hand, _ = R.announce_round(self.torrents, words, plain, self.limit, self.policy)
            for k, a in enumerate(announces):
                if isinstance(a[3], str):
                    got = [c & ~CBIT for c in hand[k] if not c & ORIGIN]
                    pick = got[0] if a[3] == "sampled" and got else \
                        next((i for i in range(self.torrents[a[0]][0]) if i not in got), NONE)
                    plain[k] = plain[k][:3] + (pick,) + plain[k][4:]
        self.announces = plain
        self.structs = (_capi.krk_announce_torrent * max(len(self.torrents), 1))()
        for k, (p, w, cur, o, at) in enumerate(self.torrents):
            self.structs[k] = _capi.krk_announce_torrent(p, w, cur, o, 0, at)
        self.anns = (_capi.krk_announce * max(len(plain), 1))()
        for k, a in enumerate(plain):
            self.anns[k] = _capi.krk_announce(*a)
        self.cap = self.limit + R.MAX_ORIGINS
        self._want = None

    def sizes(self):
        """Elements of (handout, n_out, labels)."""
        a = len(self.announces)
        return a * self.cap + SPARE, a + SPARE, 3 * a + SPARE

    def ref(self):
        """The restatement's (bits, handouts, labels): lists."""
        if self._want is None:
            self._want = R.announce_round(self.torrents, self.bits.tolist(), self.announces, self.limit, self.policy)
        return self._want

    def want(self):
        """The whole buffers after the call: (bits, handout, n_out, labels), canaries where nobody owns."""
        bits, hands, labels = self.ref()
        handout, n_out, lab = (np.full(k, CANARY32, dtype=np.uint32) for k in self.sizes())
        a = len(self.announces)
        handout[:a * self.cap] = NONE
        for k, h in enumerate(hands):
            handout[k * self.cap:k * self.cap + len(h)] = h
            n_out[k] = len(h)
            lab[3 * k:3 * k + 3] = labels[k]
        return np.array(bits, dtype=np.uint64), handout, n_out, lab


def _matrix():
    out, k = [], 0
    for p in PS:
        for limit in LIMITS:
            for w in WS:
                cur = (w - 1, 2, 3)[k % 3] % w if w > 1 else 0
                modes = [("half", "empty", "sparse", "ones")[(j + k) % 4] for j in range(w)]
                rng = Stream(p, limit, w)
                peers = [rng.below(p) for _ in range(4)]
                anns = [(0, peers[0], 0, NONE, rng.word()), (0, peers[1], 0, "sampled", rng.word()),
                        (0, peers[2], 0, "unsampled", rng.word()), (0, peers[3], COMPLETE, NONE, rng.word()),
                        (0, peers[0], COMPLETE if k % 2 else 0, peers[0], rng.word())]
                out.append(Case(f"matrix P={p} limit={limit} W={w} cur={cur} O={OS[k % 3]} policy={k % 2}",
                                [(p, w, cur, OS[k % 3], modes)], anns, limit, k % 2))
                k += 1
    return out


def named():
    """One property a case."""
    s = lambda *a: (set(a[0]), set(a[1]) if len(a) > 1 else set())  # noqa: E731
    out = []

    def add(label, torrents, announces, limit, policy=COMPLETENESS):
        out.append(Case(label, torrents, announces, limit, policy))

    # whichever window comes first, the second holds exactly `need` members
    add("a window of exactly need members", [(200, 2, 1, 0, [s(range(0, 4), [1]), s(range(100, 106), [101])])],
        [(0, 199, 0, NONE, seed) for seed in (1, 2, 3, 4)], 11)
    add("a window all of whose members are already selected",
        [(130, 3, 2, 3, [s([5, 64, 129], [5]), s([5, 64, 129], [64]), s([7, 8], [])])],
        [(0, 7, 0, NONE, seed) for seed in (11, 12, 13, 14, 15, 16)], 50)
    add("complete bits collapse across windows", [(65, 5, 3, 0, [s([1, 64]), s([1], [1]), s([64]), s([], [64]), s([2], [2])])],
        [(0, 0, 0, 0, 21)], 64)
    for p in (63, 64, 65):  # every word of every row all ones: the tail is never sampled
        add(f"all ones P={p}", [(p, 2, 1, 3, ["ones", "ones"])], [(0, p - 1, 0, NONE, 31), (0, 0, 0, "sampled", 32)], 64)
    add("all ones, more than one stride of words", [(4097, 1, 0, 8, ["ones"])],
        [(0, 4096, 0, "sampled", 41), (0, 0, 0, NONE, 42)], 64, DEFAULT)
    add("empty windows but one", [(300, 5, 1, 3, ["empty", "empty", "empty", "sparse", "empty"])],
        [(0, 17, 0, 17, 51), (0, 18, 0, NONE, 52)], 50)
    add("nobody but the announcer, no origins", [(65, 8, 5, 0, ["empty"] * 8)],
        [(0, 64, 0, 64, 61), (0, 64, 0, NONE, 62)], 50)
    add("one (torrent, peer) twice, once complete", [(64, 1, 0, 3, ["sparse"])],
        [(0, 63, 0, NONE, 71), (0, 63, COMPLETE, NONE, 72), (0, 0, 0, NONE, 73)], 64)
    add("the default policy: one class", [(100, 5, 4, 8, ["half"] * 5)], [(0, 3, 0, "sampled", 81), (0, 4, 0, NONE, 82)], 50,
        DEFAULT)
    # TestCompletenessPriorityPolicy: 10 seeders, 3 origins, 20 incomplete peers, in that order
    add("completeness_policy_test.go", [(31, 1, 0, 3, [s(range(30), range(10))])], [(0, 30, 0, 30, 91)], 50)
    # TestPriorityPolicyRemoveSource: ten peers and the source
    add("peerhandoutpolicy_test.go remove source", [(11, 1, 0, 0, [s(range(10))])], [(0, 10, 0, 10, 92)], 50, DEFAULT)
    return out


def batches():
    """A = 1 and A = 257 over three torrents (one of them of one peer)."""
    tors = [(65, 5, 2, 3, ["half", "sparse", "empty", "half", "ones"]), (1, 1, 0, 0, ["empty"]),
            (130, 8, 7, 8, ["sparse"] * 4 + ["half"] * 4)]
    rng = Stream(257)
    anns = []
    for k in range(257):
        t = k % 3
        p = rng.below(tors[t][0])
        anns.append((t, p, COMPLETE if k % 7 == 3 else 0, (NONE, p, rng.below(tors[t][0]))[k % 3], rng.word()))
    return [Case("A=1 over three torrents", tors, [(2, 129, 0, 129, 5)], 50, COMPLETENESS),
            Case("A=257 over three torrents", tors, anns, 50, COMPLETENESS)]


_cases = None


def cases():
    """Every case (built once a process)."""
    global _cases
    if _cases is None:
        _cases = _matrix() + named() + batches()
    return _cases


def case(label):
    return next(c for c in cases() if c.label == label)


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def entry_of(c, bits, hands, labels):
    """What the golden file records of a round's results: the sources as resolved, the updated
    words as a SHA-256 (little endian, the whole buffer), the handouts and the label counts --
    spelled out for the named cases, one SHA-256 of their JSON for the matrix and the 257-announce
    batch."""
    e = {"sources": [a[3] for a in c.announces], "bits": hashlib.sha256(np.asarray(bits, dtype="<u8").tobytes()).hexdigest(),
         "handouts": hands, "labels": labels}
    if c.label.startswith(("matrix", "A=257")):
        return hashlib.sha256(json.dumps(e, separators=(",", ":"), sort_keys=True).encode()).hexdigest()
    return e


def golden_entry(c):
    return entry_of(c, *c.ref())


def got_entry(c, got):
    """entry_of a backend's whole buffers."""
    bits, handout, n_out, labels = got
    a = len(c.announces)
    return entry_of(c, bits, [handout[k * c.cap:k * c.cap + int(n_out[k])].tolist() for k in range(a)],
                    labels[:3 * a].reshape(a, 3).tolist())


# ------------------------------------------------------------------ backends
def prefilled(k):
    return np.full(k, CANARY32, dtype=np.uint32)


class HostBackend:
    """krk_announce_round: no device."""

    def run(self, c):
        bits = c.bits.copy()
        outs = [prefilled(k) for k in c.sizes()]
        check(lib.krk_announce_round(c.structs, len(c.torrents), bits.ctypes.data_as(u64p), c.anns, len(c.announces),
                                     c.limit, c.policy, *(o.ctypes.data_as(u32p) for o in outs)))
        return (bits, *outs)


class HandoutBackend:
    """krk_announce_handout, announce by announce, over rows the restatement updated."""

    def run(self, c):
        bits = c.want()[0]
        outs = [prefilled(k) for k in c.sizes()]
        for k in range(len(c.announces)):
            check(lib.krk_announce_handout(c.structs, len(c.torrents), bits.ctypes.data_as(u64p), C.byref(c.anns[k]), c.limit,
                                           c.policy, outs[0][k * c.cap:].ctypes.data_as(u32p),
                                           outs[1][k:].ctypes.data_as(u32p), outs[2][3 * k:].ctypes.data_as(u32p)))
        return (bits, *outs)


class DeviceBackend:
    """krk_announce_round_dev: the bits uploaded a call, the outputs in device memory or, with
    pinned, in krk_host_alloc memory."""

    def __init__(self):
        from kraken_amd import device as D
        self.D = D

    def run(self, c, pinned=False, stream=None):
        D = self.D
        bits = D.DeviceBuffer(c.bits.nbytes)
        bits.from_host(c.bits)
        outs = [D.PinnedArray((k,), np.uint32) if pinned else D.DeviceBuffer(4 * k) for k in c.sizes()]
        for o, k in zip(outs, c.sizes()):
            if pinned:
                o.a[:] = CANARY32
            else:
                o.from_host(prefilled(k))
        check(lib.krk_announce_round_dev(c.structs, len(c.torrents), bits.ptr, c.anns, len(c.announces), c.limit, c.policy,
                                         *(o.ptr for o in outs), stream))
        check(lib.krk_stream_sync(stream))
        got = [o.a.copy() if pinned else o.to_host(np.uint32, k) for o, k in zip(outs, c.sizes())]
        return (bits.to_host(np.uint64, c.bits.size), *got)


# ------------------------------------------------------------------ comparison
def compare(c, got, want=None):
    """Mismatches of one call's whole buffers against the restatement's (or `want`), as text."""
    bad = []
    for name, g, w in zip(("bits", "handout", "n_out", "labels"), got, want or c.want()):
        if not np.array_equal(g, w):
            k = int(np.flatnonzero(g != w)[0])
            bad.append(f"{c.label}: {name}[{k}] is {int(g[k]):#x}, want {int(w[k]):#x} ({int((g != w).sum())} differ)")
    return bad


def run_cases(backend, some, **kw):
    bad = []
    for c in some:
        bad += compare(c, backend.run(c, **kw))
    return len(some), bad


# ------------------------------------------------------------------ refusals
def invalid_calls():
    """[(label, change)]: change(args) edits the argument list of a valid krk_announce_round call
    over refusal_case() -- args[0] a copy of the torrents, args[3] of the announces -- into one that
    is KRK_EINVAL."""
    def field(arr, j, name, v):
        def change(a):
            setattr(a[arr][j], name, v)
        return change

    def arg(k, v):
        def change(a):
            a[k] = v
        return change

    out = [("P = 2^30", field(0, 1, "n_peers", 1 << 30)),
           ("W = 0", field(0, 0, "n_windows", 0)),
           ("W = 9", field(0, 1, "n_windows", 9)),
           ("O = 9", field(0, 0, "n_origins", 9)),
           ("cur_row = W", field(0, 1, "cur_row", 5)),
           ("reserved set", field(0, 0, "reserved", 1)),
           ("torrent = n_torrents", field(3, 1, "torrent", 2)),
           ("peer = P", field(3, 0, "peer", 65)),
           ("source = P", field(3, 1, "source", 130)),
           ("source = NONE - 1", field(3, 0, "source", NONE - 1)),
           ("unknown flag bit", field(3, 1, "flags", 2)),
           ("unknown flag bit beside the known one", field(3, 0, "flags", COMPLETE | 0x80000000)),
           ("limit 0", arg(5, 0)), ("limit 65", arg(5, 65)), ("policy 2", arg(6, 2))]
    out += [(f"NULL argument {k}", arg(k, None)) for k in (0, 2, 3, 7, 8, 9)]
    return out


def refusal_case():
    return Case("refusals", [(65, 2, 1, 3, ["half", "sparse"]), (130, 5, 4, 0, ["half"] * 5)],
                [(0, 64, 0, NONE, 1), (1, 129, COMPLETE, 3, 2), (1, 0, 0, 0, 3)], 50, COMPLETENESS)


def call_args(c, bits, outs):
    """The argument list of a round call over c (without the stream), its arrays copied so that a
    change leaves c alone.  bits / outs: pointers."""
    structs = (_capi.krk_announce_torrent * len(c.structs))()
    anns = (_capi.krk_announce * len(c.anns))()
    for dst, src in ((structs, c.structs), (anns, c.anns)):
        C.memmove(dst, src, C.sizeof(src))
    return [structs, len(c.torrents), bits, anns, len(c.announces), c.limit, c.policy, *outs]


if __name__ == "__main__":
    import sys
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python -m tests.announce_matrix --write")
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(c.label)}:{json.dumps(golden_entry(c), separators=(',', ':'))}"
                                   for c in cases()) + "\n}\n")
    print(f"{GOLDEN}: {len(cases())} cases, {os.path.getsize(GOLDEN)} bytes")
