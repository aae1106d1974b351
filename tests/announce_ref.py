"""A restatement of the announce round's semantics (include/kraken_hip.h, "announce rounds") in
plain Python sets and `sorted`: what the tracker's announce does -- UpdatePeer, GetPeers over the
peer-set windows, the origins appended, SortPeers -- with the reference's random choices replaced
by the header's seeded keys.  It shares no code with the library (no numpy, no ctypes): the
expectation of tests/announce_matrix.py's cases and the generator of
tests/golden/announce_rounds.json.  A helper module, not a test file."""

MAX_WINDOWS, MAX_ORIGINS, MAX_LIMIT = 8, 8, 64
DEFAULT, COMPLETENESS = 0, 1
COMPLETE = 1
NONE, ORIGIN, COMPLETE_BIT = 0xFFFFFFFF, 0x80000000, 0x40000000
M64 = (1 << 64) - 1


def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def wkey(seed, w):
    return splitmix64(seed ^ ((w + 1) << 32 | 0xFFFFFFFF)) >> 32


def pkey(seed, w, i):
    return splitmix64(seed ^ ((w + 1) << 32 | i)) >> 32


def okey(seed, c):
    return splitmix64(seed ^ c) >> 32


def words(p):
    return (p + 63) // 64


class Torrent:
    """A peer store as sets: .member[w] / .complete[w] for window w (0 = current), of peers < P."""

    def __init__(self, n_peers, n_windows, cur_row, n_origins, bits_off):
        self.P, self.W, self.cur_row, self.O, self.bits_off = n_peers, n_windows, cur_row, n_origins, bits_off
        self.member = [set() for _ in range(n_windows)]
        self.complete = [set() for _ in range(n_windows)]

    def row(self, w):
        """First word of window w's member row; its complete row follows words(P) later."""
        return self.bits_off + 2 * ((self.cur_row + w) % self.W) * words(self.P)

    def load(self, bits):
        """The sets from a list of 64-bit words; bits past P are not peers."""
        for w in range(self.W):
            for dst, at in ((self.member[w], self.row(w)), (self.complete[w], self.row(w) + words(self.P))):
                dst.clear()
                for x in range(words(self.P)):
                    v = int(bits[at + x])
                    while v:
                        b = v & -v
                        i = 64 * x + b.bit_length() - 1
                        if i < self.P:
                            dst.add(i)
                        v ^= b

    def update(self, bits, peer, complete):
        """UpdatePeer: the sets and the words."""
        at = self.row(0)
        self.member[0].add(peer)
        bits[at + peer // 64] = int(bits[at + peer // 64]) | 1 << (peer % 64)
        if complete:
            at += words(self.P)
            self.complete[0].add(peer)
            bits[at + peer // 64] = int(bits[at + peer // 64]) | 1 << (peer % 64)


def handout(t, peer, flags, source, seed, limit, policy):
    """One announce over the sets of t: ([c | COMPLETE_BIT ...], [three label counts])."""
    if flags & COMPLETE:
        return [], [0, 0, 0]
    selected = {}  # peer -> complete
    for w in sorted(range(t.W), key=lambda w: (wkey(seed, w), w)):
        if len(selected) >= limit:
            break
        need = limit - len(selected)
        for i in sorted(t.member[w], key=lambda i: (pkey(seed, w, i), i))[:need]:
            selected[i] = selected.get(i, False) or (i in t.complete[w])
    entries = [(i, False, c) for i, c in selected.items() if i != source]
    entries += [(ORIGIN | o, True, True) for o in range(t.O)]

    def prio(e):
        c, origin, complete = e
        if policy != COMPLETENESS:
            return 0
        return 1 if origin else (0 if complete else 2)

    entries.sort(key=lambda e: (prio(e), okey(seed, e[0]), e[0]))
    labels = [0, 0, 0]
    for e in entries:
        labels[prio(e)] += 1
    return [c | (COMPLETE_BIT if complete and not origin else 0) for c, origin, complete in entries], labels


def announce_round(torrents, bits, announces, limit, policy):
    """torrents: [(n_peers, n_windows, cur_row, n_origins, bits_off)]; bits: 64-bit words;
    announces: [(torrent, peer, flags, source, seed)].  Returns (the updated words as a list,
    [handout a announce, n_out entries each], [labels a announce])."""
    bits = [int(v) for v in bits]
    ts = [Torrent(*t) for t in torrents]
    for t in ts:
        t.load(bits)
    for k, peer, flags, _, _ in announces:
        ts[k].update(bits, peer, bool(flags & COMPLETE))
    outs = [handout(ts[k], peer, flags, source, seed, limit, policy) for k, peer, flags, source, seed in announces]
    return bits, [o[0] for o in outs], [o[1] for o in outs]
