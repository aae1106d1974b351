"""Resend rounds (piece_resend.hip, piece_resend_math.hpp) at the kernel's pass, word and launch
edges: the cases, their expectations and the comparison, shared by
tests/test_gpu_piece_resend_matrix.py (krk_piece_resend_round_dev on the production library) and
tests/test_piece_resend_matrix_cpu.py (krk_piece_resend_round, the host form the kernel is
documented to equal).  A helper module, not a test file.

S (the peers one workgroup pass covers, one peer a thread) is read from the built library
(krk_piece_resend_geometry).  A case is a BATCH of torrents; a torrent's expectation is
tests/piece_resend_ref.py's restatement, never the library, and the named cases carry the targets
worked out by hand as well.  Every array of a batch starts at a non-zero offset (BASE) and carries
SPARE entries past its end; the outputs are prefilled with 0xA5 bytes, so a batch's expected
output is the whole buffer: every owned element stored, nothing else touched.

 random   have 1/4, blocked 1/8, the peers' bitfields at a density that puts the first eligible
          peer now in the first pass and now in a later one; the peers' tail bits all set; the
          failed list random pieces (repeats included), peers (KRK_PR_NONE included) and statuses
 named    one property each, built from a sparse description (see named())"""
import ctypes as C

import numpy as np

from kraken_amd import _capi
from kraken_amd._capi import check, lib
from tests import piece_resend_ref as R

SEED = 20261021
SPARE = 4
CANARY32 = np.uint32(0xA5A5A5A5)
BASE = (3, 5, 7)  # the first word, peer and failed entry a batch uses
u32p, u64p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
failedp = C.POINTER(_capi.krk_failed_request)
DUP, NONE = R.ALLOW_DUPLICATES, R.NONE
EXPIRED, UNSENT, INVALID = R.EXPIRED, R.UNSENT, R.INVALID
assert (EXPIRED, UNSENT, INVALID, NONE) == (_capi.KRK_PR_EXPIRED, _capi.KRK_PR_UNSENT, _capi.KRK_PR_INVALID,
                                            _capi.KRK_PR_NONE)


def geometry():
    s = C.c_uint64()
    check(lib.krk_piece_resend_geometry(C.byref(s)))
    return int(s.value)


S = geometry()
PS = (0, 1, 2, S - 1, S, S + 1, 2 * S + 1)
NS = (1, 63, 64, 65, 4097)
FS = (0, 1, 2, 300)


def words(n):
    return (n + 63) // 64


def pack(b):
    p = np.packbits(np.asarray(b, dtype=bool), bitorder="little")
    return np.concatenate([p, np.zeros(-p.size % 8, dtype=np.uint8)]).view(np.uint64)


def tail(n):
    """The last word's bits past n, as a word (0 when n is a multiple of 64)."""
    return np.uint64(((1 << 64) - 1) ^ ((1 << (n % 64)) - 1)) if n % 64 else np.uint64(0)


class Torrent:
    """rows: (1 + 2 n_peers, words(n)) uint64; failed: [(piece, peer or NONE, status)] ascending by piece."""

    def __init__(self, label, n, n_peers, flags, rows, quota, failed):
        self.label, self.n, self.n_peers, self.flags = label, int(n), int(n_peers), int(flags)
        self.rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(1 + 2 * n_peers, words(n))
        self.rows.setflags(write=False)
        self.quota = np.asarray(quota, dtype=np.int32).reshape(n_peers)
        self.failed = [tuple(int(x) for x in f) for f in failed]
        self._want = None

    def want(self):
        if self._want is None:
            self._want = R.resend_torrent(self.rows, self.n, self.n_peers, self.flags, self.quota, self.failed)
        return self._want


def random_torrent(n, n_peers, n_failed, flags, salt=0):
    rng = np.random.default_rng([SEED, n, n_peers, n_failed, flags, salt])
    W = words(n)
    rows = np.zeros((1 + 2 * n_peers, W), dtype=np.uint64)
    rows[0] = pack(rng.random(n) < 0.25)
    # about one holder a pass at the low density: the first eligible peer is often past the first pass
    density = (0.5, 1.5 / max(min(n_peers, S), 1))[salt % 2] if n_peers > 2 else 0.6
    for p in range(n_peers):
        rows[1 + 2 * p] = pack(rng.random(n) < density)
        rows[2 + 2 * p] = pack(rng.random(n) < 0.125)
    rows[1::2, -1] |= tail(n)  # the peers' tail bits set
    quota = rng.choice([-1, 0, 1, 2, 3, 40], size=n_peers)
    pieces = np.sort(rng.integers(0, n, size=n_failed))
    if n_failed > 2:  # runs of one piece
        pieces[1::3] = pieces[0:-1:3][:pieces[1::3].size]
        pieces = np.sort(pieces)
    peers = rng.integers(0, n_peers + 1, size=n_failed)
    failed = [(int(i), NONE if p == n_peers or not n_peers else int(p), int(s))
              for i, p, s in zip(pieces, peers, rng.integers(1, 4, size=n_failed))]
    return Torrent(f"random n={n} P={n_peers} F={n_failed} flags={flags:#x} salt={salt}", n, n_peers, flags, rows,
                   quota, failed)


def sparse(label, n, n_peers, failed, holders, quota=None, have=(), blocked=None, flags=0, ones=False):
    """holders / blocked: {peer: pieces}; have: pieces; quota: a list, or one value for every peer (default 1)."""
    bits = np.zeros((1 + 2 * n_peers, n), dtype=bool)
    bits[0, list(have)] = True
    for p, pieces in holders.items():
        bits[1 + 2 * p, list(pieces)] = True
    for p, pieces in (blocked or {}).items():
        bits[2 + 2 * p, list(pieces)] = True
    rows = np.stack([pack(r) for r in bits])
    if ones:
        rows[:] = np.uint64((1 << 64) - 1)
    q = np.full(n_peers, 1 if quota is None else quota, dtype=np.int32) if np.ndim(quota) == 0 else quota
    return Torrent(label, n, n_peers, flags, rows, q, failed)


class Batch:
    """Torrents packed back to back from BASE, in the order given."""

    def __init__(self, torrents, label=None):
        self.torrents = list(torrents)
        self.label = label or " | ".join(t.label for t in self.torrents)
        k = len(self.torrents)
        self.structs = (_capi.krk_request_torrent * max(k, 1))()
        self.resends = (_capi.krk_resend_torrent * max(k, 1))()
        w, p, f = BASE
        self.offs = []
        for j, t in enumerate(self.torrents):
            self.offs.append((w, p, f))
            # the policy bits, the seed and piece_off are not read: arbitrary values
            self.structs[j] = _capi.krk_request_torrent(t.n, t.n_peers, t.flags | (j & 1), 0x1234567 * j, w, p, 1 << 40)
            self.resends[j] = _capi.krk_resend_torrent(f, len(t.failed))
            w, p, f = w + t.rows.size, p + t.n_peers, f + len(t.failed)
        self.n_words, self.n_peers, self.n_failed = w + SPARE, p + SPARE, f + SPARE
        self.bits = np.full(self.n_words, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
        self.quota = np.full(self.n_peers, 0x7FFFFFFF, dtype=np.int32)  # a quota nobody owns is never read
        self.failed = (_capi.krk_failed_request * self.n_failed)()
        for j in range(self.n_failed):  # an entry nobody owns is never read: it would be refused
            self.failed[j] = _capi.krk_failed_request(0xFFFFFFF0, 0xFFFFFFF0, 9)
        for t, (w0, p0, f0) in zip(self.torrents, self.offs):
            self.bits[w0:w0 + t.rows.size] = t.rows.reshape(-1)
            self.quota[p0:p0 + t.n_peers] = t.quota
            for j, e in enumerate(t.failed):
                self.failed[f0 + j] = _capi.krk_failed_request(*e)
        self._want = None

    def sizes(self):
        """Elements of (target, quota_left, n_resent)."""
        return self.n_failed, self.n_peers, len(self.torrents) + SPARE

    def want(self):
        """The whole output buffers after the call: (target, quota_left, n_resent), 0xA5 where nobody owns."""
        if self._want is None:
            target, left, n_resent = (np.full(k, CANARY32, dtype=np.uint32) for k in self.sizes())
            left = left.view(np.int32)
            for j, (t, (_, p0, f0)) in enumerate(zip(self.torrents, self.offs)):
                tg, lf, nr = t.want()
                target[f0:f0 + len(t.failed)] = tg
                left[p0:p0 + t.n_peers] = lf
                n_resent[j] = nr
            self._want = (target, left, n_resent)
        return self._want


_cases = None


def cases():
    """Every single-torrent random case of the matrix (built once): P x N x F, with and without
    allow-duplicates, at both densities."""
    global _cases
    if _cases is None:
        _cases = [Batch([random_torrent(n, p, f, flags, salt=k)])
                  for k, (p, n, f) in enumerate((p, n, f) for p in PS for n in NS for f in FS)
                  for flags in (0, DUP)]
    return _cases


def named():
    """[(Batch, targets worked out by hand)]: one property a case."""
    E, U, I = EXPIRED, UNSENT, INVALID
    P = 2 * S + 1
    out = []

    def add(targets, *a, **kw):
        out.append((Batch([sparse(*a, **kw)]), targets))

    for s in (E, U, I):  # each status, from a peer that does not hold the piece any more
        add([1], f"status {s}", 65, 3, [(64, 0, s)], {1: [64], 2: [64]})
    add([0], "peer gone", 65, 2, [(3, NONE, E)], {0: [3], 1: [3]})
    add([NONE], "excluded peer the only holder", 65, 2, [(3, 0, E)], {0: [3]})
    add([NONE], "excluded peer the only holder, invalid", 65, 2, [(3, 0, I)], {0: [3]})
    add([1], "excluded peer the first holder", 65, 3, [(3, 0, E)], {0: [3], 1: [3], 2: [3]})
    add([0], "unsent goes back to its own peer", 65, 3, [(3, 0, U)], {0: [3], 1: [3]})
    add([2, 2, NONE], "quotas -1, 0 and 1, and 2 running out", 65, 4, [(1, NONE, E), (2, NONE, E), (3, NONE, E)],
        {p: [1, 2, 3] for p in range(3)}, quota=[-1, 0, 2, 0])
    add([2, 3, NONE], "quota 1 each", 65, 4, [(1, NONE, U), (2, NONE, U), (3, NONE, U)],
        {p: [1, 2, 3] for p in range(4)}, quota=[-1, 0, 1, 1])
    add([0, 0, 1, 1, NONE], "a quota that runs out in the middle of the list", 4097, 2,
        [(i, NONE, E) for i in (0, 64, 4000, 4095, 4096)], {0: range(4097), 1: range(4097)}, quota=[2, 2])
    add([0, NONE], "one piece twice, no duplicates", 65, 3, [(9, NONE, E), (9, NONE, E)], {0: [9], 1: [9]}, quota=3)
    add([0, 1], "one piece twice, duplicates", 65, 3, [(9, NONE, E), (9, NONE, E)], {0: [9], 1: [9]}, quota=3, flags=DUP)
    add([0, 1, NONE], "one piece three times, two holders, duplicates", 65, 3, [(9, NONE, E)] * 3, {0: [9], 1: [9]},
        quota=3, flags=DUP)
    add([1, 0, NONE], "own-peer exclusion makes the taken peers no prefix", 65, 2, [(9, 0, E), (9, 1, E), (9, NONE, U)],
        {0: [9], 1: [9]}, quota=3, flags=DUP)
    add([0, 0], "the run ends with the piece", 65, 1, [(9, NONE, E), (10, NONE, E)], {0: [9, 10]}, quota=3)
    add([0, NONE, 0], "no duplicates: NONE does not end the run's state", 65, 1, [(9, NONE, E), (9, NONE, U), (10, NONE, U)],
        {0: [9, 10]}, quota=3)
    add([NONE], "the piece in have", 65, 2, [(64, NONE, E)], {0: [64], 1: [64]}, have=[64])
    add([1], "blocked for the first holder only", 65, 2, [(64, NONE, E)], {0: [64], 1: [64]}, blocked={0: [64]})
    for first in (0, S - 1, S, P - 1):  # the first eligible peer's index; peers before it hold, but lack quota or are blocked
        holders = {p: [7] for p in range(0, first + 1, max(first // 5, 1))} | {first: [7]}
        quota = np.zeros(P, dtype=np.int32)
        quota[first:] = 1
        add([first], f"first eligible peer {first}", 64, P, [(7, NONE, E)], holders, quota=quota)
    add([2 * S, S, NONE], "two late peers, duplicates: marks past the first pass", 64, P, [(7, S, E), (7, 2 * S, I), (7, NONE, U)],
        {S: [7], 2 * S: [7]}, quota=5, flags=DUP)
    add([S + 1, S + 1, NONE], "a late peer's quota runs out", 64, P, [(1, NONE, E), (2, NONE, E), (3, NONE, E)],
        {S + 1: [1, 2, 3]}, quota=2)
    for n in (63, 64, 65):  # every row all ones, tail bits included: have is full
        add([NONE, NONE], f"all ones n={n}", n, 3, [(0, NONE, E), (n - 1, 1, U)], {}, ones=True)
    return out


_batches = {}


def batch(k):
    """A batch of k torrents that mixes the matrix's shapes, with a torrent that has no failed
    entries and one that has no peers in the middle."""
    if k not in _batches:
        ts = []
        for j in range(k):
            p, n, f = PS[(2 * j + 3) % len(PS)], NS[(3 * j + 1) % len(NS)], (7, 40, 2, 1)[j % 4]
            if k >= 3 and j == k // 2:
                f = 0
            if k >= 3 and j == k // 2 + 1:
                p = 0
            ts.append(random_torrent(n, p, f, (0, DUP)[j % 2], salt=100 + j))
        _batches[k] = Batch(ts, label=f"batch of {k}")
    return _batches[k]


# ------------------------------------------------------------------ backends
def prefilled(k):
    return np.full(k, CANARY32, dtype=np.uint32)


class HostBackend:
    """krk_piece_resend_round: no device."""

    def run(self, b, left=True):
        tg, lf, nr = (prefilled(k) for k in b.sizes())
        check(lib.krk_piece_resend_round(b.structs, b.resends, len(b.torrents), b.bits.ctypes.data_as(u64p),
                                         b.quota.ctypes.data_as(i32p), b.failed, tg.ctypes.data_as(u32p),
                                         lf.ctypes.data_as(i32p) if left else None, nr.ctypes.data_as(u32p)))
        return tg, lf.view(np.int32), nr


class DeviceBackend:
    """krk_piece_resend_round_dev: the inputs uploaded a batch, the outputs in device memory or,
    with pinned, in krk_host_alloc memory."""

    def __init__(self):
        from kraken_amd import device as D
        self.D = D
        self.inputs = {}

    def upload(self, b):
        if id(b) not in self.inputs:
            bits, quota = self.D.DeviceBuffer(b.bits.nbytes), self.D.DeviceBuffer(b.quota.nbytes)
            bits.from_host(b.bits)
            quota.from_host(b.quota)
            self.inputs[id(b)] = (b, bits, quota)
        return self.inputs[id(b)][1:]

    def outputs(self, b, pinned):
        D = self.D
        outs = [D.PinnedArray((k,), np.uint32) if pinned else D.DeviceBuffer(4 * k) for k in b.sizes()]
        for o, k in zip(outs, b.sizes()):
            if pinned:
                o.a[:] = CANARY32
            else:
                o.from_host(prefilled(k))
        return outs

    def launch(self, b, outs, left=True, stream=None):
        bits, quota = self.upload(b)
        check(lib.krk_piece_resend_round_dev(b.structs, b.resends, len(b.torrents), bits.ptr, quota.ptr, b.failed,
                                             outs[0].ptr, outs[1].ptr if left else None, outs[2].ptr, stream))

    def read(self, b, outs, pinned):
        tg, lf, nr = (o.a.copy() if pinned else o.to_host(np.uint32, k) for o, k in zip(outs, b.sizes()))
        return tg, lf.view(np.int32), nr

    def run(self, b, left=True, pinned=False):
        outs = self.outputs(b, pinned)
        self.launch(b, outs, left)
        check(lib.krk_stream_sync(None))
        return self.read(b, outs, pinned)


# ------------------------------------------------------------------ comparison
def compare(b, got, left=True):
    """Mismatches of one call's whole output buffers against the restatement's, as text."""
    bad = []
    for name, g, w in zip(("target", "quota_left", "n_resent"), got, b.want()):
        if name == "quota_left" and not left:
            w = prefilled(w.size).view(np.int32)  # not asked for: not touched
        if not np.array_equal(g, w):
            k = int(np.flatnonzero(g != w)[0])
            bad.append(f"{b.label}: {name}[{k}] is {int(g[k]):#x}, want {int(w[k]):#x} ({int((g != w).sum())} differ)")
    return bad


def run_cases(backend, batches, **kw):
    """(calls, mismatches): every batch with and without quota_left_out."""
    calls, bad = 0, []
    for b in batches:
        for left in (True, False):
            bad += compare(b, backend.run(b, left=left, **kw), left)
            calls += 1
    return calls, bad


# ------------------------------------------------------------------ refusals
def invalid_calls():
    """[(label, batch, change)]: change(args) edits the argument list of a valid call -- args[0] and
    args[1] are copies of the torrent and resend arrays, args[5] a copy of the failed array -- into
    one that is KRK_EINVAL."""
    b = Batch([random_torrent(65, 3, 4, 0, salt=7), sparse("two entries", 65, 2, [(3, 0, EXPIRED), (9, 1, UNSENT)],
                                                          {0: [3, 9], 1: [3, 9]})], label="refusals")
    f1 = b.offs[1][2]

    def field(arr, j, name, v):
        def change(a):
            setattr(a[arr][j], name, v)
        return change

    def null(k):
        def change(a):
            a[k] = None
        return change

    out = [("n_pieces 2^32", field(0, 1, "n_pieces", 1 << 32)),
           ("piece = n_pieces", field(5, f1 + 1, "piece", 65)),
           ("peer = n_peers", field(5, f1, "peer", 2)),
           ("peer = NONE - 1", field(5, f1, "peer", NONE - 1)),
           ("status 0", field(5, f1 + 1, "status", 0)),
           ("status 4", field(5, f1, "status", 4)),
           ("list descends", field(5, f1 + 1, "piece", 2)),
           ("unknown flag bit", field(0, 0, "flags", 0x200)),
           ("unknown flag bit beside a known one", field(0, 1, "flags", DUP | 0x80000000))]
    out += [(f"NULL argument {k}", null(k)) for k in (0, 1, 3, 4, 5, 6, 8)]
    return [(label, b, change) for label, change in out]


def call_args(b, bits, quota, outs):
    """The argument list of a round call over b (without the stream), its arrays copied so that a
    change leaves b alone.  bits / quota / outs: pointers."""
    structs = (_capi.krk_request_torrent * len(b.structs))()
    resends = (_capi.krk_resend_torrent * len(b.resends))()
    failed = (_capi.krk_failed_request * len(b.failed))()
    for dst, src in ((structs, b.structs), (resends, b.resends), (failed, b.failed)):
        C.memmove(dst, src, C.sizeof(src))
    return [structs, resends, len(b.torrents), bits, quota, failed, *outs]
