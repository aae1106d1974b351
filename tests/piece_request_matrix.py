"""Piece request rounds (piece_request.hip, piece_request_math.hpp) at the kernels' word, wave,
thread-stride and launch edges: the cases, their expectations and the comparison, shared by
tests/test_gpu_piece_request_matrix.py (krk_piece_request_round_dev on the production library) and
tests/test_piece_request_matrix_cpu.py (krk_piece_request_round, the host form the kernels are
documented to equal).  A helper module, not a test file.

G (the pieces one workgroup pass of the selection scan covers), S (the thread stride inside a pass,
one piece a thread; also the pieces of a count unit) and the count launch's workgroup cap are read
from the built library (krk_piece_request_geometry).  A case is a BATCH of torrents and a
pipeline limit; a torrent is built from a seed by one of the kinds below, and its expectation is
tests/piece_request_ref.py's restatement, never the library.  Every array of a batch starts at a
non-zero offset (BASE) and carries SPARE entries past its end; the outputs are prefilled with
0xA5 bytes, so a batch's expected output is the whole buffer: every owned element stored, nothing
else touched.

 random        have 1/2, peers 1/2, blocked 1/8; the peers' tail bits all set
 equal         every peer has every piece, nothing had or blocked: all counts equal, so the picks
               are the lowest indices and successive peers walk up from piece 0
 ties          as equal, but only the pieces around the word / wave boundary (64), the thread
               stride (S, 2 S), the pass (G) and the last piece are missing from `have`: equal keys on
               both sides of every boundary, handed out peer after peer
 first / last  the only candidate is piece 0 / piece N - 1
 ones          every row all ones, tail bits included (have is full: nothing to pick, counts = P)
 have_full     have all ones, the rest random;  blocked_full: every blocked row all ones
 twins         two identical peers (random), to run with and without allow-duplicates"""
import ctypes as C

import numpy as np

from kraken_amd import _capi
from kraken_amd._capi import check, lib
from tests import piece_request_ref as R

SEED = 20261021
SPARE = 4
CANARY32 = np.uint32(0xA5A5A5A5)
BASE = (3, 5, 7)  # the first word, peer and piece a batch uses
u32p, u64p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
RAREST, SAMPLE, DUP = R.RAREST_FIRST, R.SAMPLE, R.ALLOW_DUPLICATES


def geometry():
    g, t, m = C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(lib.krk_piece_request_geometry(C.byref(g), C.byref(t), C.byref(m)))
    return int(g.value), int(t.value), int(m.value)


G, S, MAX_WG = geometry()
LMAX = _capi.KRK_PR_MAX_LIMIT
N_C4 = 81920
NS = (0, 1, 63, 64, 65, S - 1, S, S + 1, G - 1, G, G + 1, 2 * G + 1, N_C4)
TIES = (62, 63, 64, 65, S - 2, S - 1, S, S + 1, 2 * S - 1, 2 * S, G - 1, G, 2 * G - 1, 2 * G)
PS = (0, 1, 2, 10, 300)
LS = (1, 3, LMAX)


def words(n):
    return (n + 63) // 64


def pack(b):
    p = np.packbits(np.asarray(b, dtype=bool), bitorder="little")
    return np.concatenate([p, np.zeros(-p.size % 8, dtype=np.uint8)]).view(np.uint64)


def tail(n):
    """The last word's bits past n, as a word (0 when n is a multiple of 64)."""
    return np.uint64(((1 << 64) - 1) ^ ((1 << (n % 64)) - 1)) if n % 64 else np.uint64(0)


def quotas(n_peers, limit, first=0):
    """-1, 0, 1, L, L in turn (the last L is "more than there are candidates" wherever fewer are left)."""
    cycle = (-1, 0, 1, limit, limit)
    return np.array([cycle[(first + p) % 5] for p in range(n_peers)], dtype=np.int32)


class Torrent:
    def __init__(self, kind, n, n_peers, flags, quota, salt=0):
        self.kind, self.n, self.n_peers, self.flags = kind, int(n), int(n_peers), int(flags)
        self.quota = np.asarray(quota, dtype=np.int32)
        assert self.quota.size == n_peers
        rng = np.random.default_rng([SEED, n, n_peers, salt])
        self.seed = int(rng.integers(0, 1 << 63)) * 2 + 1
        W, ones = words(n), np.uint64((1 << 64) - 1)
        rows = np.zeros((1 + 2 * n_peers, W), dtype=np.uint64)
        rnd = lambda p: pack(rng.random(n) < p) if n else np.zeros(0, np.uint64)
        if kind in ("random", "have_full", "blocked_full", "twins"):
            rows[0] = rnd(0.5)
            for p in range(n_peers):
                rows[1 + 2 * p], rows[2 + 2 * p] = rnd(0.5), rnd(0.125)
            if kind == "twins" and n_peers >= 2:
                rows[3:5] = rows[1:3]
            if kind == "have_full":
                rows[0] = ones
            if kind == "blocked_full":
                rows[2::2] = ones
        elif kind in ("equal", "ties", "first", "last"):
            rows[1::2] = ones
            keep = {"equal": range(n), "first": [0], "last": [n - 1],
                    "ties": (*TIES, n - 1)}[kind]
            have = np.ones(n, dtype=bool)
            have[[i for i in keep if 0 <= i < n]] = False
            rows[0] = pack(have)
        elif kind == "ones":
            rows[:] = ones
        else:
            raise ValueError(kind)
        if W and kind != "ones":  # the peers' tail bits set, have's and blocked's clear: only the call's mask stops them
            rows[1::2, -1] |= tail(n)
            rows[0::2, -1] &= ~tail(n)
            if kind == "blocked_full":
                rows[2::2, -1] = ones & ~tail(n)
        self.rows = rows
        self.rows.setflags(write=False)
        self.label = f"{kind} n={n} P={n_peers} flags={flags:#x}"
        self._want = {}

    def want(self, limit):
        if limit not in self._want:
            self._want[limit] = R.round_torrent(self.rows, self.n, self.n_peers, self.flags, self.seed, self.quota, limit)
        return self._want[limit]


class Batch:
    """Torrents packed back to back from BASE, in the order given."""

    def __init__(self, torrents, limit, label=None):
        self.torrents, self.limit = list(torrents), int(limit)
        self.label = label or f"L={limit} " + " | ".join(t.label for t in self.torrents)
        k = len(self.torrents)
        self.structs = (_capi.krk_request_torrent * max(k, 1))()
        w, p, i = BASE
        self.offs = []
        for j, t in enumerate(self.torrents):
            self.offs.append((w, p, i))
            self.structs[j] = _capi.krk_request_torrent(t.n, t.n_peers, t.flags, t.seed, w, p, i)
            w, p, i = w + t.rows.size, p + t.n_peers, i + t.n
        self.n_words, self.n_peers, self.n_pieces = w + SPARE, p + SPARE, i + SPARE
        self.bits = np.full(self.n_words, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
        self.quota = np.full(self.n_peers, 0x7FFFFFFF, dtype=np.int32)  # a quota nobody owns is never read
        for t, (w0, p0, _) in zip(self.torrents, self.offs):
            self.bits[w0:w0 + t.rows.size] = t.rows.reshape(-1)
            self.quota[p0:p0 + t.n_peers] = t.quota
        self._want = None

    def sizes(self):
        """Elements of (counts, picks, n_picked)."""
        return self.n_pieces, self.n_peers * self.limit, self.n_peers

    def want(self):
        """The whole output buffers after the call: (counts, picks, n_picked), 0xA5 where nobody owns."""
        if self._want is None:
            counts, picks, n_picked = (np.full(k, CANARY32, dtype=np.uint32) for k in self.sizes())
            for t, (_, p0, i0) in zip(self.torrents, self.offs):
                c, pk, npk = t.want(self.limit)
                counts[i0:i0 + t.n] = c
                picks[p0 * self.limit:(p0 + t.n_peers) * self.limit] = pk.reshape(-1)
                n_picked[p0:p0 + t.n_peers] = npk
            self._want = (counts, picks, n_picked)
        return self._want


def single(kind, n, n_peers, flags, limit, quota=None, salt=0):
    q = quotas(n_peers, limit, first=3) if quota is None else quota
    return Batch([Torrent(kind, n, n_peers, flags, q, salt)], limit)


_cases = None


def cases():
    """Every single-torrent case of the matrix (built once)."""
    global _cases
    if _cases is not None:
        return _cases
    out = []
    for n in NS:  # every N, both policies, the quota cycle starting at L
        for flags in (RAREST, SAMPLE):
            out.append(single("random", n, 2, flags, 3))
            out.append(single("random", n, 10, flags | (DUP if n % 2 else 0), 3, quota=quotas(10, 3)))
    for n in (65, S + 1, 2 * G + 1):  # every L and P, every quota for a lone peer
        for limit in LS:
            for flags in (RAREST, SAMPLE):
                for q in (-1, 0, 1, limit):
                    out.append(single("random", n, 1, flags, limit, quota=[q]))
                out.append(single("random", n, 2, flags, limit, quota=[limit, limit]))
                out.append(single("random", n, 0, flags, limit))
        for flags in (RAREST, SAMPLE, RAREST | DUP):  # counts past 255, the longest peer loop
            out.append(single("equal", n, 300, flags, LMAX))
            out.append(single("random", n, 300, flags, 3, quota=quotas(300, 3)))
    for n in (1, 63, 64, 65, S - 1, S, S + 1, G - 1, G, G + 1, 2 * G + 1, N_C4):
        for flags in (RAREST, SAMPLE):
            for kind in ("equal", "ties", "first", "last", "ones", "have_full", "blocked_full"):
                out.append(single(kind, n, 3, flags, 3, quota=[3, 3, 3]))
        out.append(single("ties", n, 10, RAREST, LMAX, quota=[LMAX] * 10))
        out.append(single("first", n, 2, RAREST, 1, quota=[1, 1]))  # more quota than candidates at L = 1
    for n in (65, 2 * G + 1):
        for flags in (RAREST, SAMPLE, RAREST | DUP, SAMPLE | DUP):
            out.append(single("twins", n, 2, flags, 3, quota=[3, 3]))
    _cases = out
    return out


_batches = {}


def batch(k, limit=3):
    """A batch of k torrents that mixes the N of the matrix, both policies and every kind, with a
    zero-piece and a zero-peer torrent in the middle."""
    if (k, limit) not in _batches:
        kinds = ("random", "ties", "equal", "twins", "last", "blocked_full", "random")
        ts = []
        for j in range(k):
            n = NS[(3 * j + 7) % len(NS)]
            p = (2, 10, 3, 2, 1)[j % 5]
            if k >= 3 and j == k // 2:
                n = 0
            if k >= 3 and j == k // 2 + 1:
                p = 0
            flags = (RAREST, SAMPLE, RAREST | DUP, SAMPLE)[j % 4]
            ts.append(Torrent(kinds[j % len(kinds)], n, p, flags, quotas(p, limit, first=j), salt=j + 1))
        _batches[(k, limit)] = Batch(ts, limit, label=f"batch of {k}, L={limit}")
    return _batches[(k, limit)]


# ------------------------------------------------------------------ backends
def prefilled(k):
    return np.full(k, CANARY32, dtype=np.uint32)


class HostBackend:
    """krk_piece_request_round: no device."""

    def run(self, b, counts=True):
        c, pk, npk = (prefilled(k) for k in b.sizes())
        check(lib.krk_piece_request_round(b.structs, len(b.torrents), b.bits.ctypes.data_as(u64p),
                                          b.quota.ctypes.data_as(i32p), b.limit,
                                          c.ctypes.data_as(u32p) if counts else None, pk.ctypes.data_as(u32p),
                                          npk.ctypes.data_as(u32p)))
        return c, pk, npk


class DeviceBackend:
    """krk_piece_request_round_dev: the inputs uploaded a batch, the outputs in device memory or,
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

    def launch(self, b, outs, counts=True, stream=None):
        bits, quota = self.upload(b)
        check(lib.krk_piece_request_round_dev(b.structs, len(b.torrents), bits.ptr, quota.ptr, b.limit,
                                              outs[0].ptr if counts else None, outs[1].ptr, outs[2].ptr, stream))

    def read(self, b, outs, pinned):
        return tuple(o.a.copy() if pinned else o.to_host(np.uint32, k) for o, k in zip(outs, b.sizes()))

    def run(self, b, counts=True, pinned=False):
        outs = self.outputs(b, pinned)
        self.launch(b, outs, counts)
        check(lib.krk_stream_sync(None))
        return self.read(b, outs, pinned)


# ------------------------------------------------------------------ comparison
def compare(b, got, counts=True):
    """Mismatches of one call's whole output buffers against the restatement's, as text."""
    bad = []
    want = b.want()
    for name, g, w in zip(("counts", "picks", "n_picked"), got, want):
        if name == "counts" and not counts:
            w = prefilled(w.size)  # not asked for: not touched
        if not np.array_equal(g, w):
            k = int(np.flatnonzero(g != w)[0])
            bad.append(f"{b.label}: {name}[{k}] is {int(g[k]):#x}, want {int(w[k]):#x} ({int((g != w).sum())} differ)")
    return bad


def run_cases(backend, batches, **kw):
    """(calls, mismatches): every batch with and without counts_out."""
    calls, bad = 0, []
    for b in batches:
        for counts in (True, False):
            bad += compare(b, backend.run(b, counts=counts, **kw), counts)
            calls += 1
    return calls, bad
