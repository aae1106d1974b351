"""Cleanup plans from a listing's text (krk_cleanup_plan, krk_cleanup_plan_dev: digest_hex.hip's
fused phase 1 in front of ring_select.hip's scan and scatter) at the kernels' lane, wave,
workgroup and scan-tile edges: the cases, their expectations and the comparison, shared by
tests/test_gpu_cleanup_plan_matrix.py and tests/test_cleanup_plan_matrix_cpu.py.  A helper module,
not a test file.

The listing is tests/ring_select_matrix.py's: its N_MAX seeded digests as hex names with a random
case a letter, its shapes (0, 1, 63, 64, 65, W +- 1, T W +- 1, 2 T W + W + 37), its four masks
(random, the one-shard `edges`, zeros, ones) and its EDGES.  Beside the wave, workgroup and tile
edges (never ON an EDGES position, whose names the `edges` mask must select) sit the INVALID
names -- a bad byte, 63 characters (which also moves every later name to an odd offset) and the
empty name, in turn: never selected, not even under `ones` with an expired mtime, their valid
bits 0.  The mtimes are mostly fresh, expired with probability 1/64, and at SPECIAL positions
now - ttl (not expired: the comparison is strict), now - ttl - 1 (expired) and INT64_MIN (expired:
the subtraction saturates); the `negative now` variant has now < 0 and INT64_MAX mtimes among
them (not expired: the subtraction saturates at INT64_MIN).  The expectation is a numpy
transcription of the contract (reference()), never the library; outputs are prefilled with 0xFF
and carry SPARE entries (ring_select_matrix.compare checks them)."""
import ctypes as C

import numpy as np

from kraken_amd._capi import check, lib
from tests import ring_select_matrix as R

W, T, SPARE, CANARY = R.W, R.T, R.SPARE, R.CANARY
SMALL, LARGE, SHAPES, N_MAX = R.SMALL, R.LARGE, R.SHAPES, R.N_MAX
u64p, i64p = R.u64p, C.POINTER(C.c_int64)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
NOW, TTL = 1_700_000_000_000_000_000, 3_600_000_000_000
NEG_NOW = -5_000_000_000
words = R.words

_beside = sorted({1, 62, 65, 126, 129, W - 65, W - 2, W + 1, 2 * W - 2, 2 * W + 1, T * W - 2, T * W + 1,
                  2 * T * W - 2, 2 * T * W + 1, N_MAX - 2} | {n - 2 for n in SHAPES if n > 2})
INVALID = [p for p in _beside if 0 <= p < N_MAX and p not in R.EDGES]
SPECIAL = [p for p in (2, 60, 66, 130, W - 4, W + 2, T * W - 4, T * W + 2, N_MAX - 4) if p not in R.EDGES and p not in INVALID]


def sat_sub(now, t):
    """now - t over int64 arrays, saturating: a numpy transcription of time.Time.Sub."""
    with np.errstate(over="ignore"):
        r = np.int64(now) - t
    r = np.where((t < 0) & (r < now), I64_MAX, r)  # subtracting a negative must not come out smaller
    return np.where((t > 0) & (r > now), I64_MIN, r)


class Data:
    """The shared listing, built once and left unchanged."""

    def __init__(self):
        self.ring = R.Data()
        self.masks = self.ring.masks
        rng = np.random.default_rng(R.SEED + 12)
        d = self.ring.digests
        hexd = np.frombuffer(b"0123456789abcdef", dtype=np.uint8)
        chars = np.empty((N_MAX, 64), dtype=np.uint8)
        chars[:, 0::2], chars[:, 1::2] = hexd[d >> 4], hexd[d & 15]
        upper = (chars >= 0x61) & (rng.random((N_MAX, 64)) < 0.5)
        chars[upper] -= 32
        lens = np.full(N_MAX, 64, dtype=np.uint64)
        kinds = {}
        for k, p in enumerate(INVALID):
            kinds[p] = ("byte", "short", "empty")[k % 3]
            lens[p] = {"byte": 64, "short": 63, "empty": 0}[kinds[p]]
            if kinds[p] == "byte":
                chars[p, (7 * k) % 64] = b"g/:@G`\x00\x80\xff"[k % 9]
        self.kinds = kinds
        self.off = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(lens, dtype=np.uint64)])
        keep = np.arange(64, dtype=np.uint64)[None, :] < lens[:, None]
        text = np.concatenate([chars[keep], np.zeros(1, dtype=np.uint8)])  # rows back to back; a spare byte, never read
        assert text.size == int(self.off[-1]) + 1
        self.text = text
        # mtimes
        mt = NOW - rng.integers(0, TTL, size=N_MAX, dtype=np.int64)
        old = rng.random(N_MAX) < 1 / 64
        mt[old] -= TTL
        for k, p in enumerate(SPECIAL):
            mt[p] = (NOW - TTL, NOW - TTL - 1, I64_MIN)[k % 3]
        for p in INVALID:
            mt[p] = NOW - 2 * TTL  # expired: an invalid name is not selected all the same
        self.mtime = mt
        neg = NEG_NOW - rng.integers(0, 2 * TTL, size=N_MAX, dtype=np.int64)
        for k, p in enumerate(SPECIAL + list(R.EDGES)):
            neg[p] = (I64_MAX, NEG_NOW - TTL - 1, I64_MIN, NEG_NOW - TTL)[k % 4]
        self.mtime_neg = neg
        for a in (self.off, self.text, self.mtime, self.mtime_neg):
            a.setflags(write=False)
        # the transcription's parse: a name is valid when it has 64 bytes, all of them hex digits
        lens_ = (self.off[1:] - self.off[:-1])
        table = np.full(256, -1, dtype=np.int8)
        for i, c in enumerate(b"0123456789abcdef"):
            table[c] = i
        for i, c in enumerate(b"ABCDEF"):
            table[c] = 10 + i
        is64 = lens_ == 64
        val = np.empty((N_MAX, 64), dtype=np.int8)
        for a in range(0, N_MAX, 1 << 16):  # name i's bytes are text[off[i], off[i] + 64)
            o = np.where(is64[a:a + (1 << 16)], self.off[:-1][a:a + (1 << 16)], 0).astype(np.int64)
            val[a:a + (1 << 16)] = table[text[o[:, None] + np.arange(64)]]
        self.valid = is64 & (val >= 0).all(axis=1)
        v4 = val[:, :4].astype(np.int64)
        self.shard = np.where(self.valid, v4[:, 0] << 12 | v4[:, 1] << 8 | v4[:, 2] << 4 | v4[:, 3], 0)
        assert not self.valid[INVALID].any() and self.valid.sum() == N_MAX - len(INVALID)
        assert np.array_equal(self.shard[self.valid], self.ring.shard[self.valid])

    def times(self, case):
        """(mtime column or None, now) of a case."""
        return {"none": (None, NOW), "mtime": (self.mtime, NOW), "negative now": (self.mtime_neg, NEG_NOW)}[case.times]

    def reference(self, case):
        """(bits, idx, valid words) of the contract:
        sel(i) = valid(i) & ((mask[ShardID(d_i)] ^ invert) | expired(now, mtime[i], ttl))."""
        n = case.n
        sel = R._unpack(self.masks[case.mask], 65536)[self.shard[:n]] ^ bool(case.invert)
        mt, now = self.times(case)
        if mt is not None:
            sel = sel | (sat_sub(now, mt[:n]) > TTL)
        sel = sel & self.valid[:n]
        return R._pack(sel)[:words(n)], np.flatnonzero(sel).astype(np.uint64), R._pack(self.valid[:n])[:words(n)]


class Case:
    def __init__(self, n, mask, invert, times):
        self.n, self.mask, self.invert, self.times = n, mask, invert, times
        self.label = f"n={n} mask={mask} invert={int(invert)} times={times}"


def cases(shapes=SHAPES):
    """Every shape x {random, edges} x invert x {no mtime, mtime}; zeros and ones (and their
    inverses) with mtimes -- `ones` with an expired mtime beside every invalid name -- and the
    negative now under the edges mask."""
    out = []
    for n in shapes:
        for mask in ("random", "edges"):
            for invert in (False, True):
                for times in ("none", "mtime"):
                    out.append(Case(n, mask, invert, times))
        for mask in ("zeros", "ones"):
            for invert in (False, True):
                out.append(Case(n, mask, invert, "mtime"))
        out.append(Case(n, "edges", False, "negative now"))
    return out


def caps(count):
    return sorted({0, 1, max(count - 1, 0), count, count + SPARE})


# ------------------------------------------------------------------ backends
class HostBackend:
    """krk_cleanup_plan: no device."""

    def __init__(self, data):
        self.data = data

    def run(self, case, cap, null_idx=False, null_valid=False):
        """(bits with SPARE, count, idx with SPARE, valid with SPARE) after one call into
        0xFF-prefilled outputs."""
        n, d = case.n, self.data
        bits = np.full(words(n) + SPARE, CANARY, dtype=np.uint64)
        valid = np.full(words(n) + SPARE, CANARY, dtype=np.uint64)
        idx = np.full(cap + SPARE, CANARY, dtype=np.uint64)
        count = np.full(1, CANARY, dtype=np.uint64)
        mt, now = d.times(case)
        check(lib.krk_cleanup_plan(d.text.ctypes.data, d.off.ctypes.data_as(u64p), n,
                                   mt.ctypes.data_as(i64p) if mt is not None else None, now, TTL,
                                   d.masks[case.mask].ctypes.data_as(u64p), int(case.invert), bits.ctypes.data_as(u64p),
                                   None if null_valid else valid.ctypes.data_as(u64p),
                                   None if null_idx else idx.ctypes.data_as(u64p), cap, count.ctypes.data_as(u64p)))
        return bits, int(count[0]), idx, valid


class DeviceBackend:
    """krk_cleanup_plan_dev: the text (at a byte offset of `shift`), the offsets and both mtime
    columns uploaded once; the outputs in device memory or, with pinned, in krk_host_alloc memory."""

    def __init__(self, data, shift=0):
        from kraken_amd import device as D
        self.D, self.data, self.shift = D, data, shift
        self.text = D.DeviceBuffer(data.text.nbytes + 8)
        self.text.from_host(data.text, offset=shift)
        self.off = D.DeviceBuffer(data.off.nbytes)
        self.off.from_host(data.off)
        self.mt = {}
        for k, a in (("mtime", data.mtime), ("negative now", data.mtime_neg)):
            self.mt[k] = D.DeviceBuffer(a.nbytes)
            self.mt[k].from_host(a)
        self.outs = {}

    def run(self, case, cap, null_idx=False, null_valid=False, pinned=False, mask_after=None):
        n, D = case.n, self.D
        sizes = (words(n) + SPARE, cap + SPARE, 1, words(n) + SPARE)
        if pinned not in self.outs:  # one set of outputs a memory kind, sized for the largest case
            full = (words(N_MAX) + SPARE, N_MAX + 1 + 2 * SPARE, 1, words(N_MAX) + SPARE)
            self.outs[pinned] = [D.PinnedArray((k,), np.uint64) if pinned else D.DeviceBuffer(8 * k) for k in full]
        bits, idx, count, valid = outs = self.outs[pinned]
        for o, k in zip(outs, sizes):  # the entries this call may touch, and SPARE past them
            if pinned:
                o.a[:k] = CANARY
            else:
                o.from_host(np.full(k, CANARY, dtype=np.uint64))
        mask = self.data.masks[case.mask].copy()
        now = self.data.times(case)[1]
        check(lib.krk_cleanup_plan_dev(self.text.ptr + self.shift, self.off.ptr, n,
                                       self.mt[case.times].ptr if case.times != "none" else None, now, TTL,
                                       mask.ctypes.data_as(u64p), int(case.invert), bits.ptr,
                                       None if null_valid else valid.ptr, None if null_idx else idx.ptr, cap, count.ptr,
                                       None))
        if mask_after is not None:
            mask[:] = mask_after  # the call has staged its copy
        check(lib.krk_stream_sync(None))
        if pinned:
            return bits.a[:sizes[0]].copy(), int(count.a[0]), idx.a[:sizes[1]].copy(), valid.a[:sizes[3]].copy()
        return (bits.to_host(np.uint64, sizes[0]), int(count.to_host(np.uint64, 1)[0]), idx.to_host(np.uint64, sizes[1]),
                valid.to_host(np.uint64, sizes[3]))


# ------------------------------------------------------------------ comparison
def compare(case, cap, got, want, null_valid=False):
    """Mismatches of one call's (bits, count, idx, valid) against reference() as text."""
    bits, count, idx, valid = got
    wbits, widx, wvalid = want
    bad = R.compare(case, cap, (bits, count, idx), (wbits, widx))
    nw, tag = words(case.n), f"{case.label} cap={cap}"
    if null_valid:
        if not (valid == CANARY).all():
            bad.append(f"{tag}: valid_out passed as NULL was written")
        return bad
    if not np.array_equal(valid[:nw], wvalid):
        w = int(np.flatnonzero(valid[:nw] != wvalid)[0])
        bad.append(f"{tag}: valid word {w} is {int(valid[w]):#x}, want {int(wvalid[w]):#x}")
    if not (valid[nw:] == CANARY).all():
        bad.append(f"{tag}: a word past the valid bitset's {nw} was written")
    return bad


def run_cases(backend, case_list, all_caps=True, **kw):
    """(calls, mismatches): every case at each idx_cap of caps(count) (or, without all_caps, at
    count + SPARE only), and once with a NULL index list and a NULL valid_out."""
    calls, bad = 0, []
    for case in case_list:
        want = backend.data.reference(case)
        count = int(want[1].size)
        for cap in (caps(count) if all_caps else [count + SPARE]):
            bad += compare(case, cap, backend.run(case, cap, **kw), want)
            calls += 1
        bad += compare(case, 0, backend.run(case, 0, null_idx=True, null_valid=True, **kw), want, null_valid=True)
        calls += 1
    return calls, bad


# ------------------------------------------------------------------ the unfused chain
def chain(data, case, parse, select):
    """parse -> krk_expiry_bits -> a ring selection with or_bits over the valid-only sublisting,
    mapped back to listing positions: (idx, valid bool [n]).  parse(n) -> (digests uint8 [n, 32],
    valid words); select(digests [m, 32], mask, invert, or_bits) -> idx."""
    n = case.n
    digests, vwords = parse(n)
    valid = R._unpack(vwords, n)
    good = np.flatnonzero(valid)
    mt, now = data.times(case)
    or_bits = None
    if mt is not None:
        sub = np.ascontiguousarray(mt[:n][good])
        or_bits = np.zeros(words(good.size), dtype=np.uint64)
        check(lib.krk_expiry_bits(sub.ctypes.data_as(i64p), None, good.size, now, TTL, 0,
                                  or_bits.ctypes.data_as(u64p) if good.size else None))
    idx = select(np.ascontiguousarray(digests[good]), data.masks[case.mask], case.invert, or_bits)
    return good[idx.astype(np.int64)].astype(np.uint64), valid
