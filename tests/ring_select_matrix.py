"""Ring selection (ring_select.hip, ring_select_math.hpp) at the kernel's lane, wave, workgroup
and scan-tile edges: the cases, their expectations and the comparison, shared by
tests/test_gpu_ring_select_matrix.py (krk_ring_select_dev on the production library) and
tests/test_ring_select_matrix_cpu.py (krk_ring_select, the host form the kernel is documented to
equal).  A helper module, not a test file.

Every case is a prefix of ONE seeded buffer of N_MAX random digests and one of four shard masks:
 random  every shard selected with probability 1/2;
 edges   ONE shard selected, which no digest has but those at EDGES: the first and last lane of
         a wave, of a workgroup and of a scan tile, and the last digest of every shape -- so the
         expected index list is exactly the EDGES below n;
 zeros / ones  nothing / everything selected.
The expectation is a numpy transcription of the contract (reference()), never the library.  W (the
digests a workgroup takes) and T (the workgroup counts a scan tile holds) are read from the built
library (krk_ring_select_geometry); shapes: 0, 1, 63, 64, 65, W-1, W, W+1, T W - 1, T W + 1 and two
full scan tiles plus a ragged tail.  or_bits carry set bits past n in their last word, which the
call must not let through.  Outputs are prefilled with 0xFF bytes and carry SPARE entries past
their end: every word of the bitset is stored, nothing past it, the count always, and no index
entry past min(count, idx_cap)."""
import ctypes as C

import numpy as np

from kraken_amd import _capi
from kraken_amd._capi import check, lib

SEED = 20261020
SPARE = 4
CANARY = np.uint64(0xFFFFFFFFFFFFFFFF)
EDGE_SHARD = 0xBEEF
u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)


def geometry():
    w, t = C.c_uint64(), C.c_uint64()
    check(lib.krk_ring_select_geometry(C.byref(w), C.byref(t)))
    return int(w.value), int(t.value)


W, T = geometry()
N_TAIL = 2 * T * W + W + 37  # two full scan tiles, one more workgroup and a ragged wave
N_MAX = N_TAIL
SMALL = (0, 1, 63, 64, 65, W - 1, W, W + 1)
LARGE = (T * W - 1, T * W + 1, N_TAIL)
SHAPES = SMALL + LARGE
EDGES = sorted({0, 63, 64, 127, W - 64, W - 1, W, 2 * W - 1, T * W - 1, T * W, 2 * T * W - 1, 2 * T * W}
               | {n - 1 for n in SHAPES if n})


def words(n):
    return (n + 63) // 64


def _unpack(w64, n):
    return np.unpackbits(np.ascontiguousarray(w64).view(np.uint8), bitorder="little")[:n].astype(bool)


def _pack(sel):
    b = np.packbits(sel, bitorder="little")
    return np.concatenate([b, np.zeros(-b.size % 8, dtype=np.uint8)]).view(np.uint64)


class Data:
    """The shared inputs, built once and left unchanged."""

    def __init__(self):
        rng = np.random.default_rng(SEED)
        d = rng.integers(0, 256, size=(N_MAX, 32), dtype=np.uint8)
        hit = (d[:, 0] == EDGE_SHARD >> 8) & (d[:, 1] == EDGE_SHARD & 0xFF)
        d[hit, 1] ^= 1
        d[EDGES, 0], d[EDGES, 1] = EDGE_SHARD >> 8, EDGE_SHARD & 0xFF
        self.digests = d
        self.shard = d[:, 0].astype(np.uint32) << 8 | d[:, 1]
        edges = np.zeros(1024, dtype=np.uint64)
        edges[EDGE_SHARD >> 6] = np.uint64(1) << np.uint64(EDGE_SHARD & 63)
        self.masks = {"random": rng.integers(0, 1 << 64, size=1024, dtype=np.uint64), "edges": edges,
                      "zeros": np.zeros(1024, dtype=np.uint64), "ones": np.full(1024, CANARY, dtype=np.uint64)}
        self.or_sel = rng.random(N_MAX + 64) < 1 / 64  # bits past n too: the call masks its last word
        for a in (self.digests, self.shard, self.or_sel, *self.masks.values()):
            a.setflags(write=False)

    def or_bits(self, n):
        """n bits of or_sel as words, the last word's tail bits as or_sel has them plus bit 63."""
        if not n:
            return np.zeros(0, dtype=np.uint64)
        w = _pack(self.or_sel[:words(n) * 64]).copy()
        if n % 64:
            w[-1] |= np.uint64(1) << np.uint64(63)
        return w

    def reference(self, case):
        """(bits, idx) of the contract: sel(i) = (mask[ShardID(d_i)] ^ invert) | or_bits[i]."""
        n = case.n
        sel = _unpack(self.masks[case.mask], 65536)[self.shard[:n]] ^ bool(case.invert)
        if case.with_or:
            sel = sel | _unpack(self.or_bits(n), n)
        return _pack(sel)[:words(n)], np.flatnonzero(sel).astype(np.uint64)


class Case:
    def __init__(self, n, mask, invert, with_or):
        self.n, self.mask, self.invert, self.with_or = n, mask, invert, with_or
        self.label = f"n={n} mask={mask} invert={int(invert)} or_bits={int(with_or)}"


def cases(shapes=SHAPES):
    """Every shape x {random, edges} x invert x or_bits; zeros and ones (none and all selected, and
    their inverses) without or_bits."""
    out = []
    for n in shapes:
        for mask in ("random", "edges"):
            for invert in (False, True):
                for with_or in (False, True):
                    out.append(Case(n, mask, invert, with_or))
        for mask in ("zeros", "ones"):
            for invert in (False, True):
                out.append(Case(n, mask, invert, False))
    return out


def caps(count):
    return sorted({0, max(count - 1, 0), count, count + 1})


# ------------------------------------------------------------------ backends
class HostBackend:
    """krk_ring_select: no device."""

    def __init__(self, data):
        self.data = data

    def run(self, case, cap, null_idx=False):
        """(bits with SPARE, count, idx with SPARE) after one call into 0xFF-prefilled outputs."""
        n, d = case.n, self.data
        bits = np.full(words(n) + SPARE, CANARY, dtype=np.uint64)
        idx = np.full(cap + SPARE, CANARY, dtype=np.uint64)
        count = np.full(1, CANARY, dtype=np.uint64)
        ob = d.or_bits(n) if case.with_or else None
        check(lib.krk_ring_select(d.digests.ctypes.data_as(u8p), n, d.masks[case.mask].ctypes.data_as(u64p),
                                  int(case.invert), ob.ctypes.data_as(u64p) if ob is not None else None,
                                  bits.ctypes.data_as(u64p), None if null_idx else idx.ctypes.data_as(u64p), cap,
                                  count.ctypes.data_as(u64p)))
        return bits, int(count[0]), idx


class DeviceBackend:
    """krk_ring_select_dev: the digests uploaded once (at a byte offset of `shift`), or_bits in
    device memory, the outputs in device memory or, with pinned, in krk_host_alloc memory."""

    def __init__(self, data, shift=0):
        from kraken_amd import device as D
        self.D, self.data, self.shift = D, data, shift
        self.dev = D.DeviceBuffer(32 * N_MAX + 64)
        self.dev.from_host(data.digests.reshape(-1), offset=shift)
        self.or_dev, self.outs = {}, {}

    def _or(self, n):
        if n not in self.or_dev:
            b = self.D.DeviceBuffer(8 * max(words(n), 1))
            b.from_host(self.data.or_bits(n))
            self.or_dev[n] = b
        return self.or_dev[n]

    def run(self, case, cap, null_idx=False, pinned=False, mask_after=None):
        n, D = case.n, self.D
        sizes = (words(n) + SPARE, cap + SPARE, 1)
        if pinned not in self.outs:  # one set of outputs a memory kind, sized for the largest case
            full = (words(N_MAX) + SPARE, N_MAX + 1 + SPARE, 1)
            self.outs[pinned] = [D.PinnedArray((k,), np.uint64) if pinned else D.DeviceBuffer(8 * k) for k in full]
        bits, idx, count = outs = self.outs[pinned]
        for o, k in zip(outs, sizes):  # the entries this call may touch, and SPARE past them
            if pinned:
                o.a[:k] = CANARY
            else:
                o.from_host(np.full(k, CANARY, dtype=np.uint64))
        mask = self.data.masks[case.mask].copy()
        check(lib.krk_ring_select_dev(self.dev.ptr + self.shift, n, mask.ctypes.data_as(u64p), int(case.invert),
                                      self._or(n).ptr if case.with_or else None, bits.ptr,
                                      None if null_idx else idx.ptr, cap, count.ptr, None))
        if mask_after is not None:
            mask[:] = mask_after  # the call has staged its copy
        check(lib.krk_stream_sync(None))
        if pinned:
            return bits.a[:sizes[0]].copy(), int(count.a[0]), idx.a[:sizes[1]].copy()
        return bits.to_host(np.uint64, sizes[0]), int(count.to_host(np.uint64, 1)[0]), idx.to_host(np.uint64, sizes[1])


# ------------------------------------------------------------------ comparison
def compare(case, cap, got, want):
    """Mismatches of one call's (bits, count, idx) against reference()'s (bits, idx) as text."""
    bits, count, idx = got
    wbits, widx = want
    bad, nw, keep = [], words(case.n), min(widx.size, cap)
    tag = f"{case.label} cap={cap}"
    if not np.array_equal(bits[:nw], wbits):
        w = int(np.flatnonzero(bits[:nw] != wbits)[0])
        bad.append(f"{tag}: bits word {w} is {int(bits[w]):#x}, want {int(wbits[w]):#x}")
    if not (bits[nw:] == CANARY).all():
        bad.append(f"{tag}: a word past the bitset's {nw} was written")
    if count != widx.size:
        bad.append(f"{tag}: count {count}, want {widx.size}")
    if not np.array_equal(idx[:keep], widx[:keep]):
        k = int(np.flatnonzero(idx[:keep] != widx[:keep])[0])
        bad.append(f"{tag}: idx[{k}] is {int(idx[k])}, want {int(widx[k])}")
    if not (idx[keep:] == CANARY).all():
        bad.append(f"{tag}: an index entry past min(count, cap) = {keep} was written")
    return bad


def run_cases(backend, case_list, all_caps=True, **kw):
    """(calls, mismatches): every case at each idx_cap of caps(count) (or, without all_caps, at
    count + 1 only), and once with a NULL index list."""
    calls, bad = 0, []
    for case in case_list:
        want = backend.data.reference(case)
        count = int(want[1].size)
        for cap in (caps(count) if all_caps else [count + 1]):
            bad += compare(case, cap, backend.run(case, cap, **kw), want)
            calls += 1
        bad += compare(case, 0, backend.run(case, 0, null_idx=True, **kw), want)
        calls += 1
    return calls, bad
