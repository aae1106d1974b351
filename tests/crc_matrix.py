"""The CRC-32 piece kernel (crc32_pieces.hip) at its lane, step, item and run edges: the
cases, their zlib expectations and the comparison, shared by tests/test_gpu_crc_matrix.py
(in process on the production library; one child a launch variant on the diag build) and
tests/test_crc_matrix_cpu.py (the same blobs through krk_piece_sums_host, no device).  A helper
module, not a test file.

Every blob is a view (offset, length) into ONE seeded random arena of 6 MiB, uploaded once;
views overlap freely (the kernel only reads) and end at least 64 bytes before the arena's end.
Expected sums are zlib.crc32 over the host copy of the view, piece by piece; every comparison
is bit-exact over every sum, and the sums buffer of the piece-sum calls carries 16 guard words
before and after the span that must keep their canary.

Groups (kSeg 64, kStep 4096, kItemBytes 262144 of kernels.hpp):
 A  one item, every step count and tail shape x ptr % 16, once as a whole piece (a run
    expanded on the device) and once as a partial piece (an explicit item), in ONE call;
 B  run expansion: pieces around 256 KiB multiples, 3 or 4 pieces a blob, alone in one call
    and again in one call together with A's blobs;
 C  item populations around the waves of a launch (16 a CU), as one run of 64-byte pieces and
    as explicit items;
 D  krk_chunks_crc_dev: blobs cut at piece and item boundaries, submitted in order, shuffled in
    one call (several waves XOR into one sum) and split over three calls;
 E  seeded krk_crc32_update_on(KRK_PLACE_GPU) against zlib.crc32(data, seed).

`python -m tests.crc_matrix` runs every group on the device and prints one JSON line a group
(the launch variant krk_crc_launch_variant reports, the case count, the first ten mismatches);
it exits 1 on any mismatch.  `--host` runs A, B and C through krk_piece_sums_host instead."""
import ctypes as C
import json
import sys
import time
import zlib
from collections import namedtuple

import numpy as np

from kraken_amd import _capi
from kraken_amd import device as D
from kraken_amd._capi import check, krk_blob, krk_chunk, lib

K_SEG, K_STEP, K_ITEM = 64, 4096, 262144
ARENA_BYTES = 6 << 20
SPARE = 64
SEED = 20261019
GUARD = 16
CANARY = 0xC0FFEE11
GROUPS = ("A", "B", "C", "D", "E")
HOST_GROUPS = ("A", "B", "C")

STEPS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 62, 63)
TAILS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 66, 127, 128, 4031, 4032, 4033, 4095)
ITEM_EDGE = (K_ITEM, K_ITEM + 1, K_ITEM + K_STEP + 3)
ALIGNS = (0, 1, 2, 3, 4, 7, 8, 12, 15)
ALIGNS_LONG = (0, 1, 15)  # s >= 62: bounds the bytes of the group
B_PIECES = (262143, 262144, 262145, 266240, 300000, 524287, 524288, 524289, 786433, (1 << 20) + 65)
B_ALIGNS = (0, 5)
C_FACTORS = ((16, -1), (16, 0), (16, 1), (32, -1), (32, 1), (48, 5), (64, 1))  # n = a * CUs + b
D_PIECES = (100000, 262145, 300001)
D_ALIGNS = (0, 5)
E_SEEDS = (0, 1, 0x80000000, 0xFFFFFFFF, 0x5EED1E57)
E_SIZES = (1, 3, 4, 63, 64, 65, 4095, 4096, 4097, 262143, 262144, 262145, 524289)

# One blob: L bytes at arena offset `off`, pieces of P bytes.
Blob = namedtuple("Blob", "off L P")


def n_pieces(b):
    return (b.L + b.P - 1) // b.P


def make_arena():
    """The arena's host copy, 16-byte aligned like the device allocation."""
    raw = np.empty(ARENA_BYTES + 16, dtype=np.uint8)
    a = raw[(-raw.ctypes.data) % 16:][:ARENA_BYTES]
    a[:] = np.random.default_rng(SEED).integers(0, 256, size=ARENA_BYTES, dtype=np.uint8)
    assert a.ctypes.data % 16 == 0
    return a


def _place(rng, L, align):
    """A seeded arena offset with off % 16 == align whose view leaves SPARE bytes."""
    top = (ARENA_BYTES - SPARE - L - align) // 16
    assert top >= 0, "the arena is too small for this view"
    return 16 * int(rng.integers(0, top + 1)) + align


def lengths_a():
    ls = [s * K_STEP + t for s in STEPS for t in TAILS if s * K_STEP + t]
    return ls + list(ITEM_EDGE)


def cases_a():
    """Group A: every length at every alignment, as a whole piece (P = L) and as a partial
    piece (P = L + 1)."""
    rng = np.random.default_rng(SEED + 1)
    out = []
    for L in lengths_a():
        for al in (ALIGNS_LONG if L // K_STEP >= 62 else ALIGNS):
            out.append(Blob(_place(rng, L, al), L, L))
            out.append(Blob(_place(rng, L, al), L, L + 1))
    return out


def cases_b():
    rng = np.random.default_rng(SEED + 2)
    return [Blob(_place(rng, L, al), L, P) for P in B_PIECES for L in (3 * P, 3 * P + 1, 4 * P - 1) for al in B_ALIGNS]


def populations(cus):
    return [1, 15, 16, 17] + [a * cus + b for a, b in C_FACTORS]


def cases_c(cus):
    """Group C: [(n, kind, blobs)], one call each: kind "run" is one blob of n 64-byte pieces
    (one run, one item a piece), kind "items" n blobs of 100 bytes with P = 101 (explicit items),
    each a different view."""
    rng = np.random.default_rng(SEED + 3)
    out = []
    for n in populations(cus):
        out.append((n, "run", [Blob(_place(rng, 64 * n, 0), 64 * n, 64)]))
        out.append((n, "items", [Blob(64 + 7 * i, 100, 101) for i in range(n)]))
    return out


def cases_d():
    rng = np.random.default_rng(SEED + 4)
    return [Blob(_place(rng, 3 * P + 777, al), 3 * P + 777, P) for P in D_PIECES for al in D_ALIGNS]


def cuts_d(b, rng):
    """Chunk boundaries of a group D blob: the multiples of 64 nearest to every piece boundary
    and to every piece start + kItemBytes, and four seeded random ones."""
    near = lambda x: (x + 32) // 64 * 64
    cuts = {near(k * b.P) for k in range(1, n_pieces(b))}
    cuts |= {near(k * b.P + K_ITEM) for k in range(n_pieces(b))}
    cuts |= {64 * int(x) for x in rng.integers(1, b.L // 64, size=4)}
    return [0] + sorted(c for c in cuts if 0 < c < b.L) + [b.L]


def cases_e():
    """Group E: (seed, n, arena offset); the offsets take every residue of 16 in turn."""
    rng = np.random.default_rng(SEED + 5)
    return [(seed, n, _place(rng, n, (3 * k + j) % 16)) for j, seed in enumerate(E_SEEDS)
            for k, n in enumerate(E_SIZES)]


# ------------------------------------------------------------------ backends
class DeviceBackend:
    """The arena in device memory; krk_piece_sums_dev."""

    def __init__(self):
        self.host = make_arena()
        self.buf = D.DeviceBuffer(ARENA_BYTES)
        assert self.buf.ptr % 16 == 0
        self.buf.from_host(self.host)
        self.base = self.buf.ptr

    def close(self):
        self.buf.free()

    def variant(self):
        v = C.c_int(-1)
        check(lib.krk_crc_launch_variant(C.byref(v)))
        return v.value

    def cus(self):
        return D.device_cus()

    def piece_sums(self, blobs, sums_off, image):
        """One call over `blobs`; the sums buffer holds `image` before it, returned after."""
        sb = D.DeviceBuffer(image.nbytes)
        try:
            sb.from_host(image)
            D.piece_sums_dev_arrays([self.base + b.off for b in blobs], [b.L for b in blobs], [b.P for b in blobs],
                                    sums_off, sb.ptr)
            D.synchronize()
            return sb.to_host(np.uint32, image.size)
        finally:
            sb.free()


class HostBackend:
    """The same views as pageable host memory through krk_piece_sums_host: no device."""

    def __init__(self, cus=256):
        self.host = make_arena()
        self.base = self.host.ctypes.data
        self._cus = cus

    def close(self):
        pass

    def variant(self):
        return None

    def cus(self):
        return self._cus

    def piece_sums(self, blobs, sums_off, image):
        n = len(blobs)
        a = np.zeros(n, dtype=D.KRK_BLOB_DTYPE)
        a["data"], a["length"] = [self.base + b.off for b in blobs], [b.L for b in blobs]
        a["piece_length"], a["sums_offset"] = [b.P for b in blobs], sums_off
        got = image.copy()
        check(lib.krk_piece_sums_host(a.ctypes.data_as(C.POINTER(krk_blob)), n, got.ctypes.data_as(C.POINTER(C.c_uint32))))
        return got


# ------------------------------------------------------------------ expectations
_WANT = {}


def expected(host, b):
    """zlib.crc32 of every piece of view b, computed once a process."""
    v = _WANT.get(b)
    if v is None:
        assert 0 <= b.off and b.off + b.L + SPARE <= ARENA_BYTES
        mv = memoryview(host)[b.off:b.off + b.L]
        v = _WANT[b] = np.array([zlib.crc32(mv[a:a + b.P]) for a in range(0, b.L, b.P)], dtype=np.uint32)
    return v


def compare(label, blobs, sums_off, got, want):
    """Mismatches of a whole sums buffer as (case description, got, want): one entry a blob with
    a wrong sum (its first wrong piece), one for a guard or gap word that changed."""
    bad = np.nonzero(got != want)[0]
    if bad.size == 0:
        return []
    starts = np.asarray(sums_off, dtype=np.int64)
    ends = starts + np.array([n_pieces(b) for b in blobs], dtype=np.int64)
    order = np.argsort(starts, kind="stable")
    out, seen = [], set()
    for i in bad:
        k = int(np.searchsorted(starts[order], i, side="right")) - 1
        j = int(order[k]) if k >= 0 else -1
        if j >= 0 and i < ends[j]:
            if j in seen:
                continue
            seen.add(j)
            b = blobs[j]
            desc = f"{label} blob {j} off={b.off} (ptr%16={b.off % 16}) L={b.L} P={b.P} piece {int(i - starts[j])}"
        else:
            desc = f"{label} word {int(i)} outside every blob's sums (guard or gap)"
        out.append((desc, int(got[i]), int(want[i])))
    return out


def piece_call(backend, blobs, label, flip=None):
    """One piece-sum call over `blobs`, their sums back to back between two guards.  flip: the
    index of a blob whose first EXPECTED sum is corrupted (the reporting's own test)."""
    offs, o = [], GUARD
    for b in blobs:
        offs.append(o)
        o += n_pieces(b)
    image = np.full(o + GUARD, CANARY, dtype=np.uint32)
    want = image.copy()
    for b, so in zip(blobs, offs):
        want[so:so + n_pieces(b)] = expected(backend.host, b)
    if flip is not None:
        want[offs[flip]] ^= 1
    got = backend.piece_sums(blobs, offs, image)
    assert got.size == want.size
    return compare(label, blobs, offs, got, want)


# ------------------------------------------------------------------ groups
def _group_a(backend, flip):
    blobs = cases_a()
    return len(blobs), piece_call(backend, blobs, "A", flip)


def _group_b(backend, flip):
    b, a = cases_b(), cases_a()
    bad = piece_call(backend, b, "B", flip)
    bad += piece_call(backend, a + b, "A+B")
    return 2 * len(b) + len(a), bad


def _group_c(backend, flip):
    n_cases, bad = 0, []
    for k, (n, kind, blobs) in enumerate(cases_c(backend.cus())):
        bad += piece_call(backend, blobs, f"C n={n} {kind}", flip if k == 0 else None)
        n_cases += len(blobs)
    return n_cases, bad


def _chunks_call(backend, sums_ptr, rows):
    """rows: (blob, sums offset, chunk start, chunk end) -> one krk_chunks_crc_dev call."""
    arr = D.chunk_array([backend.base + b.off + s for b, _, s, _ in rows], [s for _, _, s, _ in rows],
                        [e - s for _, _, s, e in rows], [b.L for b, _, _, _ in rows], [b.P for b, _, _, _ in rows],
                        [so for _, so, _, _ in rows], np.arange(len(rows)))
    check(lib.krk_chunks_crc_dev(arr.ctypes.data_as(C.POINTER(krk_chunk)), len(rows), sums_ptr, None))


def _group_d(backend, flip):
    blobs = cases_d()
    rng = np.random.default_rng(SEED + 6)
    offs, o, rows = [], GUARD, []
    for b in blobs:
        offs.append(o)
        cuts = cuts_d(b, rng)
        rows += [(b, o, s, e) for s, e in zip(cuts[:-1], cuts[1:])]
        o += n_pieces(b)
    want = np.zeros(o + GUARD, dtype=np.uint32)
    for b, so in zip(blobs, offs):
        want[so:so + n_pieces(b)] = expected(backend.host, b)
    if flip is not None:
        want[offs[flip]] ^= 1
    shuffled = [rows[i] for i in rng.permutation(len(rows))]
    ways = {"in order": [rows], "shuffled in one call": [shuffled],
            "three calls": [shuffled[0::3], shuffled[1::3], shuffled[2::3]]}
    bad = []
    sb = D.DeviceBuffer(want.nbytes)
    try:
        for way, calls in ways.items():
            sb.zero()  # the chunk calls XOR into what is there
            for call in calls:
                _chunks_call(backend, sb.ptr, call)
            D.synchronize()
            bad += compare(f"D {way} ({len(rows)} chunks)", blobs, offs, sb.to_host(np.uint32, want.size), want)
    finally:
        sb.free()
    return len(blobs) * len(ways), bad


def _group_e(backend, flip):
    cases = cases_e()
    bad = []
    for k, (seed, n, off) in enumerate(cases):
        assert off + n + SPARE <= ARENA_BYTES
        out = C.c_uint32()
        check(lib.krk_crc32_update_on(_capi.KRK_PLACE_GPU, seed, backend.host.ctypes.data + off, n, C.byref(out)))
        want = zlib.crc32(memoryview(backend.host)[off:off + n], seed) ^ (1 if flip == k else 0)
        if out.value != want:
            bad.append((f"E seed={seed:#x} n={n} off={off} (ptr%16={off % 16})", out.value, want))
    return len(cases), bad


_RUN = {"A": _group_a, "B": _group_b, "C": _group_c, "D": _group_d, "E": _group_e}


def run_group_counted(name, backend, flip=None):
    """(compared cases, mismatches) of group `name` on `backend`."""
    return _RUN[name](backend, flip)


def run_group(name, backend, flip=None):
    """The mismatches of group `name` on `backend` as (case description, got, want)."""
    return run_group_counted(name, backend, flip)[1]


def main(argv):
    host = "--host" in argv
    backend = HostBackend() if host else DeviceBackend()
    failed = False
    try:
        for g in (HOST_GROUPS if host else GROUPS):
            t0 = time.perf_counter()
            n, bad = run_group_counted(g, backend)
            failed |= bool(bad)
            print(json.dumps({"group": g, "variant": backend.variant(), "cases": n, "n_mismatches": len(bad),
                              "mismatches": bad[:10], "seconds": round(time.perf_counter() - t0, 3)}), flush=True)
    finally:
        backend.close()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
