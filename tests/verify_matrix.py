"""The verify kernels (piece_bitfield.hip: piece_bitfield_kernel, bitfield_count_kernel,
digest_equal_kernel) at their word, count-loop, stride, owner-search and sums-layout edges: the
cases, their expectations and the comparison, shared by tests/test_gpu_verify_matrix.py
(krk_verify_batch_dev on the production library) and tests/test_verify_matrix_cpu.py (the same
batches blob by blob through krk_piece_bitfield, the host packer the kernel is documented to
equal).  A helper module, not a test file.

Every blob is a view (offset, length) into ONE seeded random buffer of 1 MiB, uploaded once;
the krk_blob arrays are built column-wise with KRK_BLOB_DTYPE.  Expected sums are zlib.crc32
piece by piece, digests hashlib.sha256, bitfield words numpy.packbits through
tests/verify_cache.ref_words (ONE call a batch over the blobs' bits laid out at their words),
n_bad a numpy count.  A piece is made bad by flipping a bit of its EXPECTED sum.  Every output
is prefilled with 0xFF before every call and compared whole.

Groups (pieces of 16 bytes; kWaves 4, kMaxBlocks 65536 of piece_bitfield.hip):
 A  blobs of 4095 .. 12,289 pieces -- 64, 65, 128, 129 and 193 words: the count kernel's
    k += 64 loop runs a second, third and fourth pass -- all good, all bad and a chosen set;
 B  empty blobs before, between and after the others (the owner search's tie rule), a batch of
    empty blobs only (no word: the count launch alone, bits_out NULL) and one one-piece blob;
 C  263,000 blobs of 1 .. 3 pieces, 276 of them empty: more words AND more blobs than
    kMaxBlocks * kWaves, so both kernels stride;
 D  A's and B's blobs with sums_offset permuted against blob order, with gaps, and starting at
    1,000, the expected values in the gaps once 0 and once not: the results of the
    contiguous layout;
 E  1,031 blobs with digests (more than four blocks of digest_equal_kernel): one flipped bit in
    each of the 32 digest bytes decides one blob alone; device and page-locked outputs.

`python -m tests.verify_matrix` runs every group on the device and prints one JSON line a
group (cases, mismatches, seconds: host reference / device calls); it exits 1 on any mismatch.
`--host` runs A - D through krk_piece_bitfield instead."""
import ctypes as C
import hashlib
import json
import sys
import time
import zlib

import numpy as np

from kraken_amd import device as D
from kraken_amd._capi import check, krk_blob, lib
from tests.verify_cache import ref_words

P = 16
BUF_BYTES = 1 << 20
SEED = 20261019
FLIP = 0x00010000
GROUPS = ("A", "B", "C", "D", "E")
HOST_GROUPS = ("A", "B", "C", "D")

# restated from piece_bitfield.hip: beyond K_MAX_BLOCKS workgroups of K_WAVES waves (one word, or
# one blob, a wave) the waves stride
K_WAVES, K_MAX_BLOCKS = 4, 1 << 16
STRIDE_UNITS = K_WAVES * K_MAX_BLOCKS
DIGEST_BLOCK = 256

A_PIECES = (4095, 4096, 4097, 8191, 8192, 8193, 12289)
B_LAYOUTS = {"mixed": (0, 0, 0, 5, 0, 0, 64, 0, 65, 0, 0), "empty only": (0, 0, 0, 0, 0), "one piece": (1,)}
C_BLOBS = 263_000
C_BAD_SHARE = 0.07
E_BLOBS = 1031
E_PIECE = 64
E_BYTE13 = (0, 255, 256, 257, 1030)


class Batch:
    """Blobs as columns: data offsets in the buffer, lengths, pieces of P bytes, and where each
    blob's sums lie (sums_off; contiguous in blob order unless given)."""

    def __init__(self, label, off, lengths, piece=P, sums_off=None):
        self.label, self.piece = label, int(piece)
        self.off = np.asarray(off, dtype=np.int64)
        self.L = np.asarray(lengths, dtype=np.int64)
        self.n = self.L.size
        assert self.off.size == self.n and (self.off >= 0).all() and (self.off + self.L <= BUF_BYTES).all()
        self.np = (self.L + self.piece - 1) // self.piece
        self.first = np.concatenate([[0], np.cumsum(self.np)]).astype(np.int64)  # a blob's first piece, blob order
        self.pieces = int(self.first[-1])
        self.sums_off = self.first[:-1].copy() if sums_off is None else np.asarray(sums_off, dtype=np.int64)
        self.word_off = np.concatenate([[0], np.cumsum((self.np + 63) // 64)]).astype(np.int64)
        self.words = int(self.word_off[-1])
        self.blob_of = np.repeat(np.arange(self.n, dtype=np.int64), self.np)  # piece (blob order) -> blob
        self.k_of = np.arange(self.pieces, dtype=np.int64) - self.first[self.blob_of]  # ... -> piece of its blob
        self.sum_index = self.sums_off[self.blob_of] + self.k_of  # ... -> index of its sum
        assert np.unique(self.sum_index).size == self.pieces, "two pieces share a sum"
        self.exp_size = int(self.sum_index.max()) + 1 if self.pieces else 0

    def with_sums_off(self, label, sums_off):
        return Batch(f"{self.label} {label}", self.off, self.L, self.piece, sums_off)

    def blob_array(self, base):
        a = np.zeros(max(self.n, 1), dtype=D.KRK_BLOB_DTYPE)
        a["data"][:self.n] = np.where(self.L > 0, base + self.off, 0).astype(np.uint64)
        a["length"][:self.n], a["piece_length"][:self.n], a["sums_offset"][:self.n] = self.L, self.piece, self.sums_off
        return a

    def true_sums(self, host):
        """zlib.crc32 of every piece at its sum's index; 0 in the gaps.  Computed once."""
        v = getattr(self, "_true", None)
        if v is None:
            mv, p = memoryview(host), self.piece
            v = np.zeros(self.exp_size, dtype=np.uint32)
            flat = np.empty(self.pieces, dtype=np.uint32)
            j = 0
            for o, L in zip(self.off.tolist(), self.L.tolist()):
                for a in range(o, o + L, p):
                    flat[j] = zlib.crc32(mv[a:min(a + p, o + L)])
                    j += 1
            assert j == self.pieces
            v[self.sum_index] = flat
            v.setflags(write=False)
            self._true = v
        return v

    def expected(self, host, bad, gap_value=0):
        """The expected sums a caller passes: the true ones, those of the `bad` pieces (a bool a
        piece, blob order) with one bit flipped, `gap_value` where no piece's sum lies."""
        e = np.full(self.exp_size, gap_value, dtype=np.uint32)
        t = self.true_sums(host)
        e[self.sum_index] = t[self.sum_index]
        e[self.sum_index[bad]] ^= FLIP
        return e

    def want(self, bad):
        """(bitfield words, n_bad a blob) for the bad pieces, from numpy alone."""
        bits = np.zeros(self.words * 64, dtype=bool)
        bits[self.word_off[:-1][self.blob_of] * 64 + self.k_of] = ~bad
        n_bad = np.bincount(self.blob_of[bad], minlength=self.n).astype(np.uint32)
        return ref_words(bits), n_bad


def _offsets(rng, lengths):
    return np.array([int(rng.integers(0, BUF_BYTES - int(L) + 1)) for L in lengths], dtype=np.int64)


def _lengths(pieces, short):
    """Lengths of blobs of `pieces` pieces whose last piece has `short` (1 .. P) bytes."""
    pieces, short = np.asarray(pieces, dtype=np.int64), np.asarray(short, dtype=np.int64)
    return np.where(pieces > 0, (pieces - 1) * P + short, 0)


# ------------------------------------------------------------------ the groups' batches
def batch_a():
    rng = np.random.default_rng(SEED + 1)
    L = _lengths(A_PIECES, 7)
    return Batch("A", _offsets(rng, L), L)


def chosen_a(b):
    """Bad pieces 0, 63, 64, 4095, 4096, n - 1 of every blob and one in every 64-word group."""
    bad = np.zeros(b.pieces, dtype=bool)
    for i in range(b.n):
        n, f = int(b.np[i]), int(b.first[i])
        ps = {p for p in (0, 63, 64, 4095, 4096, n - 1) if p < n}
        ps |= {p for p in (4096 * g + (1237 * g + 77 + i) % 4096 for g in range((n + 4095) // 4096)) if p < n}
        bad[f + np.array(sorted(ps), dtype=np.int64)] = True
    return bad


def batches_b():
    rng = np.random.default_rng(SEED + 2)
    out = []
    for name, pieces in B_LAYOUTS.items():
        L = _lengths(pieces, [1 + (5 * i) % P for i in range(len(pieces))])
        out.append(Batch(f"B {name}", _offsets(rng, L), L))
    return out


def chosen_b(b):
    """Bad pieces 0, 4, 63 and 64 of every blob that has them."""
    bad = np.zeros(b.pieces, dtype=bool)
    for k in (0, 4, 63, 64):
        bad[b.first[:-1][b.np > k] + k] = True
    return bad


def bad_sets(b, chosen):
    return {"all good": np.zeros(b.pieces, dtype=bool), "all bad": np.ones(b.pieces, dtype=bool), "chosen": chosen(b)}


def empty_c():
    i = np.arange(C_BLOBS)
    e = i % 1000 == 999
    e[:3] = e[-3:] = True
    e[131072:131076] = e[262143:262147] = True
    return e


def batch_c():
    rng = np.random.default_rng(SEED + 3)
    i = np.arange(C_BLOBS)
    pieces = np.where(empty_c(), 0, 1 + i % 3)
    L = _lengths(pieces, P - rng.integers(0, P, C_BLOBS))  # a short last piece on most
    off = rng.integers(0, BUF_BYTES - 3 * P, C_BLOBS)
    b = Batch("C", off, L)
    # both launches stride only past kMaxBlocks * kWaves words and blobs: say so instead of
    # passing hollow if piece_bitfield.hip's constants (restated above) change
    assert b.words > STRIDE_UNITS and b.n > STRIDE_UNITS, "group C no longer makes the kernels stride"
    return b


def bad_c(b):
    return np.random.default_rng(SEED + 4).random(b.pieces) < C_BAD_SHARE


def layouts_d(b, rng):
    """[(label, sums_off)]: b's sums permuted against blob order, with gaps of 1 .. 5 sums after
    every blob, starting at 1,000, and all three at once."""
    def lay(order, gap, start):
        so, at = np.zeros(b.n, dtype=np.int64), start
        for k, i in enumerate(order):
            so[i] = at
            at += int(b.np[i]) + (1 + k % 5 if gap else 0)
        return so
    ident, perm = np.arange(b.n), rng.permutation(b.n)
    return [("permuted", lay(perm, False, 0)), ("gapped", lay(ident, True, 0)), ("from 1000", lay(ident, False, 1000)),
            ("permuted, gapped, from 1000", lay(perm, True, 1000))]


def cases_d():
    """[(batch in another sums layout, its bad pieces)]: the blobs of A and of B's mixed batch."""
    rng = np.random.default_rng(SEED + 5)
    out = []
    for base, chosen in ((batch_a(), chosen_a), (batches_b()[0], chosen_b)):
        for label, so in layouts_d(base, rng):
            b = base.with_sums_off(label, so)
            out.append((b, chosen(b)))
    return out


def batch_e():
    rng = np.random.default_rng(SEED + 6)
    L = np.arange(E_BLOBS) % 201  # 0 .. 200 bytes
    b = Batch("E", _offsets(rng, L), L, piece=E_PIECE)
    assert b.n > 4 * DIGEST_BLOCK, "group E no longer fills more than four blocks of digest_equal_kernel"
    return b


def digests_e(host, b):
    """(true digests, expected digests, want ok): blob 32 + k has bit k % 8 of digest byte k
    flipped, blobs E_BYTE13 byte 13 wrong; every other blob, the empty ones included, verifies."""
    true = np.frombuffer(b"".join(hashlib.sha256(memoryview(host)[o:o + L]).digest()
                                  for o, L in zip(b.off.tolist(), b.L.tolist())), dtype=np.uint8).reshape(-1, 32)
    exp = true.copy()
    ok = np.ones(b.n, dtype=bool)
    for k in range(32):
        exp[32 + k, k] ^= 1 << (k % 8)
        ok[32 + k] = False
    for i in E_BYTE13:
        exp[i, 13] ^= 0x5A
        ok[i] = False
    return true, exp, ok


# ------------------------------------------------------------------ backends
def make_buffer():
    return np.random.default_rng(SEED).integers(0, 256, size=BUF_BYTES, dtype=np.uint8)


class DeviceBackend:
    """The buffer in device memory; krk_verify_batch_dev."""

    def __init__(self):
        self.host = make_buffer()
        self.buf = D.DeviceBuffer(BUF_BYTES)
        self.buf.from_host(self.host)
        self.call_s = 0.0

    def close(self):
        self.buf.free()

    def verify(self, b, expected, digests=None, pinned=False, no_bits=False):
        """One call; (bits, n_bad, digest_ok or None), every output prefilled with 0xFF."""
        shapes = [(max(b.words, 1), np.uint64), (max(b.n, 1), np.uint32), (max(b.n, 1), np.uint8)]
        if pinned:
            outs = [D.PinnedArray((k,), dt) for k, dt in shapes]
            for o in outs:
                o.a.view(np.uint8)[:] = 0xFF
        else:
            outs = [D.DeviceBuffer(k * np.dtype(dt).itemsize) for k, dt in shapes]
            for o in outs:
                o.from_host(np.full(o.nbytes, 0xFF, dtype=np.uint8))
        blobs = b.blob_array(self.buf.ptr)
        exp = np.ascontiguousarray(expected, dtype=np.uint32)
        dg = None if digests is None else np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1)
        u8p, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
        assert not no_bits or b.words == 0
        t0 = time.perf_counter()
        check(lib.krk_verify_batch_dev(blobs.ctypes.data_as(C.POINTER(krk_blob)), b.n,
                                       exp.ctypes.data_as(u32p) if exp.size else None,
                                       dg.ctypes.data_as(u8p) if dg is not None else None,
                                       None if no_bits else outs[0].ptr, outs[1].ptr,
                                       outs[2].ptr if dg is not None else None, None))
        D.synchronize()
        self.call_s += time.perf_counter() - t0
        got = [o.a.copy() if pinned else o.to_host(dt, k) for o, (k, dt) in zip(outs, shapes)]
        if not pinned:
            for o in outs:
                o.free()
        return got[0][:b.words], got[1][:b.n], (got[2][:b.n] if dg is not None else None), got[0][b.words:]


class HostBackend:
    """The same batches blob by blob through krk_piece_bitfield over the true sums: no device."""

    def __init__(self):
        self.host = make_buffer()
        self.call_s = 0.0
        # the library's symbol under a prototype that takes plain addresses: one call a blob
        self._f = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p)(
            ("krk_piece_bitfield", lib))

    def close(self):
        pass

    def verify(self, b, expected, digests=None, pinned=False, no_bits=False):
        assert digests is None
        sums = b.true_sums(self.host)
        exp = np.ascontiguousarray(expected, dtype=np.uint32)
        bits = np.full(max(b.words, 1), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        n_bad = np.full(max(b.n, 1), 0xFFFFFFFF, dtype=np.uint32)
        s0, e0, b0, n0 = sums.ctypes.data, exp.ctypes.data, bits.ctypes.data, n_bad.ctypes.data
        t0 = time.perf_counter()
        for i, (so, c, w) in enumerate(zip(b.sums_off.tolist(), b.np.tolist(), b.word_off.tolist())):
            rc = self._f(s0 + 4 * so if c else None, e0 + 4 * so if c else None, c, b0 + 8 * w if c else None, n0 + 4 * i)
            assert rc == 0, (b.label, i)
        self.call_s += time.perf_counter() - t0
        return bits[:b.words], n_bad[:b.n], None, bits[b.words:]


# ------------------------------------------------------------------ comparison
def compare(label, b, got, want_bits, want_bad, want_ok=None):
    """Mismatches as (description, got, want): one entry a blob with a wrong word (its first),
    one a blob with a wrong count, one a blob with a wrong digest flag; the first ten of each."""
    bits, n_bad, ok, spare = got
    out = []
    if bits.size != want_bits.size or n_bad.size != want_bad.size:
        return [(f"{label}: {bits.size} words and {n_bad.size} counts, {want_bits.size} and {want_bad.size} expected", 0, 0)]
    if spare.size and not (spare == 0xFFFFFFFFFFFFFFFF).all():
        out.append((f"{label}: the word after the batch's last was written", int(spare[0]), 0xFFFFFFFFFFFFFFFF))
    seen = set()
    for w in np.nonzero(bits != want_bits)[0]:
        i = int(np.searchsorted(b.word_off, w, side="right")) - 1
        if i in seen or len(seen) >= 10:
            continue
        seen.add(i)
        out.append((f"{label} blob {i} ({int(b.np[i])} pieces, sums at {int(b.sums_off[i])}) word "
                    f"{int(w - b.word_off[i])} (batch word {int(w)})", int(bits[w]), int(want_bits[w])))
    for i in np.nonzero(n_bad != want_bad)[0][:10]:
        out.append((f"{label} blob {int(i)} ({int(b.np[i])} pieces) n_bad", int(n_bad[i]), int(want_bad[i])))
    if want_ok is not None:
        for i in np.nonzero(ok.astype(bool) != want_ok)[0][:10]:
            out.append((f"{label} blob {int(i)} ({int(b.L[i])} bytes) digest_ok", int(ok[i]), int(want_ok[i])))
    return out


def _run(backend, b, bad, label, gap_value=0, **kw):
    want_bits, want_bad = b.want(bad)
    return compare(label, b, backend.verify(b, b.expected(backend.host, bad, gap_value), **kw), want_bits, want_bad)


# ------------------------------------------------------------------ groups
def _group_a(backend):
    b = batch_a()
    bad = []
    for name, s in bad_sets(b, chosen_a).items():
        bad += _run(backend, b, s, f"A {name}")
    return 3 * b.n, bad


def _group_b(backend):
    n, bad = 0, []
    for b in batches_b():
        for name, s in bad_sets(b, chosen_b).items():
            bad += _run(backend, b, s, f"{b.label}, {name}")
            n += b.n
        if b.words == 0:  # no word to write: bits_out may be NULL
            bad += _run(backend, b, np.zeros(0, dtype=bool), f"{b.label}, bits_out NULL", no_bits=True)
            n += b.n
    return n, bad


def _group_c(backend):
    b = batch_c()
    return b.n, _run(backend, b, bad_c(b), "C")


def _group_d(backend):
    n, out = 0, []
    for b, bad in cases_d():
        base = Batch("contiguous", b.off, b.L, b.piece)
        want = base.want(bad)
        for gap_value in (0, 0xDEADBEEF):
            got = backend.verify(b, b.expected(backend.host, bad, gap_value))
            out += compare(f"D {b.label}, gaps {gap_value:#x}", b, got, *want)
            n += b.n
    return n, out


def _group_e(backend):
    b = batch_e()
    true, exp, want_ok = digests_e(backend.host, b)
    none = np.zeros(b.pieces, dtype=bool)
    want_bits, want_bad = b.want(none)
    out = []
    for pinned in (False, True):
        where = "page-locked outputs" if pinned else "device outputs"
        got = backend.verify(b, b.expected(backend.host, none), digests=exp, pinned=pinned)
        out += compare(f"E {where}", b, got, want_bits, want_bad, want_ok)
    got = backend.verify(b, b.expected(backend.host, none), digests=true)
    out += compare("E true digests", b, got, want_bits, want_bad, np.ones(b.n, dtype=bool))
    return 3 * b.n, out


_RUN = {"A": _group_a, "B": _group_b, "C": _group_c, "D": _group_d, "E": _group_e}


def run_group_counted(name, backend):
    """(compared blobs, mismatches) of group `name` on `backend`."""
    return _RUN[name](backend)


def main(argv):
    host = "--host" in argv
    if not host:
        D.set_device(0)
        D.set_sha_host_offload(0)  # every SHA-256 chain of group E on the device
    backend = HostBackend() if host else DeviceBackend()
    failed = False
    try:
        for g in (HOST_GROUPS if host else GROUPS):
            t0, c0 = time.perf_counter(), backend.call_s
            n, bad = run_group_counted(g, backend)
            failed |= bool(bad)
            total, calls = time.perf_counter() - t0, backend.call_s - c0
            print(json.dumps({"group": g, "cases": n, "n_mismatches": len(bad), "mismatches": bad[:10],
                              "seconds": round(total, 3), "call_seconds": round(calls, 3),
                              "reference_seconds": round(total - calls, 3)}), flush=True)
    finally:
        backend.close()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
