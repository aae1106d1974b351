"""Re-piecing stored piece sums to a coarser piece length (piece_repiece.hip, repiece_math.hpp)
at the kernel's segment, stride-pass, owner-search, wave-stride, sums-layout and 64-bit distance
edges: the cases, their expectations and the comparison, shared by
tests/test_gpu_repiece_matrix.py (krk_repiece_batch_dev on the production library) and
tests/test_repiece_matrix_cpu.py (krk_repiece_batch / krk_repiece_sums, the host forms the kernel
is documented to equal).  A helper module, not a test file.

Every blob of groups A - E is a view (offset, length) into ONE seeded random buffer of 1 MiB;
its stored sums are zlib.crc32 of its old pieces and the expected sums zlib.crc32 of its new
pieces.  Group F has no bytes: seeded random "sums", the expected values from the plain-Python
GF(2) reference tests/repiece_ref.py.  The output is prefilled with 0xFF once, every case is
called twice into the same buffers and compared whole, gaps and a spare tail included.

Groups (old pieces of PO = 16 bytes unless stated; new pieces of k old ones; kWaves 4,
kMaxBlocks 65536 of piece_repiece.hip):
 A  k <= 64, g = 64 / k new pieces a wave: k in A_K, g-1, g, g+1, 2g and 2g+1 new pieces, the
    last new piece holding 1, k-1 and k old pieces, the last old piece 1 byte, PO-1 bytes and full;
 B  k > 64, one new piece a wave, the lanes striding its old pieces by 64: k in B_K (2, 2, 2, 3
    and 65 passes), k-1, k and k+1 old pieces; a single new sum is also zlib.crc32 of the blob;
 C  empty blobs before, between and after the others (the owner search's tie rule), a batch of
    empty blobs only, blobs shorter than one old piece;
 D  263,000 blobs of 1 .. 3 new pieces, k = 2, 276 of them empty: more units than kMaxBlocks *
    kWaves, so the waves stride;
 E  one batch where every blob has its own (PO in E_PO, k), sums_offset / out_offset permuted
    against blob order, with gaps, starting at 1,000;
 F  64-bit distances: PO = 2^33, k in F_K, lengths near 2^40 with a partial last piece.

`python -m tests.repiece_matrix` runs every group on the device and prints one JSON line a group;
`--host` runs them through krk_repiece_batch instead.  It exits 1 on any mismatch."""
import ctypes as C
import json
import sys
import time
import zlib

import numpy as np

from kraken_amd import _capi
from kraken_amd._capi import check, krk_repiece_blob, lib
from tests import repiece_ref as R

PO = 16
BUF_BYTES = 1 << 20
SEED = 20261020
CANARY = 0xFFFFFFFF
SPARE = 8  # sums past the batch's last, which no call may touch
GROUPS = ("A", "B", "C", "D", "E", "F")

# restated from piece_repiece.hip: beyond K_MAX_BLOCKS workgroups of K_WAVES waves (one unit a
# wave) the waves stride
K_WAVES, K_MAX_BLOCKS, LANES = 4, 1 << 16, 64
STRIDE_UNITS = K_WAVES * K_MAX_BLOCKS

A_K = (1, 2, 3, 4, 5, 21, 22, 31, 32, 33, 63, 64)
B_K = (65, 127, 128, 129, 4097)
B_PASSES = (2, 2, 2, 3, 65)
D_BLOBS = 263_000
D_TEMPLATES = 1021
E_PO = (1, 3, 16, 4096)
E_K = (1, 2, 3, 5, 7, 21, 33, 64, 65, 129, 200)
F_PO = 1 << 33
F_K = (3, 129)
F_LENGTHS = ((1 << 40) - 12345, (1 << 40) + 1, (1 << 40) + (1 << 33) + 777, (1 << 41) + 5)

REPIECE_DTYPE = np.dtype([("length", "<i8"), ("piece_length", "<i8"), ("new_piece_length", "<i8"),
                          ("sums_offset", "<u8"), ("out_offset", "<u8")])
assert REPIECE_DTYPE.itemsize == C.sizeof(krk_repiece_blob)


def make_buffer():
    return np.random.default_rng(SEED).integers(0, 256, size=BUF_BYTES, dtype=np.uint8)


def units_of(n_new, k):
    """The kernel's units of a blob: g = 64 / k new pieces a unit for k <= 64, else one."""
    g = np.where(k <= LANES, LANES // np.minimum(k, LANES), 1)
    return (n_new + g - 1) // g


class Batch:
    """Blobs as columns (L, po, k), where their stored sums lie in `old` (sums_off) and their new
    ones in the output (out_off), and `want`: the whole output -- 0xFF where no sum lies."""

    def __init__(self, label, L, po, k, old_sums, new_sums, order=None, gap=False, start=0, rng=None):
        self.label = label
        self.L, self.po, self.k = (np.asarray(x, dtype=np.int64) for x in (L, po, k))
        self.n = self.L.size
        self.n_old = (self.L + self.po - 1) // self.po
        self.n_new = (self.L + self.po * self.k - 1) // (self.po * self.k)
        assert [len(s) for s in old_sums] == self.n_old.tolist() and [len(s) for s in new_sums] == self.n_new.tolist()
        self.units = int(units_of(self.n_new, self.k).sum())
        order = np.arange(self.n) if order is None else np.asarray(order)
        self.sums_off, self.out_off = np.zeros(self.n, dtype=np.int64), np.zeros(self.n, dtype=np.int64)
        a = b = start
        for pos, i in enumerate(order.tolist()):
            self.sums_off[i], self.out_off[i] = a, b
            a += int(self.n_old[i]) + (1 + pos % 5 if gap else 0)
            b += int(self.n_new[i]) + (1 + pos % 3 if gap else 0)
        rng = rng or np.random.default_rng(SEED + 99)
        self.old = rng.integers(0, 1 << 32, size=a + SPARE, dtype=np.uint64).astype(np.uint32)  # the gaps: noise
        self.want = np.full(b + SPARE, CANARY, dtype=np.uint32)
        for i in range(self.n):
            if self.n_old[i]:
                self.old[self.sums_off[i]:self.sums_off[i] + self.n_old[i]] = old_sums[i]
                self.want[self.out_off[i]:self.out_off[i] + self.n_new[i]] = new_sums[i]
        self.old.setflags(write=False)
        self.want.setflags(write=False)

    def blob_array(self):
        a = np.zeros(max(self.n, 1), dtype=REPIECE_DTYPE)
        a["length"][:self.n], a["piece_length"][:self.n] = self.L, self.po
        a["new_piece_length"][:self.n] = self.po * self.k
        a["sums_offset"][:self.n], a["out_offset"][:self.n] = self.sums_off, self.out_off
        return a


class _Bytes:
    """zlib.crc32 piece sums of views into the buffer, each (offset, length, piece) once."""

    def __init__(self, host):
        self.mv, self.memo = memoryview(host), {}

    def sums(self, off, L, piece):
        key = (off, L, piece)
        v = self.memo.get(key)
        if v is None:
            v = self.memo[key] = np.array([zlib.crc32(self.mv[a:min(a + piece, off + L)])
                                           for a in range(off, off + L, piece)], dtype=np.uint32)
        return v


def _from_bytes(label, host, blobs, **layout):
    """A Batch of blobs [(offset, L, po, k)]: old and new sums by zlib.crc32 over the bytes."""
    z = _Bytes(host)
    assert all(0 <= o and o + L <= BUF_BYTES for o, L, _, _ in blobs)
    return Batch(label, [b[1] for b in blobs], [b[2] for b in blobs], [b[3] for b in blobs],
                 [z.sums(o, L, po) for o, L, po, k in blobs], [z.sums(o, L, po * k) for o, L, po, k in blobs], **layout)


def _length(n_new, k, last_olds, tail, po=PO):
    """A blob of n_new new pieces whose last holds last_olds old pieces, the last of `tail` bytes."""
    return 0 if n_new <= 0 else ((n_new - 1) * k + last_olds - 1) * po + tail


# ------------------------------------------------------------------ the groups' batches
def shapes_a(k):
    """[(n_new, old pieces of the last new piece, bytes of the last old piece)] of one k."""
    g = LANES // k
    out = []
    for n_new in (g - 1, g, g + 1, 2 * g, 2 * g + 1):
        for last_olds in sorted({1, max(k - 1, 1), k}):
            for tail in (1, PO - 1, PO):
                out.append((n_new, last_olds, tail))
    return out


def batches_a(host):
    rng = np.random.default_rng(SEED + 1)
    out = []
    for k in A_K:
        Ls = [_length(n, k, m, t) for n, m, t in shapes_a(k)]
        blobs = [(int(rng.integers(0, BUF_BYTES - L + 1)), L, PO, k) for L in Ls]
        out.append(_from_bytes(f"A k={k}", host, blobs))
    return out


def batches_b(host):
    rng = np.random.default_rng(SEED + 2)
    out = []
    for k, passes in zip(B_K, B_PASSES):
        assert (k + LANES - 1) // LANES == passes
        blobs = []
        for n_old in (k - 1, k, k + 1):
            for tail in (1, PO):
                L = (n_old - 1) * PO + tail
                blobs.append((int(rng.integers(0, BUF_BYTES - L + 1)), L, PO, k))
        b = _from_bytes(f"B k={k}", host, blobs)
        for (o, L, _, _), n_new, oo in zip(blobs, b.n_new.tolist(), b.out_off.tolist()):
            if n_new == 1:  # the single sum is the blob's whole CRC-32
                assert int(b.want[oo]) == zlib.crc32(memoryview(host)[o:o + L])
        out.append(b)
    return out


C_LAYOUTS = {
    # (L, k): empty blobs before, between and after; blobs shorter than one old piece
    "mixed": ((0, 2), (0, 65), (0, 1), (5 * PO, 2), (0, 3), (0, 200), (64 * PO + 3, 1), (0, 2), (130 * PO, 65),
              (7, 4), (0, 1), (PO - 1, 129), (1, 1), (0, 64), (0, 7)),
    "empty only": ((0, 1), (0, 2), (0, 64), (0, 65), (0, 4097)),
    "shorter than a piece": ((1, 2), (PO - 1, 64), (PO - 1, 65), (PO, 3)),
}


def batches_c(host):
    rng = np.random.default_rng(SEED + 3)
    return [_from_bytes(f"C {name}", host, [(int(rng.integers(0, BUF_BYTES - L + 1)), L, PO, k) for L, k in lay])
            for name, lay in C_LAYOUTS.items()]


def empty_d():
    i = np.arange(D_BLOBS)
    e = i % 1000 == 999
    e[:3] = e[-3:] = True
    e[131072:131076] = e[262143:262147] = True
    return e


def batch_d(host):
    """Blobs drawn from D_TEMPLATES (offset, length) shapes, assembled with numpy; contiguous."""
    rng = np.random.default_rng(SEED + 4)
    z, k = _Bytes(host), 2
    t_new = 1 + np.arange(D_TEMPLATES) % 3
    t_L = (t_new - 1) * k * PO + rng.integers(1, k * PO + 1, D_TEMPLATES)  # a last new piece of 1 .. 32 bytes
    t_off = rng.integers(0, BUF_BYTES - 3 * k * PO, D_TEMPLATES)
    t_old = np.zeros((D_TEMPLATES, 3 * k), dtype=np.uint32)
    t_want = np.zeros((D_TEMPLATES, 3), dtype=np.uint32)
    for t in range(D_TEMPLATES):
        o, n = z.sums(int(t_off[t]), int(t_L[t]), PO), z.sums(int(t_off[t]), int(t_L[t]), k * PO)
        t_old[t, :o.size], t_want[t, :n.size] = o, n
    pick = rng.integers(0, D_TEMPLATES, D_BLOBS)
    b = Batch.__new__(Batch)
    b.label, b.n = "D", D_BLOBS
    b.L = np.where(empty_d(), 0, t_L[pick]).astype(np.int64)
    b.po, b.k = np.full(D_BLOBS, PO, dtype=np.int64), np.full(D_BLOBS, k, dtype=np.int64)
    b.n_old, b.n_new = (b.L + PO - 1) // PO, (b.L + k * PO - 1) // (k * PO)
    b.units = int(units_of(b.n_new, b.k).sum())
    b.sums_off = np.concatenate([[0], np.cumsum(b.n_old)[:-1]]).astype(np.int64)
    b.out_off = np.concatenate([[0], np.cumsum(b.n_new)[:-1]]).astype(np.int64)
    old = np.full(int(b.n_old.sum()) + SPARE, 0x5A5A5A5A, dtype=np.uint32)
    want = np.full(int(b.n_new.sum()) + SPARE, CANARY, dtype=np.uint32)
    for j in range(3 * k):
        m = b.n_old > j
        old[b.sums_off[m] + j] = t_old[pick[m], j]
    for j in range(3):
        m = b.n_new > j
        want[b.out_off[m] + j] = t_want[pick[m], j]
    b.old, b.want = old, want
    # the waves stride only past kMaxBlocks * kWaves units: say so instead of passing hollow if
    # piece_repiece.hip's constants (restated above) change
    assert b.units > STRIDE_UNITS, "group D no longer makes the waves stride"
    return b


def blobs_e():
    """[(L, po, k)]: two whole new pieces and a partial third, for every (po, k) that fits."""
    out = [(0, 16, 2)]
    for po in E_PO:
        for k in E_K:
            L = 2 * po * k + po * (k // 2) + max(po // 2, 1)
            if L <= BUF_BYTES // 8:
                out.append((L, po, k))
        out.append((0, po, 65))
    return out


def batch_e(host):
    rng = np.random.default_rng(SEED + 5)
    shapes = blobs_e()
    blobs = [(int(rng.integers(0, BUF_BYTES - L + 1)), L, po, k) for L, po, k in shapes]
    return _from_bytes("E", host, blobs, order=rng.permutation(len(blobs)), gap=True, start=1000, rng=rng)


def batch_f():
    rng = np.random.default_rng(SEED + 6)
    L, po, k, old, new = [], [], [], [], []
    for kk in F_K:
        for length in F_LENGTHS:
            n_old = R.num_pieces(length, F_PO)
            s = rng.integers(0, 1 << 32, size=n_old, dtype=np.uint64).astype(np.uint32)
            L.append(length), po.append(F_PO), k.append(kk), old.append(s)
            new.append(np.array(R.repiece(s.tolist(), length, F_PO, kk * F_PO), dtype=np.uint32))
    return Batch("F", L, po, k, old, new, order=rng.permutation(len(L)), gap=True, start=1000, rng=rng)


def batches(group, host):
    if group == "A":
        return batches_a(host)
    if group == "B":
        return batches_b(host)
    if group == "C":
        return batches_c(host)
    if group == "D":
        return [batch_d(host)]
    if group == "E":
        return [batch_e(host)]
    assert group == "F"
    return [batch_f()]


# ------------------------------------------------------------------ backends
u32p = C.POINTER(C.c_uint32)
blobp = C.POINTER(krk_repiece_blob)


class HostBackend:
    """krk_repiece_batch: no device."""

    def __init__(self):
        self.host = make_buffer()
        self.call_s = 0.0

    def close(self):
        pass

    def outputs(self, b, pinned=False):
        return np.full(b.want.size, CANARY, dtype=np.uint32)

    def call(self, b, out):
        blobs = b.blob_array()
        t0 = time.perf_counter()
        rc = lib.krk_repiece_batch(blobs.ctypes.data_as(blobp), b.n, b.old.ctypes.data_as(u32p), out.ctypes.data_as(u32p))
        self.call_s += time.perf_counter() - t0
        check(rc)
        return out.copy()


class SumsBackend(HostBackend):
    """The same batches blob by blob through krk_repiece_sums."""

    def call(self, b, out):
        t0 = time.perf_counter()
        for i in range(b.n):
            so, oo, no, nn = int(b.sums_off[i]), int(b.out_off[i]), int(b.n_old[i]), int(b.n_new[i])
            check(lib.krk_repiece_sums(b.old[so:so + no].ctypes.data_as(u32p) if no else None, no, int(b.L[i]), int(b.po[i]),
                                       int(b.po[i] * b.k[i]), out[oo:oo + nn].ctypes.data_as(u32p) if nn else None, nn))
        self.call_s += time.perf_counter() - t0
        return out.copy()


class DeviceBackend:
    """krk_repiece_batch_dev: the stored sums in device memory, the output in device or
    page-locked host memory."""

    def __init__(self):
        from kraken_amd import device as D
        self.D = D
        self.host = make_buffer()
        self.call_s = 0.0

    def close(self):
        pass

    def outputs(self, b, pinned=False):
        D = self.D
        if pinned:
            out = D.PinnedArray((b.want.size,), np.uint32)
            out.a[:] = CANARY
        else:
            out = D.DeviceBuffer(4 * b.want.size)
            out.from_host(np.full(b.want.size, CANARY, dtype=np.uint32))
        out.old = D.DeviceBuffer(4 * b.old.size)  # the batch's stored sums, uploaded once
        out.old.from_host(b.old)
        return out

    def call(self, b, out):
        blobs = b.blob_array()
        t0 = time.perf_counter()
        check(lib.krk_repiece_batch_dev(blobs.ctypes.data_as(blobp), b.n, out.old.ptr, out.ptr, None))
        self.D.synchronize()
        self.call_s += time.perf_counter() - t0
        return out.a.copy() if isinstance(out, self.D.PinnedArray) else out.to_host(np.uint32, b.want.size)


# ------------------------------------------------------------------ comparison
def compare(label, b, got):
    """Mismatches as (description, got, want): one entry a blob with a wrong sum (its first), and
    one for a word outside every blob's range that was written; the first ten."""
    if got.size != b.want.size:
        return [(f"{label}: {got.size} output words, {b.want.size} expected", 0, 0)]
    diff = np.flatnonzero(got != b.want)
    if not diff.size:
        return []
    out, seen = [], set()
    order = np.argsort(b.out_off, kind="stable")
    starts = b.out_off[order]
    for w in diff.tolist():
        if len(out) >= 10:
            break
        p = int(np.searchsorted(starts, w, side="right")) - 1
        while p >= 0 and b.n_new[order[p]] == 0:
            p -= 1
        i = int(order[p]) if p >= 0 else -1
        if i >= 0 and w < b.out_off[i] + b.n_new[i]:
            if i not in seen:
                seen.add(i)
                out.append((f"{label} blob {i} (L {int(b.L[i])}, po {int(b.po[i])}, k {int(b.k[i])}, out at "
                            f"{int(b.out_off[i])}) new piece {w - int(b.out_off[i])}", int(got[w]), int(b.want[w])))
        else:
            out.append((f"{label}: output word {w}, which belongs to no blob, was written", int(got[w]), CANARY))
    return out


def run_batch(backend, b, pinned=False):
    """The batch called twice into the same 0xFF-prefilled buffers, compared whole each time."""
    out = backend.outputs(b, pinned)
    bad = []
    for nth in ("first call", "second call"):
        bad += compare(f"{b.label}, {nth}{', page-locked' if pinned else ''}", b, backend.call(b, out))
    return bad


def run_group_counted(group, backend, pinned=False):
    """(compared blobs, mismatches) of group `group` on `backend`."""
    n, bad = 0, []
    for b in batches(group, backend.host):
        bad += run_batch(backend, b, pinned)
        n += b.n
    return n, bad


# ------------------------------------------------------------------ refusals
def refusals():
    """[(what, (length, piece_length, new_piece_length), code, message or None)]: the rows a
    batch form refuses, before anything is written or launched."""
    E = _capi.KRK_EINVAL
    return [("piece length 0", (100, 0, 16), E, "piece length must be positive"),
            ("piece length negative", (100, -16, 16), E, "piece length must be positive"),
            ("new piece length 0", (100, 16, 0), E, "piece length must be positive"),
            ("new piece length negative", (100, 16, -32), E, "piece length must be positive"),
            ("not a multiple", (100, 16, 40), E, "new piece length 40 is not a multiple of piece length 16"),
            ("finer", (100, 16, 8), E, "new piece length 8 is not a multiple of piece length 16"),
            ("negative length", (-1, 16, 32), E, None)]


def refusal_batch(row):
    """A batch of three blobs whose middle one is `row`: the good ones around it may not run."""
    a = np.zeros(3, dtype=REPIECE_DTYPE)
    a[0] = (64, 16, 32, 0, 0)
    a[1] = (*row, 4, 2)
    a[2] = (48, 16, 48, 11, 9)
    return a


def main(argv):
    host = "--host" in argv
    if not host:
        from kraken_amd import device as D
        D.set_device(0)
    backend = HostBackend() if host else DeviceBackend()
    failed = False
    for g in GROUPS:
        t0, c0 = time.perf_counter(), backend.call_s
        n, bad = run_group_counted(g, backend)
        failed |= bool(bad)
        total, calls = time.perf_counter() - t0, backend.call_s - c0
        print(json.dumps({"group": g, "cases": n, "n_mismatches": len(bad), "mismatches": bad[:10],
                          "seconds": round(total, 3), "call_seconds": round(calls, 3),
                          "reference_seconds": round(total - calls, 3)}), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
