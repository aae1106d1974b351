"""The SHA-256 host share and tail handoff (offload.cpp, batch_dev.cpp offload_split) at their
edges: the cases, the planner rates they inject, a builder and the expectations.  A helper module
for tests/test_sha_share_plan_cpu.py (the cases' plans, no device) and
tests/test_gpu_sha_share_matrix.py (the runs).

Every case carries the plan it requires -- the takeovers (blob index, GPU prefix bytes) in the host
threads' queue order, or the set of blobs hashed whole on the host -- and plan_of() asserts that
the library's planners (krk_sha_tail_plan, krk_host_offload_plan), asked the way offload_split
asks them, answer exactly that under the case's rates and threads.  The plans are deterministic in
the injected rates; with r = 2^26 B/s a GPU stream and h = 2^28 B/s a host thread the planner's
doubles are exact, and a takeover that begins when its thread has hashed H bytes has the GPU
prefix floor64(H / 4).  tail_lens() builds chain lengths forward from that rule.

Expectations come from hashlib and zlib over host bytes of a seeded numpy generator; nothing of
the library is used for them."""
import ctypes as C
import hashlib
import heapq
import json
import os
import zlib
from collections import namedtuple

import numpy as np

from kraken_amd import device as D
from kraken_amd._capi import check, krk_blob, lib

CANARY = 0xC3
SPARE_ROWS = 3   # canary rows after the last digest / piece sum, compared too
SPARE_BYTES = 64  # after the last chain of a case's data


def geometry():
    """(bytes of one device-to-host copy, buffers of an offload thread's ring, of a resumer's)."""
    c, w, r = C.c_uint64(), C.c_uint32(), C.c_uint32()
    check(lib.krk_sha_offload_geometry(C.byref(c), C.byref(w), C.byref(r)))
    return c.value, w.value, r.value


CHUNK, DEPTH, RESUMER_DEPTH = geometry()
MiB = 1 << 20

R_STREAM, H_THREAD = 1 << 26, 1 << 28  # the tail cases' model rates: h / r = 4


def tail_rates(threads):
    """Powers of two: a GPU stream 2^26 B/s, a host thread its share 2^28 B/s of the D2H rate
    (one thread's SHA-NI, 1e9 x 0.98 / 0.85, is not the binding term)."""
    return dict(sha_stream_bps=[float(R_STREAM)] * 3, d2h_bps=float(threads * H_THREAD), h2d_bps=float(1 << 34),
                host_sha_bps=1e9, host_crc_bps=1e10, host_copy_bps=1e10, cus=256)


def whole_rates(big, longest_short):
    """Rates under which offload_plan takes exactly the `big` blobs of a batch whose other chains are
    at most longest_short bytes: the host's side is its bytes over the D2H rate (SHA-NI priced at
    1e12 B/s vanishes), and that rate lets the big blobs end just before the GPU's longest short
    chain (2^20 B/s a stream) and one more short chain end just after it.  Tails gain nothing: the
    host's bytes bind either way, and a prefix saves 2^20 / d2h of a tail."""
    r = float(1 << 20)
    g = longest_short / r
    return dict(sha_stream_bps=[r] * 3, d2h_bps=(sum(big) + longest_short / 2) / g, h2d_bps=float(1 << 34),
                host_sha_bps=1e12, host_crc_bps=1e12, host_copy_bps=1e12, cus=256)


def tail_lens(threads, tails):
    """Forward construction of a tail-handoff batch under tail_rates(threads): chain k is taken over
    by the thread that frees first, which has hashed H bytes by then (H / h seconds), so the GPU's
    prefix is start = floor64(r H / h) = floor64(H / 4) and the chain is start + tails[k] bytes long.
    The first `threads` chains start at 0.  Returns (lengths, starts), longest first as the planner
    walks them; the lengths must come out strictly descending."""
    free = [0] * threads
    lens, starts = [], []
    for tau in tails:
        t = heapq.heappop(free)
        y = t // 4 // 64 * 64
        lens.append(y + tau)
        starts.append(y)
        heapq.heappush(free, t + tau)
    assert all(a > b for a, b in zip(lens, lens[1:])), ("not descending", lens)
    return lens, starts


# A case: blob lengths, host threads, planner rates, and the required plan -- `tails`: the takeovers
# [(blob index, GPU prefix)] in the host queue's order (ascending prefix, stable over longest
# first), or None with `whole`: the set of blobs the host hashes whole (empty: no share).
# piece_lengths: the metainfo_digest runs; aligns: ptr % 16 of chain i is aligns[i % len(aligns)].
Case = namedtuple("Case", "name lens threads rates tails whole piece_lengths aligns")


def place(n, where, chain_lens, others):
    """n blob lengths: chain_lens[k] at index where[k], `others` in order in the remaining slots."""
    assert len(where) == len(chain_lens) == len(set(where)) and len(where) + len(others) == n
    lens = [None] * n
    for i, L in zip(where, chain_lens):
        lens[i] = L
    it = iter(others)
    return [next(it) if L is None else L for L in lens]


def queue_of(where, starts):
    """The host queue of takeovers listed longest first: stable by ascending GPU prefix."""
    return sorted(zip(where, starts), key=lambda p: p[1])


def tail_case(name, threads, tails, where, others, piece_lengths=(64,), aligns=(0,)):
    lens, starts = tail_lens(threads, tails)
    n = len(where) + len(others)
    return Case(name, place(n, where, lens, others), threads, tail_rates(threads), queue_of(where, starts), None,
                tuple(piece_lengths), tuple(aligns))


# ---------------------------------------------------------------- block edges (one thread, bytes)
# Chain 0 starts at 0 and is 256 m bytes, so the next takeover's prefix is 64 m exactly and a
# one-byte tail cannot end on the GPU first; a short last tail needs the host's bytes before it to
# be a multiple of 256 for the same reason (test_sha_share_plan_cpu.py shows the condition).  Every
# batch holds a chain the GPU keeps, an empty blob and a one-byte blob.
BLOCK_EDGE_CASES = [
    # [300, 200, 64] of the planner's hand check: prefix 64, tail 136
    tail_case("b-136", 1, [300, 136], [0, 1], [64, 0, 1]),
    tail_case("b-55", 1, [256, 55], [1, 3], [3, 0, 1]),
    tail_case("b-63", 1, [256, 63], [3, 0], [1, 3, 0]),
    tail_case("b-56-64", 1, [1024, 512, 64, 56], [4, 0, 2, 6], [17, 0, 1]),
    tail_case("b-65", 1, [1024, 512, 65], [0, 2, 5], [0, 33, 1]),
    tail_case("b-1", 1, [1024, 256, 1], [2, 4, 1], [1, 0, 9]),
]
SMALLEST_BLOCK_EDGE = "b-55"

# ------------------------------------------------------------------ chunk edges (CHUNK = C bytes)
C_ = CHUNK
P_ODD = 3 * MiB + 4097  # does not divide C


def _head(tau):
    """The shortest first chain (a multiple of 256) that stays longer than a takeover behind it
    with tail tau: L0 > L0 / 4 + tau."""
    return (4 * tau // 3 // 256 + 1) * 256


CHUNK_EDGE_CASES = [
    tail_case("c-3C+1", 1, [_head(3 * C_ + 1), 3 * C_ + 1], [1, 0], [4096, 0], (MiB, P_ODD), (3, 8)),
    tail_case("c-2C+1-C+1", 1, [_head(2 * C_ + 1), 2 * C_ + 1, C_ + 1], [2, 0, 1], [1, 100], (MiB, P_ODD), (0, 5)),
    tail_case("c-2C-C", 1, [_head(2 * C_), 2 * C_, C_], [0, 1, 3], [63], (MiB, P_ODD), (15, 0)),
    tail_case("c-C-1-C-64", 2, [_head(C_) + 64, _head(C_), C_ - 1, C_ - 64], [3, 1, 0, 4], [0, 65], (MiB, P_ODD),
              (1, 0)),
]

# ----------------------------------------------------------------------------- queue against slots
# More takeovers than threads; their blob indices neither ascending nor adjacent, GPU-only chains
# and empty blobs between them; the queue (ascending prefix) differs from the slot order.
QUEUE_CASES = [
    tail_case("q-t1", 1, [1536, 768, 448, 200], [7, 2, 9, 4], [5, 0, 40, 0, 1, 77, 0]),
    tail_case("q-t2", 2, [2048, 1536, 1024, 800, 600, 300], [10, 3, 8, 0, 12, 5], [0, 30, 1, 0, 99, 0, 64, 2]),
]

# -------------------------------------------------------------------------------- pointer alignment
ALIGN_CASES = [tail_case("a-%d" % a, 1, [300, 136], [0, 1], [64, 0, 1], aligns=(a,)) for a in range(16)]

# ------------------------------------------- threads at or above the chains that would be taken
# Every takeover would start at 0: tail_plan's batch end equals the whole-blob plan's, which the
# 5 % rule keeps.
_b136 = BLOCK_EDGE_CASES[0].lens
FALLBACK_CASES = [
    Case("f-t2", _b136, 2, tail_rates(2), None, {0, 1}, (64,), (0,)),
    Case("f-t3", _b136, 3, tail_rates(3), None, {0, 1, 2}, (64,), (0,)),
    # a D2H rate below one GPU stream's: the host cannot end any chain sooner
    Case("f-none", _b136, 4, dict(tail_rates(4), d2h_bps=float(1 << 25)), None, set(), (64,), (0,)),
]

# --------------------------------------------------------------------------------------- whole blobs
WHOLE_BIG = [C_ - 1, C_, C_ + 1, 2 * C_ - 1, 2 * C_, 2 * C_ + 1, 3 * C_, 3 * C_ + 1, 4 * C_ + 13]
_SHORT = [65536 - 7 * i for i in range(200)]
_WHOLE_LENS = [0, 1] + WHOLE_BIG[:4] + _SHORT[:100] + WHOLE_BIG[4:] + _SHORT[100:] + [63, 64]
_WHOLE_SET = {i for i, L in enumerate(_WHOLE_LENS) if L in WHOLE_BIG}
WHOLE_THREADS = [1, 3, len(WHOLE_BIG) + 3]
WHOLE_CASES = [Case("w-t%d" % t, _WHOLE_LENS, t, whole_rates(WHOLE_BIG, max(_SHORT)), None, _WHOLE_SET,
                    (MiB,), (0, 3)) for t in WHOLE_THREADS]

# A host share that ends long before the GPU's part: one blob of two chunks on the host (a few ms)
# beside 4 MiB chains the GPU keeps (tens of ms a chain).  The call returns while the library's
# streams still run; only the joins into the caller's stream order its outputs.
_GPU_LONG = [4 * MiB + 3, C_ + 1, 0, 4 * MiB, 4 * MiB - 64]
GPU_LONG_CASE = Case("w-gpu-long", _GPU_LONG, 1, whole_rates([C_ + 1], 4 * MiB + 3), None, {1}, (MiB,), (0, 7))

# ---------------------------------------------------------------------------------- pooled worker sets
# Consecutive calls of one thread whose worker set grows (2 -> 4 threads) and is then used in part (1).
POOL_CASES = [QUEUE_CASES[1], tail_case("p-t4", 4, [4096, 3584, 3072, 2560, 1500, 1200, 800], [1, 8, 3, 6, 10, 0, 4],
                                        [0, 50, 1, 7]), QUEUE_CASES[0]]

TAIL_CASES = BLOCK_EDGE_CASES + CHUNK_EDGE_CASES + QUEUE_CASES + ALIGN_CASES + POOL_CASES[1:2]
ALL_CASES = TAIL_CASES + FALLBACK_CASES + WHOLE_CASES + [GPU_LONG_CASE]
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)


class settings:
    """The process-wide knobs of a case (planner rates, offload threads, SHA-256 launch plan) for a
    `with` block; all three restored after it.  offload=False (planning only, no device) leaves the
    offload threads alone."""

    def __init__(self, case, offload=True, sha_plan=0):
        self.case, self.offload, self.sha_plan = case, offload, sha_plan

    def __enter__(self):
        try:
            D.set_planner_rates(self.case.rates)
            if self.offload:
                D.set_sha_host_offload(self.case.threads)
            check(lib.krk_set_sha_plan(self.sha_plan))
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        if self.offload:  # back to what the gpu fixture sets for the session
            D.set_sha_host_offload(0)
        D.set_planner_rates(None)
        check(lib.krk_set_sha_plan(0))
        return False


def plan_of(case):
    """What offload_split decides for the case, from the library's planners under the case's rates
    and threads: ("tails", [(idx, start)]) when tail_plan is non-empty and ends the batch more than
    5 % sooner than the whole-blob plan, else ("whole", {idx}).  Asserts that it is the plan the
    case requires and returns it."""
    with settings(case, offload=False):
        idx, start, end_s, gpu_s = D.sha_tail_plan(case.lens, case.threads)
        widx, g, h = D.sha_offload_plan(case.lens, case.threads)
    tails = idx.size > 0 and end_s < 0.95 * max(g, h)
    got = ("tails", list(zip(idx.tolist(), start.tolist()))) if tails else ("whole", set(widx.tolist()))
    if case.tails is not None:
        assert got == ("tails", [tuple(p) for p in case.tails]), (case.name, got, end_s, g, h)
        for i, y in case.tails:
            assert y % 64 == 0 and y < case.lens[i], (case.name, i, y)  # a tail of 0 bytes cannot be planned
    else:
        assert got == ("whole", case.whole), (case.name, got, end_s, g, h)
    return got


def takeovers(case):
    """[(blob index, GPU prefix, tail bytes)] of a tail case, in queue order."""
    return [(i, y, case.lens[i] - y) for i, y in case.tails]


# ------------------------------------------------------------------------------------------ builder
Built = namedtuple("Built", "case host buf offs digests sums_off n_sums sums")


def build(case, seed=None, first_block=None):
    """The case's bytes in one device buffer -- chains back to back at their ptr % 16, SPARE_BYTES
    after the last -- with hashlib's digests and, per piece length, zlib's piece sums.
    first_block: {blob index: 64 bytes} written over the chain's first block before hashing."""
    if seed is None:
        seed = zlib.crc32(repr((case.lens, case.aligns)).encode())
    offs, cur = [], 0
    for i, L in enumerate(case.lens):
        o = (cur + 15) // 16 * 16 + case.aligns[i % len(case.aligns)]
        offs.append(o)
        cur = o + L
    host = np.random.default_rng(seed).integers(0, 256, size=cur + SPARE_BYTES, dtype=np.uint8)
    for i, b in (first_block or {}).items():
        assert case.lens[i] >= 64 and len(b) == 64
        host[offs[i]:offs[i] + 64] = np.frombuffer(bytes(b), dtype=np.uint8)
    buf = D.DeviceBuffer(host.size)
    assert buf.ptr % 16 == 0
    buf.from_host(host)
    hb = host.tobytes()
    digests = np.frombuffer(b"".join(hashlib.sha256(hb[o:o + L]).digest() for o, L in zip(offs, case.lens)),
                            dtype=np.uint8).reshape(-1, 32)
    sums_off, n_sums, sums = {}, {}, {}
    for P in case.piece_lengths:
        cnt = [(L + P - 1) // P for L in case.lens]
        so = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
        s = np.array([zlib.crc32(hb[o + q:o + min(q + P, L)]) for o, L in zip(offs, case.lens)
                      for q in range(0, L, P)], dtype=np.uint32)
        sums_off[P], n_sums[P], sums[P] = so[:-1], int(so[-1]), s
    return Built(case, host, buf, offs, digests, sums_off, n_sums, sums)


class Outputs:
    """Digest and sums buffers of one call, prefilled with the canary, SPARE_ROWS rows past the
    last.  read_back(stream) queues their copies into pinned host memory on the call's own stream, so
    that the stream's order is all that stands between the call and what check() compares: the
    whole buffers."""

    def __init__(self, b, P=None):
        self.b, self.P = b, P
        n = len(b.case.lens)
        self.dig = D.DeviceBuffer(32 * (n + SPARE_ROWS))
        self.dig.from_host(np.full(self.dig.nbytes, CANARY, dtype=np.uint8))
        self.h_dig = D.PinnedArray((n + SPARE_ROWS, 32), np.uint8, dma_target=True)
        self.h_dig.a[:] = 0
        self.sums = self.h_sums = None
        if P is not None:
            self.sums = D.DeviceBuffer(4 * (b.n_sums[P] + SPARE_ROWS))
            self.sums.from_host(np.full(self.sums.nbytes, CANARY, dtype=np.uint8))
            self.h_sums = D.PinnedArray((b.n_sums[P] + SPARE_ROWS,), np.uint32, dma_target=True)
            self.h_sums.a[:] = 0

    def read_back(self, stream):
        """Queue the copies of both buffers on `stream`; they are valid once it is synchronised."""
        self.h_dig.fill_from_async(self.dig, stream)
        if self.sums is not None:
            self.h_sums.fill_from_async(self.sums, stream)

    def check(self, what):
        b, n = self.b, len(self.b.case.lens)
        want = np.full((n + SPARE_ROWS, 32), CANARY, dtype=np.uint8)
        want[:n] = b.digests
        bad = np.flatnonzero((self.h_dig.a != want).any(axis=1))
        assert bad.size == 0, (what, b.case.name, "digest rows", bad.tolist(), [b.case.lens[i] for i in bad if i < n])
        if self.sums is not None:
            ws = np.full(b.n_sums[self.P] + SPARE_ROWS, CANARY * 0x01010101, dtype=np.uint32)
            ws[:b.n_sums[self.P]] = b.sums[self.P]
            bad = np.flatnonzero(self.h_sums.a != ws)
            assert bad.size == 0, (what, b.case.name, self.P, "sums words", bad[:8].tolist())

    def free(self):
        self.dig.free()
        if self.sums is not None:
            self.sums.free()


def sha256_call(b, out, stream=None):
    """krk_sha256_dev over the built case into out.dig, queued on `stream`."""
    n = len(b.case.lens)
    ptrs = (C.c_void_p * n)(*[b.buf.ptr + o for o in b.offs])
    lens = np.array(b.case.lens, dtype=np.uint64)
    check(lib.krk_sha256_dev(ptrs, lens.ctypes.data_as(C.POINTER(C.c_uint64)), n, out.dig.ptr, stream))


def metainfo_digest_call(b, out, stream=None):
    """krk_metainfo_digest_dev over the built case at piece length out.P into out.sums, out.dig."""
    n, P = len(b.case.lens), out.P
    arr = (krk_blob * n)(*[krk_blob(b.buf.ptr + o, L, P, int(so))
                           for o, L, so in zip(b.offs, b.case.lens, b.sums_off[P])])
    check(lib.krk_metainfo_digest_dev(arr, n, out.sums.ptr, out.dig.ptr, stream))


def last_tail_of(case):
    """What krk_sha_last_tail must report after a call of the case."""
    if case.tails is None:
        return {"chains": 0, "gpu_prefix_bytes": 0}
    return {"chains": len(case.tails), "gpu_prefix_bytes": sum(y for _, y in case.tails)}


# ------------------------------------------------------------------------------ sentinel collision
SENTINEL_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sha_sentinel_block.json")
SENTINEL_CASE = "b-136"  # its blob 1 is taken over at 64: the block before is the whole GPU prefix


def sentinel_fixture():
    """tools/find_sentinel_block.cpp's output: {"collision", "control"} -> (64-byte block, word index
    or -1, 8-word midstate after the block from the IV), and the note's fill."""
    with open(SENTINEL_FIXTURE) as f:
        j = json.load(f)
    out = {k: (bytes.fromhex(j[k]["block"]), j[k]["word"], tuple(int(w, 16) for w in j[k]["midstate"]), j[k]["counter"])
           for k in ("collision", "control")}
    return out, int(j["sentinel"], 16)
