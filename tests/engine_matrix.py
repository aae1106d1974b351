"""The submission engine (kraken_amd/csrc/engine.cpp, with digester.cpp and piece_stream.cpp on
top of it) at its slot, block and piece edges: the
write plans, their references from hashlib and zlib, and the runner over the C ABI, shared by
tests/test_gpu_engine_matrix.py (KRK_PLACE_GPU: the engine's slot requests, state rows, portions
and fold) and tests/test_engine_matrix_cpu.py (KRK_PLACE_HOST: the same plans through
host_meta.cpp's tail buffer and the host piece loop, no device).  A helper module, not a test file.

S = 524288 is the engine's slot, B = 64 a SHA-256 block, I = 262144 kItemBytes of kernels.hpp,
Q = 8 the requests an owner keeps in flight (kSlotBytes and kOwnerInflight of engine.hpp: constants,
no switch changes them).  All data is views into ONE seeded arena; every comparison is bit-exact over every output.

A plan is a list of steps -- ("w", n) a write of n bytes, ("z", null) a zero-length write with a
NULL or a non-NULL buffer, ("s",) a sum -- over the view [off, off + total).  Every sum is compared
with hashlib.sha256 of the bytes written so far: Digest() does not reset.  A piece plan is a view,
a piece length and the sizes of its writes; n_sums and length of krk_piece_stream_end with a NULL
buffer, then every sum of a second call into a buffer with 16 canary words after `cap`, are
compared with one zlib.crc32 a piece.  The plans of a group run concurrently, one thread a plan, at
most 64 owners live at once, so the engine coalesces them into a few launches.

Groups:
 A  Digester: A1 tails (every padding residue from the IV and from a state row), A2 the slot edge
    (six totals x nine splits), A3 where the sums fall, A4 more than Q requests of one owner,
    A5 a state row reused by the next digester;
 B  piece streams: 16 piece lengths in a structural relation to S and I x totals x splits;
 C  krk_crc32_update_on around Q requests in flight (the retire-while-submitting branch);
 D  one crowd: 32 digesters, 32 piece streams and four crc32_update threads released by one
    barrier; the engine must have coalesced them (krk_engine_stats), else it proved nothing;
 E  A2, A3 and A4 with the slot pool at its minimum cap (in a fresh process: `--pend`).
    SlotPool::try_acquire returns no slot while free + growable <= reserve, and the reserve is at
    least the 16 slots of one chunk, which is all the minimum cap allows: free + growable never
    exceeds 16, so no digester ever fills a slot in place, every pending byte sits in the pageable
    pend buffer and krk_digester_sum takes its no-slot branch.  (This follows from the code, it is
    not an observation.)

`python -m tests.engine_matrix` runs A to D on the device and prints one JSON line a group (the
case count, bytes moved, seconds, the first ten mismatches); it exits 1 on any mismatch.  `--host`
runs A, B and C on the host placement, `--pend` is group E's child."""
import ctypes as C
import hashlib
import json
import sys
import threading
import time
import zlib
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from kraken_amd import _capi
from kraken_amd._capi import KRK_PLACE_GPU, KRK_PLACE_HOST, check, lib

S, B, I, Q = 524288, 64, 262144, 8
SEED = 20261020
ARENA_BYTES = 12 * S + 4096
MAX_LIVE = 64
GUARD = 16
CANARY = 0xC0FFEE11
GROUPS = ("A", "B", "C", "D")
HOST_GROUPS = ("A", "B", "C")

# What a group may move and ask of its reference (asserted in tests/test_engine_matrix_cpu.py).
CAP_A_BYTES = 192 << 20
CAP_B_BYTES = 256 << 20
CAP_B_CRC_CALLS = 3_000_000
CAP_C_BYTES = 64 << 20

A1_IV = tuple(range(131))                         # final-only requests from the IV
A1_ROW = tuple(range(64)) + (119, 120)            # one slot, then a final of r bytes from the row
A2_TOTALS = (S - 1, S, S + 1, 2 * S, 2 * S + 1, 3 * S + 17)
A2_SPLITS = ("whole", "1+rest", "S-1+rest", "S-1+1+rest", "S+rest", "S+1+rest", "63+1+rest", "130x1+rest", "zeros")
A3_SPLITS = ("S-1+1+rest", "1+rest")
A4_TOTAL = (Q + 2) * S + 1
# (S / 2 is I: sixteen distinct piece lengths)
B_PIECES = tuple(dict.fromkeys((1, 3, 63, 64, 65, 4096, 65536, I - 1, I, I + 1, S // 2, S - 1, S, S + 1, 2 * S,
                                2 * S + 1, 4 * S)))
B_TOTAL_CAP = 3 * S + 17
B_SMALL_P_CAP = S + 3                             # P <= 3: the reference is one zlib.crc32 call a piece
B_SPLITS = ("whole", "S", "1+rest", "P")
C_SIZES = (Q * S - 1, Q * S, Q * S + 1, (Q + 1) * S + 5, 12 * S)
C_SEEDS = (0, 1, 0x80000000, 0xFFFFFFFF)
E_LIVE = 40

# A digester plan: `steps` over the arena view [off, off + total).
Plan = namedtuple("Plan", "name off total steps")
# A piece plan: the view, the piece length, the write sizes; erange: also ask with cap = n_sums - 1.
PiecePlan = namedtuple("PiecePlan", "name off total P writes erange")
# A crc32_update case.
CrcCase = namedtuple("CrcCase", "seed off n")

W = lambda n: ("w", n)
Z_NULL, Z_PTR, SUM = ("z", True), ("z", False), ("s",)


def make_arena():
    a = np.empty(ARENA_BYTES, dtype=np.uint8)
    a[:] = np.random.default_rng(SEED).integers(0, 256, size=ARENA_BYTES, dtype=np.uint8)
    return a


_ARENA = []


def arena():
    """The arena, made once a process and never written."""
    if not _ARENA:
        a = make_arena()
        a.setflags(write=False)
        _ARENA.append(a)
    return _ARENA[0]


def _place(rng, total):
    return int(rng.integers(0, ARENA_BYTES - total + 1))


def total_of(steps):
    return sum(s[1] for s in steps if s[0] == "w")


def _plan(rng, name, steps):
    steps = tuple(steps)
    t = total_of(steps)
    return Plan(name, _place(rng, t), t, steps)


def cut(total, sizes):
    """Writes of `sizes` in turn, each clipped to what is left, then the rest; none of zero bytes."""
    out, left = [], total
    for n in sizes:
        n = min(n, left)
        if n:
            out.append(n)
        left -= n
    if left:
        out.append(left)
    return out


def split_writes(total, split):
    """The write sizes of a named A2 split of `total` bytes."""
    sizes = {"whole": [], "1+rest": [1], "S-1+rest": [S - 1], "S-1+1+rest": [S - 1, 1], "S+rest": [S],
             "S+1+rest": [S + 1], "63+1+rest": [63, 1], "130x1+rest": [1] * 130, "zeros": []}[split]
    return cut(total, sizes)


# ------------------------------------------------------------------ group A
def plans_a1():
    rng = np.random.default_rng(SEED + 1)
    out = [_plan(rng, f"A1 iv r={r}", [W(r) if r else Z_PTR, SUM]) for r in A1_IV]
    out += [_plan(rng, f"A1 row r={r}", [W(S + r), SUM]) for r in A1_ROW]
    return out


def plans_a2():
    rng = np.random.default_rng(SEED + 2)
    out = []
    for T in A2_TOTALS:
        for split in A2_SPLITS:
            ws = [W(n) for n in split_writes(T, split)]
            if split == "zeros":  # before, between the write and the sums, and after
                steps = [Z_NULL, Z_PTR] + ws + [Z_PTR, Z_NULL, SUM, Z_NULL, Z_PTR, SUM]
            else:
                steps = ws + [SUM]
            out.append(_plan(rng, f"A2 T={T} {split}", steps))
    return out


def plans_a3():
    rng = np.random.default_rng(SEED + 3)
    out = []
    for T in A2_TOTALS:
        for split in A3_SPLITS:
            steps = []
            for n in split_writes(T, split):
                steps += [W(n), SUM]
            out.append(_plan(rng, f"A3 T={T} {split} sum after every write", steps))
    out.append(_plan(rng, "A3 sum; sum", [SUM, SUM]))
    out.append(_plan(rng, "A3 sum at 0, writes, sum", [SUM, W(100), W(S), SUM]))
    out.append(_plan(rng, "A3 sum at S, one byte, sum", [W(S), SUM, W(1), SUM]))
    out.append(_plan(rng, "A3 sum at 2S, one byte, sum", [W(2 * S), SUM, W(1), SUM]))
    out.append(_plan(rng, "A3 sum at S-1 pending, write(1), sum", [W(S - 1), SUM, W(1), SUM]))
    return out


def plans_a4():
    rng = np.random.default_rng(SEED + 4)
    return [_plan(rng, "A4 (Q+2)S+1 in one call", [W(A4_TOTAL), SUM]),
            _plan(rng, "A4 (Q+2)S+1 in writes of S/2+1", [W(n) for n in cut(A4_TOTAL, [S // 2 + 1] * 20)] + [SUM])]


def plans_a5():
    """Run in ONE thread with nothing else live, each digester freed before the next is made: the
    free list of state rows is LIFO, so the second gets the row the first left 2S bytes deep."""
    rng = np.random.default_rng(SEED + 5)
    return [_plan(rng, "A5 first: 2S, freed unsummed", [W(2 * S)]),
            _plan(rng, "A5 second: S+1 on the reused row", [W(S + 1), SUM]),
            _plan(rng, "A5 third: sum of nothing", [SUM])]


def plans_a():
    """The concurrent plans of group A (A5 runs after them, alone)."""
    return plans_a1() + plans_a2() + plans_a3() + plans_a4()


# ------------------------------------------------------------------ group B
def totals_b(P):
    ts = [0, 1, P - 1, P, P + 1, S, S + 1, 2 * S + P + 1]
    if S % P == 0:
        ts.append(2 * S)  # request ends and piece ends coincide
    if P <= 3:
        ts = [t for t in ts if t <= B_SMALL_P_CAP]
    out = []
    for t in ts:
        t = min(t, B_TOTAL_CAP)
        if t not in out:
            out.append(t)
    return out


def piece_writes(total, P, split):
    if split == "whole":
        return cut(total, [])
    if split == "S":
        return cut(total, [S] * (total // S))
    if split == "1+rest":
        return cut(total, [1])
    if split == "P":
        return cut(total, [P] * (total // P)) if P >= 4096 else None
    raise KeyError(split)


def plans_b():
    rng = np.random.default_rng(SEED + 6)
    out = []
    for P in B_PIECES:
        asked = False
        for T in totals_b(P):
            off = _place(rng, T)  # the splits of a total share its view and its reference
            seen = []
            for split in B_SPLITS:
                ws = piece_writes(T, P, split)
                if ws is None or ws in seen:
                    continue
                seen.append(ws)
                er = not asked and T > 0
                asked |= er
                out.append(PiecePlan(f"B P={P} T={T} {split}", off, T, P, tuple(ws), er))
    out.append(PiecePlan(f"B P={S + 1} T={A4_TOTAL} whole", _place(rng, A4_TOTAL), A4_TOTAL, S + 1, (A4_TOTAL,), False))
    return out


# ------------------------------------------------------------------ group C
def cases_c():
    """Every size with two of the seeds in turn, every seed at two sizes or more: all four seeds at
    all five sizes would move 90 MiB, over the group's cap."""
    rng = np.random.default_rng(SEED + 7)
    return [CrcCase(C_SEEDS[(k + j) % 4], _place(rng, n), n) for k, n in enumerate(C_SIZES) for j in (0, 2)]


# ------------------------------------------------------------------ group D
def crowd_d():
    """(32 digester plans, 32 piece plans): every split shape of A2, A3's sum plans, every P of B."""
    a2, a3, b = plans_a2(), plans_a3(), plans_b()
    dig = a3 + [p for p in a2 if p.total != 3 * S + 17 or "130x1" in p.name][:: 2]
    dig = dig[:32]
    per_p = [max((p for p in b if p.P == P), key=lambda p: (p.total, len(p.writes))) for P in B_PIECES]
    rest = [p for p in b if p not in per_p and p.total >= S][:: 5]
    return dig, (per_p + rest)[:32]


# ------------------------------------------------------------------ references
_SHA, _CRC = {}, {}


def want_digests(p):
    """hashlib.sha256 of the bytes written before each sum of plan p, computed once a process."""
    key = (p.off, p.steps)
    v = _SHA.get(key)
    if v is None:
        mv, h, pos, v = memoryview(arena()), hashlib.sha256(), p.off, []
        for s in p.steps:
            if s[0] == "w":
                h.update(mv[pos:pos + s[1]])
                pos += s[1]
            elif s[0] == "s":
                v.append(h.copy().digest())
        _SHA[key] = v
    return v


def want_sums(p):
    """zlib.crc32 of every piece of the view of piece plan p, computed once a process."""
    key = (p.off, p.total, p.P)
    v = _CRC.get(key)
    if v is None:
        mv = memoryview(arena())[p.off:p.off + p.total]
        v = _CRC[key] = np.array([zlib.crc32(mv[a:a + p.P]) for a in range(0, p.total, p.P)], dtype=np.uint32)
    return v


def crc_calls_b(plans):
    return sum(-(-t // P) for (_, t, P) in {(p.off, p.total, p.P) for p in plans})


# ------------------------------------------------------------------ runners
def run_digester(p, placement, flip=False, before_write=None):
    """Plan p on one digester: mismatches as (description, got, want)."""
    base = arena().ctypes.data
    want = want_digests(p)
    h = C.c_void_p()
    check(lib.krk_digester_new_on(placement, C.byref(h)))
    bad, pos, k = [], p.off, 0
    out = (C.c_uint8 * 32)()
    try:
        where = C.c_int(-1)
        check(lib.krk_digester_placement(h, C.byref(where)))
        if where.value != placement:
            bad.append((f"{p.name}: placement", where.value, placement))
        for s in p.steps:
            if s[0] == "w":
                if before_write:
                    before_write()
                check(lib.krk_digester_write(h, base + pos, s[1]))
                pos += s[1]
            elif s[0] == "z":
                check(lib.krk_digester_write(h, None if s[1] else base + pos, 0))
            else:
                C.memset(out, 0xAA, 32)
                check(lib.krk_digester_sum(h, out))
                w = want[k]
                if flip and k == 0:
                    w = bytes([w[0] ^ 1]) + w[1:]
                if bytes(out) != w:
                    bad.append((f"{p.name}: sum {k} after {pos - p.off} bytes (off={p.off})", bytes(out).hex(), w.hex()))
                k += 1
    finally:
        lib.krk_digester_free(h)
    return bad


def run_piece(p, placement, flip=False):
    base = arena().ctypes.data
    want = want_sums(p)
    if flip:
        want = want.copy()
        want[0] ^= 1
    s = C.c_void_p()
    check(lib.krk_piece_stream_begin_on(placement, p.P, C.byref(s)))
    bad = []
    try:
        where = C.c_int(-1)
        check(lib.krk_piece_stream_placement(s, C.byref(where)))
        if where.value != placement:
            bad.append((f"{p.name}: placement", where.value, placement))
        pos = p.off
        for n in p.writes:
            check(lib.krk_piece_stream_update(s, base + pos, n))
            pos += n
        n_sums, length = C.c_uint64(1 << 60), C.c_uint64(1 << 60)
        check(lib.krk_piece_stream_end(s, None, 0, C.byref(n_sums), C.byref(length)))
        if (n_sums.value, length.value) != (want.size, p.total):
            bad.append((f"{p.name}: (n_sums, length)", [n_sums.value, length.value], [int(want.size), p.total]))
            return bad
        n = int(want.size)
        if p.erange:  # a buffer one sum short: refused, the count still reported, nothing written
            buf = np.full(n - 1 + GUARD, CANARY, dtype=np.uint32)
            n2 = C.c_uint64(1 << 60)
            rc = lib.krk_piece_stream_end(s, buf.ctypes.data_as(C.POINTER(C.c_uint32)), n - 1, C.byref(n2), None)
            if rc != _capi.KRK_ERANGE or n2.value != n or not (buf[n - 1:] == CANARY).all():
                bad.append((f"{p.name}: cap = n_sums - 1", [rc, n2.value], [_capi.KRK_ERANGE, n]))
        buf = np.full(n + GUARD, CANARY, dtype=np.uint32)
        n2, l2 = C.c_uint64(1 << 60), C.c_uint64(1 << 60)
        check(lib.krk_piece_stream_end(s, buf.ctypes.data_as(C.POINTER(C.c_uint32)), n, C.byref(n2), C.byref(l2)))
        if (n2.value, l2.value) != (n, p.total):
            bad.append((f"{p.name}: second end (n_sums, length)", [n2.value, l2.value], [n, p.total]))
        if not (buf[n:] == CANARY).all():
            bad.append((f"{p.name}: canary after cap", buf[n:].tolist(), [CANARY] * GUARD))
        ne = np.nonzero(buf[:n] != want)[0]
        if ne.size:
            i = int(ne[0])
            bad.append((f"{p.name}: piece {i} of {n} ({ne.size} wrong, off={p.off}, writes={list(p.writes)[:4]}...)",
                        int(buf[i]), int(want[i])))
    finally:
        lib.krk_piece_stream_free(s)
    return bad


def run_crc(c, placement, flip=False):
    a = arena()
    out = C.c_uint32()
    check(lib.krk_crc32_update_on(placement, c.seed, a.ctypes.data + c.off, c.n, C.byref(out)))
    want = zlib.crc32(memoryview(a)[c.off:c.off + c.n], c.seed) ^ (1 if flip else 0)
    return [] if out.value == want else [(f"C seed={c.seed:#x} n={c.n} off={c.off}", out.value, want)]


def _concurrently(jobs, live=MAX_LIVE):
    """jobs: callables returning mismatch lists; one thread a job, at most `live` at once."""
    if not jobs:
        return []
    with ThreadPoolExecutor(min(live, len(jobs))) as ex:
        futs = [ex.submit(j) for j in jobs]
        return [m for f in futs for m in f.result()]


def _bytes(plans):
    return sum(p.total for p in plans)


def _group_a(placement, flip):
    plans = plans_a()
    for p in plans + plans_a5():
        want_digests(p)  # the references first: the run itself is the engine's
    t0 = time.perf_counter()
    bad = _concurrently([lambda p=p, k=k: run_digester(p, placement, flip and k == 0) for k, p in enumerate(plans)])
    a5 = plans_a5()
    for p in a5:
        bad += run_digester(p, placement)
    return len(plans) + len(a5), _bytes(plans + a5), time.perf_counter() - t0, bad


def _group_b(placement, flip):
    plans = plans_b()
    for p in plans:
        want_sums(p)
    t0 = time.perf_counter()
    bad = _concurrently([lambda p=p, k=k: run_piece(p, placement, flip and k == 1) for k, p in enumerate(plans)])
    return len(plans), _bytes(plans), time.perf_counter() - t0, bad


def _group_c(placement, flip):
    cases = cases_c()
    t0 = time.perf_counter()
    bad = []
    for k, c in enumerate(cases):
        bad += run_crc(c, placement, flip and k == 0)
    return len(cases), sum(c.n for c in cases), time.perf_counter() - t0, bad


def engine_stats():
    v = [C.c_uint64() for _ in range(5)]
    check(lib.krk_engine_stats(*[C.byref(x) for x in v]))
    return [x.value for x in v]


def _group_d(placement, flip):
    dig, pcs = crowd_d()
    crc = cases_c()
    for p in dig:
        want_digests(p)
    for p in pcs:
        want_sums(p)
    n_crc_threads = 4
    # (the timeout only breaks the barrier for the others when a thread failed before reaching it)
    bar = threading.Barrier(len(dig) + len(pcs) + n_crc_threads, timeout=120)

    def digester(p):
        once = []  # the barrier falls at the plan's first write, its digester made
        return run_digester(p, placement, before_write=lambda: once or (once.append(1), bar.wait()))

    def wait_then(f, *a):
        bar.wait()
        return f(*a)

    jobs = []
    for p in dig:
        if any(s[0] == "w" for s in p.steps):
            jobs.append(lambda p=p: digester(p))
        else:
            jobs.append(lambda p=p: wait_then(run_digester, p, placement))
    jobs += [lambda p=p: wait_then(run_piece, p, placement) for p in pcs]
    jobs += [lambda k=k: wait_then(lambda: [m for c in crc[k::n_crc_threads] for m in run_crc(c, placement)])
             for k in range(n_crc_threads)]
    s0 = engine_stats() if placement == KRK_PLACE_GPU else None
    t0 = time.perf_counter()
    bad = _concurrently(jobs, live=len(jobs))
    el = time.perf_counter() - t0
    if s0 is not None:  # a condition on the test, not a rate: without coalescing D proved nothing
        s1 = engine_stats()
        sha_b, sha_j, crc_b, crc_r = (s1[i] - s0[i] for i in range(4))
        if not (sha_b > 0 and sha_j > sha_b):
            bad.append(("D: SHA jobs per SHA launch must exceed 1", [sha_j, sha_b], "jobs > launches"))
        if not (crc_b > 0 and crc_r > crc_b):
            bad.append(("D: CRC requests per CRC batch must exceed 1", [crc_r, crc_b], "requests > batches"))
    return len(jobs), _bytes(dig) + _bytes(pcs) + sum(c.n for c in crc), el, bad


_RUN = {"A": _group_a, "B": _group_b, "C": _group_c, "D": _group_d}


def run_group_counted(name, placement, flip=False):
    """(cases, bytes moved, seconds of the run, mismatches) of group `name` on `placement`.  flip:
    one EXPECTED value of A, B or C is corrupted (the reporting's own test)."""
    return _RUN[name](placement, flip)


def run_group(name, placement):
    return run_group_counted(name, placement)[3]


def plans_e():
    return plans_a2() + plans_a3() + plans_a4()


def run_pend():
    """Group E, in a fresh process: the pool cap at its minimum BEFORE anything else touches the
    engine, then A2, A3 and A4 with E_LIVE owners live.  Returns the JSON record."""
    cap, waits = C.c_uint64(), C.c_uint64()
    check(lib.krk_engine_set_pool_cap(1, C.byref(cap), C.byref(waits)))
    plans = plans_e()
    for p in plans:
        want_digests(p)
    t0 = time.perf_counter()
    bad = _concurrently([lambda p=p: run_digester(p, KRK_PLACE_GPU) for p in plans], live=E_LIVE)
    el = time.perf_counter() - t0
    check(lib.krk_engine_set_pool_cap(0, C.byref(cap), C.byref(waits)))
    return {"group": "E", "cases": len(plans), "bytes": _bytes(plans), "seconds": round(el, 3), "cap": cap.value,
            "waits": waits.value, "pinned": engine_stats()[4], "n_mismatches": len(bad), "mismatches": bad[:10]}


def main(argv):
    host = "--host" in argv
    if not host:
        from kraken_amd import device as D
        assert D.device_count() > 0, "no gfx950 device"
        D.set_device(0)
    if "--pend" in argv:
        rec = run_pend()
        print(json.dumps(rec), flush=True)
        return 1 if rec["n_mismatches"] else 0
    failed = False
    for g in (HOST_GROUPS if host else GROUPS):
        n, nbytes, el, bad = run_group_counted(g, KRK_PLACE_HOST if host else KRK_PLACE_GPU)
        failed |= bool(bad)
        print(json.dumps({"group": g, "cases": n, "bytes": nbytes, "seconds": round(el, 3), "n_mismatches": len(bad),
                          "mismatches": bad[:10]}), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
