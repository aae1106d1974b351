"""GPU parity: the SHA-256 kernels (sha256_multi.hip) at their structural edges, bit-exact
against hashlib and the plain-Python reference (tests/sha256_ref.py), under every production
launch plan:

1. every data alignment (ptr % 16) x every tail residue (len % 64), one-shot;
2. the same grid as final chunks continued from an injected midstate;
3. every pair (own block count, workgroup block count) inside ONE workgroup, final and
   non-final streams, zero-length chunks of both kinds;
4. launch populations around the streams a workgroup takes, and the AUTO tier boundaries;
5. digest pointers of no alignment, midstate rows, and the bytes next to both left untouched;
6. chunk offsets of 2^29 .. 2^40 bytes (the 64-bit padding length), with the piece CRCs.

All data comes from one seeded random array uploaded once; streams are laid out back to back
(a stream's 16-byte chunks hold its neighbours' bytes), with at least 64 spare bytes after the
last one.  Nothing here depends on what lies past an allocation."""
import ctypes as C
import hashlib
import zlib
from collections import namedtuple

import numpy as np
import pytest

from kraken_amd import device as D
from kraken_amd._capi import check, krk_chunk, lib
from tests import sha256_ref as R

pytestmark = pytest.mark.gpu

PLANS = [1, 2, 3, 4, 5, 6]
PER = {1: 64, 2: 32, 3: 128, 4: 64, 5: 8, 6: 16}  # streams a workgroup takes (KRK_SHA_PLAN_*)
ARENA_BYTES = 4 << 20
CANARY = 0xC3
P4M = 4 << 20

Arena = namedtuple("Arena", "host hb buf")
# One stream: n bytes at arena offset `off`, `prefix` bytes absorbed before them (the chunk's
# offset; > 0: `state` is injected as the midstate), final or a run of whole blocks; its digest
# or midstate goes to blob slot `slot`.
Stream = namedtuple("Stream", "off n prefix final state slot")


@pytest.fixture(scope="module")
def arena(gpu):
    host = np.random.default_rng(20251019).integers(0, 256, size=ARENA_BYTES, dtype=np.uint8)
    buf = D.DeviceBuffer(ARENA_BYTES)
    assert buf.ptr % 16 == 0
    buf.from_host(host)
    yield Arena(host, host.tobytes(), buf)
    buf.free()


@pytest.fixture
def sha_plan():
    """Sets a process-wide SHA-256 launch plan (krk_set_sha_plan), restores AUTO after."""
    def set_plan(p):
        check(lib.krk_set_sha_plan(p))
    yield set_plan
    check(lib.krk_set_sha_plan(0))


class Layout:
    """Arena offsets with a chosen ptr % 16, back to back; 64 bytes stay spare at the end."""

    def __init__(self):
        self.cur = 0

    def take(self, n, align=0):
        o = (self.cur + 15) // 16 * 16 + align
        assert o + n + 64 <= ARENA_BYTES, "the arena is too small for this layout"
        self.cur = o + n
        return o


def rand_state(rng):
    return tuple(int(x) for x in rng.integers(0, 1 << 32, size=8, dtype=np.uint64))


_MID, _WANT = {}, {}


def want(a, s):
    """The digest (final) or the 8-word midstate (non-final) of stream s, computed once a
    session: the plans share their streams.  The midstate after the whole blocks does not
    depend on the absorbed count, so it is shared by streams that differ only there."""
    key = s[:5]
    v = _WANT.get(key)
    if v is not None:
        return v
    d = a.hb[s.off:s.off + s.n]
    if s.final and s.prefix == 0:
        v = hashlib.sha256(d).digest()
    else:
        h = s.state if s.prefix else R.IV
        full = s.n // 64 * 64
        mk = (h, s.off, full)
        mid = _MID.get(mk)
        if mid is None:
            mid = _MID[mk] = R.resume(h, 0, d[:full], False)
        v = R.resume(mid, s.prefix + full, d[full:], True) if s.final else mid
    _WANT[key] = v
    return v


def chunks_call(a, streams, state_ptr, sums_ptr, digests_ptr, piece_length=P4M, sums_offsets=None):
    """One krk_metainfo_digest_chunks_dev call over `streams` (a non-final stream's blob goes on
    for another block).  Each chunk's piece sum lands in its own word of the sums buffer."""
    n = len(streams)
    arr = D.chunk_array([a.buf.ptr + s.off for s in streams], [s.prefix for s in streams],
                        [s.n for s in streams], [s.prefix + s.n + (0 if s.final else 64) for s in streams],
                        piece_length, np.arange(n) if sums_offsets is None else sums_offsets,
                        [s.slot for s in streams])
    check(lib.krk_metainfo_digest_chunks_dev(arr.ctypes.data_as(C.POINTER(krk_chunk)), n, state_ptr, sums_ptr,
                                             digests_ptr, None))


def state_image(n_slots, streams, fill=CANARY):
    """The state_dev image before a call: `fill` bytes, the injected midstates in their rows."""
    img = np.full(n_slots * 8, fill * 0x01010101, dtype=np.uint32)
    for s in streams:
        if s.prefix:
            img[8 * s.slot:8 * s.slot + 8] = s.state
    return img


# ------------------------------------------------------------------ 1, 2: alignment x tail
GRID = [(al, 64 * k + r) for k in range(3) for al in range(16) for r in range(64)]


@pytest.fixture(scope="module")
def grid(arena):
    lay = Layout()
    return [lay.take(n, al) for al, n in GRID]


@pytest.mark.parametrize("plan", PLANS)
def test_alignment_x_tail_one_shot(arena, grid, sha_plan, plan):
    """krk_sha256_dev over every ptr % 16 in 0..15 x every len % 64 in 0..63 behind 0, 1 and 2
    whole blocks (3,072 streams, one launch): both value muxes of the schedule builder, the
    keep < 4 masks, the 0x80 byte at every position, one and two padding blocks."""
    sha_plan(plan)
    n = len(GRID)
    ptrs = np.array([arena.buf.ptr + o for o in grid], dtype=np.uint64)
    lens = np.array([ln for _, ln in GRID], dtype=np.uint64)
    out = D.DeviceBuffer(32 * n)
    check(lib.krk_sha256_dev(ptrs.ctypes.data_as(C.POINTER(C.c_void_p)), lens.ctypes.data_as(C.POINTER(C.c_uint64)),
                             n, out.ptr, None))
    D.synchronize()
    got = out.to_host(np.uint8, 32 * n).reshape(-1, 32)
    bad = [(plan, al, ln) for (al, ln), o, g in zip(GRID, grid, got)
           if bytes(g) != want(arena, Stream(o, ln, 0, True, None, 0))]
    assert not bad, f"{len(bad)} of {n} digests wrong, first (plan, ptr % 16, length): {bad[:8]}"


@pytest.mark.parametrize("plan", PLANS)
def test_alignment_x_tail_from_midstate(arena, grid, sha_plan, plan):
    """The same grid as final chunks at offset 64, each from its own random midstate in
    state_dev: the kShaFromState load of every kernel body at every alignment and tail
    (length 0 included: one pure padding block from a midstate)."""
    sha_plan(plan)
    rng = np.random.default_rng(7)
    streams = [Stream(o, ln, 64, True, rand_state(rng), i) for i, ((_, ln), o) in enumerate(zip(GRID, grid))]
    n = len(streams)
    st, sums, dg = D.DeviceBuffer(32 * n), D.DeviceBuffer(4 * n), D.DeviceBuffer(32 * n)
    st.from_host(state_image(n, streams))
    sums.zero()
    chunks_call(arena, streams, st.ptr, sums.ptr, dg.ptr)
    D.synchronize()
    got = dg.to_host(np.uint8, 32 * n).reshape(-1, 32)
    bad = [(plan, al, ln) for (al, ln), s, g in zip(GRID, streams, got) if bytes(g) != want(arena, s)]
    assert not bad, f"{len(bad)} of {n} digests wrong, first (plan, ptr % 16, length): {bad[:8]}"


# ------------------------------------------------------------------ 3: one workgroup
BLOCKS = [1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 23, 24, 25, 26, 31, 32, 33, 47, 48, 49, 50, 73]


def build_forms():
    """For every kernel block count m in 0..73 the streams that have it (slot filled in later):
    'run': a non-final run of m whole blocks (even m: from a midstate at offset 64, m = 0 the
    zero-length chunk whose row must come back unchanged; odd m: from the IV); 'pad1': a
    final stream of m - 1 whole blocks and a tail below 56 bytes (one padding block; every
    third from a midstate); 'pad2': m - 2 whole blocks and a tail of 56..63 bytes (two padding
    blocks; odd m from a midstate).  One data region and one midstate per (form, m), so the
    launches of different workgroup block counts share their expected values."""
    lay, rng = Layout(), np.random.default_rng(33)
    f = {}
    for m in range(0, max(BLOCKS) + 1):
        pre = 0 if m % 2 else 64
        f["run", m] = Stream(lay.take(64 * m, m % 16), 64 * m, pre, False, rand_state(rng) if pre else None, 0)
        if m >= 1:
            n, pre = 64 * (m - 1) + (7 * m + 3) % 56, 192 if m % 3 == 0 else 0
            f["pad1", m] = Stream(lay.take(n, (5 * m + 1) % 16), n, pre, True, rand_state(rng) if pre else None, 0)
        if m >= 2:
            n, pre = 64 * (m - 2) + 56 + m % 8, 128 if m % 2 else 0
            f["pad2", m] = Stream(lay.take(n, (3 * m + 2) % 16), n, pre, True, rand_state(rng) if pre else None, 0)
    # offset == blob_length, a multiple of 64: one pure padding block from a midstate
    f["empty_final"] = Stream(lay.take(0, 9), 0, 1 << 12, True, rand_state(rng), 0)
    return f


@pytest.fixture(scope="module")
def forms():
    return build_forms()


def one_workgroup_launches(forms, per):
    """[(workgroup block count N, streams of one launch)]: every launch holds at most `per`
    streams (one workgroup) -- one of N blocks, the others of every m in 0..N-1 in each form."""
    launches, slot = [], 0
    for N in BLOCKS:
        long_ = forms[("run", "pad1", "pad2")[N % 3], N]
        others = [forms["empty_final"]]
        for m in range(N):
            others += [forms[k, m] for k in ("run", "pad1", "pad2") if (k, m) in forms]
        for at in range(0, len(others), per - 1):
            batch = []
            for s in [long_] + others[at:at + per - 1]:
                batch.append(s._replace(slot=slot))
                slot += 1
            launches.append((N, batch))
    return launches, slot


@pytest.mark.parametrize("plan", PLANS)
def test_block_counts_inside_one_workgroup(arena, forms, sha_plan, plan):
    """Every (own block count m, workgroup block count N) for N in BLOCKS, m in 0..N-1: the
    ring slots (periods 4, 3 and 3), the producer's register rotation (3 steps), the eight-lane
    step of 8 blocks and its unroll of 4, and the per-lane freeze of finished streams while the
    workgroup runs on to N.  Final digests and non-final state rows, word for word."""
    sha_plan(plan)
    launches, n_slots = one_workgroup_launches(forms, PER[plan])
    streams = [s for _, b in launches for s in b]
    st, dg = D.DeviceBuffer(32 * n_slots), D.DeviceBuffer(32 * n_slots)
    sums = D.DeviceBuffer(4 * PER[plan])
    st.from_host(state_image(n_slots, streams))
    dg.from_host(np.full(32 * n_slots, CANARY, dtype=np.uint8))
    sums.zero()
    for N, batch in launches:
        assert len(batch) <= PER[plan]
        chunks_call(arena, batch, st.ptr, sums.ptr, dg.ptr)
    D.synchronize()
    digests = dg.to_host(np.uint8, 32 * n_slots).reshape(-1, 32)
    state = st.to_host(np.uint32, 8 * n_slots).reshape(-1, 8)
    bad = []
    for N, batch in launches:
        for s in batch:
            got = bytes(digests[s.slot]) if s.final else tuple(int(x) for x in state[s.slot])
            if got != want(arena, s):
                own = s.n // 64 + ((2 if s.n % 64 >= 56 else 1) if s.final else 0)
                bad.append(dict(plan=plan, workgroup_blocks=N, own_blocks=own, final=s.final, length=s.n,
                                prefix=s.prefix, align=s.off % 16))
    assert not bad, f"{len(bad)} of {len(streams)} streams wrong, first {bad[:6]}"


# ------------------------------------------------------------------ 4: populations
def population(arena, count, max_len):
    """`count` streams of distinct data, lengths 0..max_len - 1, every alignment."""
    lay = Layout()
    lens = [(37 * i + 11) % max_len for i in range(count)]
    offs = [lay.take(n, i % 16) for i, n in enumerate(lens)]
    return offs, lens


def run_population(arena, offs, lens, n):
    ptrs = np.array([arena.buf.ptr + o for o in offs[:n]], dtype=np.uint64)
    ln = np.array(lens[:n], dtype=np.uint64)
    out = D.DeviceBuffer(32 * n)
    check(lib.krk_sha256_dev(ptrs.ctypes.data_as(C.POINTER(C.c_void_p)), ln.ctypes.data_as(C.POINTER(C.c_uint64)), n,
                             out.ptr, None))
    D.synchronize()
    return out.to_host(np.uint8, 32 * n).reshape(-1, 32)


@pytest.mark.parametrize("plan", PLANS)
def test_populations_around_a_workgroup(arena, sha_plan, plan):
    """n streams of 1 to 3 blocks for n around the streams a workgroup takes: a lone stream, a
    second pair that is dead, holds one stream or lacks one, a full workgroup, and a second
    and third workgroup of one stream."""
    sha_plan(plan)
    per = PER[plan]
    offs, lens = population(arena, 2 * per + 1, 183)  # 183 = 3 * 64 - 9: at most three blocks
    for n in sorted({1, per // 2, per // 2 + 1, per - 1, per, per + 1, 2 * per + 1}):
        got = run_population(arena, offs, lens, n)
        bad = [(i, lens[i]) for i in range(n)
               if bytes(got[i]) != want(arena, Stream(offs[i], lens[i], 0, True, None, 0))]
        assert not bad, f"plan {plan}, {n} streams: {len(bad)} digests wrong, first (stream, length): {bad[:8]}"


def test_auto_tier_boundaries(arena):
    """AUTO at and one past 16, 32 and 64 streams a CU: the plan each side of a boundary
    launches, and every digest of one-block streams."""
    cus = D.device_cus()
    ns = [16 * cus, 16 * cus + 1, 32 * cus, 32 * cus + 1, 64 * cus, 64 * cus + 1]
    assert [D.sha_plan_for(n) for n in ns] == [5, 2, 2, 4, 4, 3]
    offs, lens = population(arena, ns[-1], 56)  # below 56 bytes: one block
    ref = [want(arena, Stream(o, n, 0, True, None, 0)) for o, n in zip(offs, lens)]
    for n in ns:
        got = run_population(arena, offs, lens, n)
        bad = [(i, lens[i]) for i in range(n) if bytes(got[i]) != ref[i]]
        assert not bad, f"{n} streams (plan {D.sha_plan_for(n)}): {len(bad)} digests wrong, first {bad[:8]}"


# ------------------------------------------------------------------ 5: outputs
SLOTS = 70001


def first_diff(got, exp):
    d = np.nonzero(got != exp)[0]
    return None if d.size == 0 else (int(d[0]), int(d.size))


@pytest.mark.parametrize("plan", PLANS)
def test_unaligned_outputs_and_untouched_neighbours(arena, sha_plan, plan):
    """digests_dev = buffer + d for d in 1, 4, 8, 12, 16 (kraken_hip.h promises no alignment:
    the byte-store branch of each kernel body), final and non-final chunks in sparse blob
    slots: every digest and state row is right -- the row layout is 8 words a slot, H order --
    and every other byte of both buffers still holds what it held before the call."""
    sha_plan(plan)
    lay, rng = Layout(), np.random.default_rng(5)

    def mk(n, pre, fin, slot):
        return Stream(lay.take(n, (7 * slot + 1) % 16), n, pre, fin, rand_state(rng) if pre else None, slot)

    streams = [mk(100, 0, True, 0), mk(128, 0, False, 5), mk(61, 128, True, 6), mk(192, 64, False, 1000),
               mk(0, 64, False, 1001), mk(0, 0, True, 69999), mk(200, 1 << 20, True, 70000)]
    st, dg, sums = D.DeviceBuffer(32 * SLOTS), D.DeviceBuffer(32 * SLOTS + 64), D.DeviceBuffer(4 * len(streams))
    sums.zero()
    before = state_image(SLOTS, streams)
    exp_state = before.copy()
    for s in streams:
        if not s.final:
            exp_state[8 * s.slot:8 * s.slot + 8] = want(arena, s)
    # the one-shot call: streams 0 .. 19 of a population, digest i at buffer + d + 32 i
    offs, lens = population(arena, 20, 183)
    ptrs = np.array([arena.buf.ptr + o for o in offs], dtype=np.uint64)
    ln = np.array(lens, dtype=np.uint64)
    for d in (1, 4, 8, 12, 16):
        st.from_host(before)
        dg.from_host(np.full(dg.nbytes, CANARY, dtype=np.uint8))
        chunks_call(arena, streams, st.ptr, sums.ptr, dg.ptr + d)
        D.synchronize()
        exp = np.full(dg.nbytes, CANARY, dtype=np.uint8)
        for s in streams:
            if s.final:
                exp[d + 32 * s.slot:d + 32 * s.slot + 32] = np.frombuffer(want(arena, s), dtype=np.uint8)
        diff = first_diff(dg.to_host(np.uint8), exp)
        assert diff is None, f"plan {plan}, digests at +{d}: first wrong byte {diff[0]} (slot {(diff[0] - d) // 32}), {diff[1]} wrong"
        diff = first_diff(st.to_host(np.uint32), exp_state)
        assert diff is None, f"plan {plan}, digests at +{d}: first wrong state word {diff[0]} (slot {diff[0] // 8}), {diff[1]} wrong"

        dg.from_host(np.full(dg.nbytes, CANARY, dtype=np.uint8))
        check(lib.krk_sha256_dev(ptrs.ctypes.data_as(C.POINTER(C.c_void_p)), ln.ctypes.data_as(C.POINTER(C.c_uint64)),
                                 len(offs), dg.ptr + d, None))
        D.synchronize()
        exp = np.full(dg.nbytes, CANARY, dtype=np.uint8)
        for i, (o, n) in enumerate(zip(offs, lens)):
            exp[d + 32 * i:d + 32 * i + 32] = np.frombuffer(want(arena, Stream(o, n, 0, True, None, 0)), dtype=np.uint8)
        diff = first_diff(dg.to_host(np.uint8), exp)
        assert diff is None, f"plan {plan}, krk_sha256_dev digests at +{d}: first wrong byte {diff[0]}, {diff[1]} wrong"


# ------------------------------------------------------------------ 6: 64-bit offsets
OFFSETS = [(1 << 29) - 64, 1 << 29, (1 << 32) - 64, 1 << 32, (1 << 32) + (1 << 29), 1 << 40]
TAILS = [0, 1, 55, 56, 64, 4096 + 3, 200_000]


@pytest.fixture(scope="module")
def tails(arena):
    """One data region and one midstate per length, shared by the offsets: the expected digests
    then differ only in the padded bit length, and the 3,125 blocks of the longest run go
    through the Python reference once."""
    lay, rng = Layout(), np.random.default_rng(64)
    return {n: (lay.take(n, (3 * i + 1) % 16), rand_state(rng)) for i, n in enumerate(TAILS)}


def piece_sums_expected(data, offset, P):
    """{piece index: sum} of a chunk `data` at blob offset `offset` that ends its blob.  A piece
    that starts inside the chunk: zlib.crc32 of its slice.  A piece the chunk enters mid-way
    gets the chunk's XOR share only: CRC-32 is affine in the message, crc32(M) = L(M) ^
    crc32(0^|M|) with L linear and blind to leading zeros, so the share of the piece's last
    bytes B is L(B) = crc32(B) ^ crc32(0^|B|)."""
    end, out = offset + len(data), {}
    if not data:
        return out
    for pi in range(offset // P, (end - 1) // P + 1):
        ps, pe = pi * P, min((pi + 1) * P, end)
        if ps >= offset:
            out[pi] = zlib.crc32(data[ps - offset:pe - offset])
        else:
            b = data[:pe - offset]
            out[pi] = zlib.crc32(b) ^ zlib.crc32(bytes(len(b)))
    return out


@pytest.mark.parametrize("offset", OFFSETS)
def test_64bit_offsets_sha_and_crc(arena, tails, offset):
    """Final chunks at offsets of 2^29 .. 2^40 bytes from an injected midstate, one call each
    (AUTO plan): the 64-bit bit length of the padding (its high word is nonzero from 2^29 bytes
    on, and above 2^32 - 1 in bytes from 2^32), and the piece CRCs at piece index offset / P
    (4 MiB pieces; 1 MiB at 2^40: 2^20 sums).  Sums before the chunk's first piece stay zero."""
    cases = [(n, P4M) for n in TAILS] + ([(4096 + 3, 1 << 20)] if offset == 1 << 40 else [])
    st, dg = D.DeviceBuffer(32), D.DeviceBuffer(32)
    for n, P in cases:
        off, state = tails[n]
        s = Stream(off, n, offset, True, state, 0)
        count = int(lib.krk_num_pieces(offset + n, P))
        sums = D.DeviceBuffer(4 * count)
        sums.zero()
        st.from_host(state_image(1, [s]))
        dg.zero()
        chunks_call(arena, [s], st.ptr, sums.ptr, dg.ptr, piece_length=P, sums_offsets=[0])
        D.synchronize()
        assert bytes(dg.to_host(np.uint8, 32)) == want(arena, s), (offset, n, P)
        got = sums.to_host(np.uint32, count)
        exp = np.zeros(count, dtype=np.uint32)
        for pi, v in piece_sums_expected(arena.hb[off:off + n], offset, P).items():
            exp[pi] = v
        assert not got[:offset // P].any(), (offset, n, P)
        assert np.array_equal(got, exp), (offset, n, P, np.nonzero(got != exp)[0][:4])
        sums.free()


def test_64bit_offset_chunk_split_inside_a_piece(arena):
    """A piece at 2^32 bytes hashed in two calls, [kP, kP + 64 m) then the rest: the second
    chunk starts mid-piece and continues from the state row the first one wrote; the piece's
    XOR-accumulated sum is zlib.crc32 of the whole slice."""
    base, m, n = 1 << 32, 3, 5000 + 7
    lay = Layout()
    off, state = lay.take(n, 13), rand_state(np.random.default_rng(9))
    count = int(lib.krk_num_pieces(base + n, P4M))
    st, dg, sums = D.DeviceBuffer(32), D.DeviceBuffer(32), D.DeviceBuffer(4 * count)
    sums.zero()
    first = Stream(off, 64 * m, base, False, state, 0)
    st.from_host(state_image(1, [first]))
    arr = D.chunk_array([arena.buf.ptr + off], [base], [64 * m], [base + n], P4M, [0], [0])
    check(lib.krk_metainfo_digest_chunks_dev(arr.ctypes.data_as(C.POINTER(krk_chunk)), 1, st.ptr, sums.ptr, dg.ptr, None))
    D.synchronize()
    assert tuple(int(x) for x in st.to_host(np.uint32, 8)) == want(arena, first)
    arr = D.chunk_array([arena.buf.ptr + off + 64 * m], [base + 64 * m], [n - 64 * m], [base + n], P4M, [0], [0])
    check(lib.krk_metainfo_digest_chunks_dev(arr.ctypes.data_as(C.POINTER(krk_chunk)), 1, st.ptr, sums.ptr, dg.ptr, None))
    D.synchronize()
    assert bytes(dg.to_host(np.uint8, 32)) == R.resume(state, base, arena.hb[off:off + n], True)
    got = sums.to_host(np.uint32, count)
    assert not got[:base // P4M].any()
    assert int(got[base // P4M]) == zlib.crc32(arena.hb[off:off + n])
