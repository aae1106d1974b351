"""GPU parity: the eight-lane SHA-256 consumer (sha256_w8_kernel, block8p) at the edges of its
block loop, bit-exact against hashlib, under both eight-lane launch plans (KRK_SHA_PLAN_8LANE,
KRK_SHA_PLAN_8LANE_2PAIR).  The loop runs whole producer steps (8 blocks, no guard, the chaining
snapshot selected by two constant half masks) while every live stream of the wave has the whole
step, and the rest in guarded four-block iterations whose snapshot masks are compared per block:

1. block counts 1, 2, 3, 4, 5, 7, 8, 9, 23, 24, 25, 32, 33 a stream, a whole wave of one count:
   tails of 1 .. 3 blocks, the 4- and 8-block iteration edges, the ring wrap at 3 slots x 8
   blocks; byte lengths on and one off the 55 / 56 / 64-byte padding edges;
2. those counts mixed in ONE wave, in both lane orders: streams freeze at different blocks while
   the wave runs on, the shortest stream ending inside a whole step, on its edge, or in the tail;
3. stream populations 1, 7, 8, 9, 17: a part-filled wave and a second workgroup;
4. a 25-block stream cut 9 + 16 through the chunked entry point: the first launch ends in a
   midstate after a whole step and a one-block tail, the second starts from it.

A snapshot under the wrong mask, a slot offset that wraps a step early or late, or a tail that
starts in the wrong slot shows as a wrong digest here."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from kraken_amd import device as D
from kraken_amd._capi import check, krk_chunk, lib

pytestmark = pytest.mark.gpu

PLANS = [5, 6]  # KRK_SHA_PLAN_8LANE (8 streams a workgroup), KRK_SHA_PLAN_8LANE_2PAIR (16)
COUNTS = [1, 2, 3, 4, 5, 7, 8, 9, 23, 24, 25, 32, 33]
# eight block counts a wave; the shortest stream has 1 (no whole step), 7, 13, 11 (ends inside
# the second step) and 16 blocks (ends on a step's edge)
MIXES = [
    [1, 2, 3, 4, 5, 7, 8, 9],
    [23, 24, 25, 32, 33, 9, 8, 7],
    [13, 33, 32, 25, 24, 23, 33, 32],
    [33, 33, 11, 33, 33, 33, 33, 33],
    [24, 25, 24, 25, 16, 32, 33, 17],
]
ARENA_BYTES = 1 << 20


@pytest.fixture(scope="module")
def arena(gpu):
    host = np.random.default_rng(20261021).integers(0, 256, size=ARENA_BYTES, dtype=np.uint8)
    buf = D.DeviceBuffer(ARENA_BYTES)
    buf.from_host(host)
    yield host.tobytes(), buf
    buf.free()


@pytest.fixture
def sha_plan():
    def set_plan(p):
        check(lib.krk_set_sha_plan(p))
    yield set_plan
    check(lib.krk_set_sha_plan(0))


_WANT = {}


def want(hb, off, n):
    v = _WANT.get((off, n))
    if v is None:
        v = _WANT[off, n] = hashlib.sha256(hb[off:off + n]).digest()
    return v


def blocks(n):
    """Blocks the kernel runs for a final stream of n bytes."""
    return n // 64 + (2 if n % 64 >= 56 else 1)


def lengths(m):
    """Final lengths of m blocks on and one off the padding edges: a tail of 0 (the 64-byte
    edge), 1, 54 and 55 bytes (the last with one padding block), and (m >= 2) of 56, 57 and 63
    bytes (two padding blocks, so one data block fewer)."""
    ls = [64 * (m - 1) + t for t in (0, 1, 54, 55)]
    if m >= 2:
        ls += [64 * (m - 2) + t for t in (56, 57, 63)]
    assert all(blocks(n) == m for n in ls)
    return ls


def place(lens):
    """Arena offsets of the streams, back to back from varying ptr % 16."""
    offs, cur = [], 0
    for i, n in enumerate(lens):
        o = (cur + 15) // 16 * 16 + (5 * i) % 16
        offs.append(o)
        cur = o + n
    assert cur + 64 <= ARENA_BYTES
    return offs


def one_shot(arena, lens):
    """krk_sha256_dev over the streams; the list of streams whose digest is wrong."""
    hb, buf = arena
    offs, n = place(lens), len(lens)
    ptrs = np.array([buf.ptr + o for o in offs], dtype=np.uint64)
    ln = np.array(lens, dtype=np.uint64)
    out = D.DeviceBuffer(32 * n)
    check(lib.krk_sha256_dev(ptrs.ctypes.data_as(C.POINTER(C.c_void_p)), ln.ctypes.data_as(C.POINTER(C.c_uint64)),
                             n, out.ptr, None))
    D.synchronize()
    got = out.to_host(np.uint8, 32 * n).reshape(-1, 32)
    out.free()
    return [(i, lens[i], blocks(lens[i])) for i in range(n) if bytes(got[i]) != want(hb, offs[i], lens[i])]


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("m", COUNTS)
def test_uniform_wave_block_counts(arena, sha_plan, plan, m):
    """Eight streams of m blocks each, one launch per length form: m // 8 whole steps, then a
    tail of m % 8 blocks in one or two guarded iterations."""
    sha_plan(plan)
    for n in lengths(m):
        bad = one_shot(arena, [n] * 8)
        assert not bad, f"plan {plan}, {m} blocks, length {n}: wrong (stream, length, blocks) {bad}"


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("mix", range(len(MIXES)))
def test_ragged_wave(arena, sha_plan, plan, reverse, mix):
    """Eight block counts side by side in one wave, for every length form: whole steps stop at
    the shortest stream, and past it each stream's chaining value freezes at its own block."""
    sha_plan(plan)
    order = MIXES[mix][::-1] if reverse else MIXES[mix]
    for form in range(7):
        lens = [lengths(m)[form % len(lengths(m))] for m in order]
        bad = one_shot(arena, lens)
        assert not bad, f"plan {plan}, mix {order}, form {form}: wrong (stream, length, blocks) {bad}"


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("n_streams", [1, 7, 8, 9, 17])
def test_stream_populations(arena, sha_plan, plan, n_streams):
    """Part-filled waves and workgroups: the dead lanes do not hold the whole steps back and run
    the same rounds on nothing."""
    sha_plan(plan)
    counts = [COUNTS[(5 * i + 8) % len(COUNTS)] for i in range(n_streams)]
    lens = [lengths(m)[i % len(lengths(m))] for i, m in enumerate(counts)]
    bad = one_shot(arena, lens)
    assert not bad, f"plan {plan}, {n_streams} streams: wrong (stream, length, blocks) {bad}"


@pytest.mark.parametrize("plan", PLANS)
def test_midstate_cut_9_16(arena, sha_plan, plan):
    """A blob of 25 blocks cut after 9: chunk one (one whole step and a one-block tail) ends in
    a midstate, chunk two (kShaFromState: two whole steps) starts from it; eight such blobs fill
    the wave and the digest is the one-shot digest."""
    sha_plan(plan)
    hb, buf = arena
    total = 64 * 24 + 41
    assert blocks(total) == 25
    offs = place([total] * 8)
    cuts = [64 * 9] * 8
    st, sums, dg = D.DeviceBuffer(32 * 8), D.DeviceBuffer(4 * 8), D.DeviceBuffer(32 * 8)
    st.zero()
    sums.zero()
    for first in (True, False):
        arr = D.chunk_array([buf.ptr + o + (0 if first else c) for o, c in zip(offs, cuts)],
                            [0 if first else c for c in cuts],
                            [c if first else total - c for c in cuts], [total] * 8, 4 << 20, np.arange(8),
                            list(range(8)))
        check(lib.krk_metainfo_digest_chunks_dev(arr.ctypes.data_as(C.POINTER(krk_chunk)), 8, st.ptr, sums.ptr,
                                                 dg.ptr, None))
    D.synchronize()
    got = dg.to_host(np.uint8, 32 * 8).reshape(-1, 32)
    bad = [i for i in range(8) if bytes(got[i]) != want(hb, offs[i], total)]
    for b in (st, sums, dg):
        b.free()
    assert not bad, f"plan {plan}: wrong streams {bad}"
