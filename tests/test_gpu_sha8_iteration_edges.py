"""GPU parity: the eight-lane SHA-256 consumer (sha256_w8_kernel, block8p) at the edges of its
four-block loop iteration and of its W delivery, bit-exact against hashlib, under both
eight-lane launch plans (KRK_SHA_PLAN_8LANE, KRK_SHA_PLAN_8LANE_2PAIR):

1. block counts a stream around the unroll (1 .. 13), a whole wave of one count, at lengths
   just under, on and just over a block boundary (one and two padding blocks);
2. block counts {1, 2, 3, 4, 5, 8, 9, 13} in ONE wave, in both lane orders: streams freeze at
   different iterations while their neighbours go on;
3. stream populations 1, 7, 8, 9, 17: a part-filled wave, exactly one, a second workgroup, a
   third with one stream;
4. a blob cut at a block count that is no multiple of the unroll: the first chunk ends in a
   midstate, the second starts from it, the digest is the one-shot digest;
5. 3 x 8 + 1 producer steps: the ring wraps, and the W read-ahead of the next block crosses
   every slot boundary.

The consumer reads the next block's first W quads while it runs the current block, and holds W
in registers it loads itself; a wrong wait, a read landing in a register still in use, or a
chaining value snapshot taken in the wrong iteration shows as a wrong digest here."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from kraken_amd import device as D
from kraken_amd._capi import check, krk_chunk, lib

pytestmark = pytest.mark.gpu

PLANS = [5, 6]  # KRK_SHA_PLAN_8LANE (8 streams a workgroup), KRK_SHA_PLAN_8LANE_2PAIR (16)
COUNTS = [1, 2, 3, 4, 5, 7, 8, 9, 12, 13]
MIXED = [1, 2, 3, 4, 5, 8, 9, 13]
ARENA_BYTES = 1 << 20


@pytest.fixture(scope="module")
def arena(gpu):
    host = np.random.default_rng(20261020).integers(0, 256, size=ARENA_BYTES, dtype=np.uint8)
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
    """Final lengths of m blocks: on the boundary, just over, the longest one-padding-block
    tail, and (m >= 2) just under the boundary and the shortest two-padding-block tail."""
    ls = [64 * (m - 1), 64 * (m - 1) + 1, 64 * (m - 1) + 55]
    if m >= 2:
        ls += [64 * (m - 1) - 1, 64 * (m - 1) - 8]
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
    """Eight streams of m blocks each, one launch per length form: every stream of the wave
    ends in the same iteration, at every position of the four-block body."""
    sha_plan(plan)
    for n in lengths(m):
        bad = one_shot(arena, [n] * 8)
        assert not bad, f"plan {plan}, {m} blocks, length {n}: wrong (stream, length, blocks) {bad}"


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("reverse", [False, True])
def test_mixed_block_counts_in_one_wave(arena, sha_plan, plan, reverse):
    """Block counts {1, 2, 3, 4, 5, 8, 9, 13} side by side in one wave, for every length form:
    a stream's chaining value freezes in its own iteration and the others run on."""
    sha_plan(plan)
    order = MIXED[::-1] if reverse else MIXED
    for form in range(5):
        lens = [lengths(m)[form % len(lengths(m))] for m in order]
        bad = one_shot(arena, lens)
        assert not bad, f"plan {plan}, form {form}: wrong (stream, length, blocks) {bad}"


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("n_streams", [1, 7, 8, 9, 17])
def test_stream_populations(arena, sha_plan, plan, n_streams):
    """Part-filled waves and workgroups: the dead lanes run the same rounds on nothing."""
    sha_plan(plan)
    lens = [lengths(COUNTS[(3 * i) % len(COUNTS)])[i % 3] for i in range(n_streams)]
    bad = one_shot(arena, lens)
    assert not bad, f"plan {plan}, {n_streams} streams: wrong (stream, length, blocks) {bad}"


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("cut", [1, 3, 5, 6, 9])
def test_midstate_cut_off_the_unroll(arena, sha_plan, plan, cut):
    """A blob of 13 blocks cut after `cut` blocks: chunk one ends in a midstate, chunk two
    starts from it; eight such blobs fill the wave.  The even streams are cut at `cut`, never
    a multiple of the unroll; the odd streams one block later (a multiple of it for cut = 3),
    so streams freezing in the same and in neighbouring blocks share the wave."""
    sha_plan(plan)
    hb, buf = arena
    total = 64 * 12 + 41
    offs = place([total] * 8)
    cuts = [64 * (cut + i % 2) for i in range(8)]
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
    bad = [(i, cuts[i] // 64) for i in range(8) if bytes(got[i]) != want(hb, offs[i], total)]
    for b in (st, sums, dg):
        b.free()
    assert not bad, f"plan {plan}: wrong (stream, blocks before the cut) {bad}"


@pytest.mark.parametrize("plan", PLANS)
def test_ring_wrap(arena, sha_plan, plan):
    """Streams of 3 x 8 + 1 producer steps (193 and 200 blocks) beside short ones: the
    three-slot ring wraps eight times and every slot boundary is crossed by the read-ahead."""
    sha_plan(plan)
    lens = [64 * 192 + 3, 64 * 199 + 20, 64 * 191 + 60, 100, 64 * 24 + 1, 64 * 23 + 57, 64 * 16, 0]
    assert [blocks(n) for n in lens[:3]] == [193, 200, 193]
    bad = one_shot(arena, lens)
    assert not bad, f"plan {plan}: wrong (stream, length, blocks) {bad}"
