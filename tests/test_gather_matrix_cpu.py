"""The gather matrix harness (tests/gather_matrix.py) checked where no GPU is: its case lists
reach what the module says they reach, no two destination rooms overlap, the expected-image
builder agrees with a plain numpy restatement of the kernel's word arithmetic, and the
comparison reports a wrong byte and a stray write -- all right before a kernel is involved."""
import ctypes as C

import numpy as np
import pytest

from kraken_amd import _capi
from kraken_amd._capi import lib
from tests import gather_matrix as M


@pytest.fixture(scope="module")
def arena():
    a = M.make_arena_bytes()
    a.setflags(write=False)
    return a


def _inside(spans):
    return all(s.src is None and s.n == 0 or 0 <= s.src and s.src + s.n <= M.ARENA_BYTES and s.n > 0 for s in spans)


def test_group_a_cases():
    assert [len(M.tails(r)) for r in range(16)] == [4, 4, 5, 6, 6, 6, 6, 6, 5, 5, 6, 6, 6, 6, 6, 5]
    for r in range(1, 16):  # the two lengths either side of in_words growing by one
        assert 16 - r in M.tails(r) and min(16, 17 - r) in M.tails(r)
    spans, size, calls = M.cases("A")
    assert len(spans) == 88 * 21 == 1848 and calls == [list(range(1848))] and _inside(spans)
    assert sum(s.n for s in spans) == 24_326_592 and M.n_tiles(spans) == 1848 + 88 == 1936  # 23.2 MiB
    assert M.n_tiles(spans) > 256  # more tiles than a grid of max(64, CUs) workgroups: the tile stride runs
    assert {M.out_words(s) for s in spans} == set(M.OUT_WORDS)
    for s in spans:
        assert s.n == 16 * (M.out_words(s) - 1) + ((s.n - 1) % 16 + 1)
    # every (source residue, in_words - out_words, out_words a multiple of 64) that can occur:
    # an aligned source never needs the extra word
    triples = {(s.src % 16, M.in_words(s) - M.out_words(s), M.out_words(s) % 64 == 0) for s in spans}
    assert triples == {(r, d, m) for r in range(16) for d in ((0, 1) if r else (0,)) for m in (False, True)}
    assert len(triples) == 62
    # ... at every out_words of the list, both sides of the extra word for every r > 0
    for w in M.OUT_WORDS:
        mine = {(s.src % 16, M.in_words(s) - M.out_words(s)) for s in spans if M.out_words(s) == w}
        assert mine == {(r, d) for r in range(16) for d in ((0, 1) if r else (0,))}, w
    # every funnel shape: the dword shift r >> 2 and the byte shift r & 3 (0: no v_alignbyte)
    assert {((s.src % 16) >> 2, (s.src % 16) & 3) for s in spans} == {(q, b) for q in range(4) for b in range(4)}


def test_group_b_and_c_cases():
    spans, size, calls = M.cases("B")
    assert len(spans) == 2 * sum(len(M.tails(r)) for r in M.B_RESIDUES) == 60 and len(calls) == 1 and _inside(spans)
    assert {s.src % 16 for s in spans} == set(M.B_RESIDUES)
    assert {(s.n + M.K_TILE - 1) // M.K_TILE for s in spans} == {3, 4}
    for s in spans:  # every tile but the last is whole, so each tile's source keeps the residue
        assert s.n // M.K_TILE in M.B_TILES and 1 <= s.n % M.K_TILE <= 16
    assert M.disjoint(spans, size)

    spans, size, calls = M.cases("C")
    a = M.cases("A")[0]
    zeros = [s for s in spans if s.n == 0]
    ends = [s for s in spans if s.n and s.src + s.n == M.ARENA_BYTES]
    assert len(zeros) == 1848 // M.C_ZERO_EVERY == 36 and all(s.src is None for s in zeros)
    assert len(ends) == 16 * len(M.C_END_WORDS) == 48 and {s.src % 16 for s in ends} == set(range(16))
    assert {M.out_words(s) for s in ends} == set(M.C_END_WORDS)
    assert len(spans) == 1848 + 36 + 48 and _inside(spans)
    assert [(s.src, s.n) for s in spans if s.n and s.src + s.n != M.ARENA_BYTES] == [(s.src, s.n) for s in a]
    assert len(calls) == 3 and sorted(i for c in calls for i in c) == list(range(len(spans)))
    assert all(any(spans[i].n == 0 for i in c) and any(spans[i] in ends for i in c) for c in calls)
    assert M.disjoint(spans, size)


@pytest.mark.parametrize("group", M.GROUPS)
def test_destinations_do_not_overlap(group):
    spans, size, _ = M.cases(group)
    assert M.disjoint(spans, size)
    assert all(s.dst % 16 == 0 for s in spans) and size % 16 == 0
    # the plain statement of it: every byte of the buffer belongs to at most one room
    owner = np.zeros(size, dtype=np.uint8)
    for s in spans:
        owner[s.dst:s.dst + M.roundup16(s.n)] += 1
    assert owner.max() == 1
    # disjoint() itself refuses an overlap and a missing gap
    s0 = next(s for s in spans if s.n > 16)
    assert not M.disjoint(list(spans) + [M.Span(s0.src, 1, s0.dst + 16)], size)
    assert not M.disjoint([M.Span(0, 16, 16), M.Span(0, 16, 32)], 64)
    assert M.disjoint([M.Span(0, 16, 16), M.Span(0, 16, 48)], 80)


def _kernel_words(arena, src, n):
    """gather_kernel's arithmetic restated: aligned words i and i + 1 of the source (zero from
    in_words on), bytes [r, r + 16) of the pair, for every output word."""
    r = src % 16
    ow, iw = (n + 15) // 16, (r + n + 15) // 16
    words = np.zeros((ow + 1, 16), dtype=np.uint8)
    words[:iw] = arena[src - r:src - r + 16 * iw].reshape(iw, 16)
    pair = np.concatenate([words[:ow], words[1:ow + 1]], axis=1)
    return pair[:, r:r + 16].reshape(-1)


def test_image_builder_against_the_word_arithmetic(arena):
    spans, size, _ = M.cases("A")
    want, mask = M.expected_image(arena, spans, size)
    small = [s for s in spans if s.n <= 2100]
    assert len(small) == 88 * 9
    for s in small:
        assert s.src - s.src % 16 + 16 * M.in_words(s) <= M.ARENA_BYTES  # the words read lie inside the arena
        out = _kernel_words(arena, s.src, s.n)
        assert out.size == M.roundup16(s.n)
        assert np.array_equal(out[:s.n], arena[s.src:s.src + s.n]), s
        assert np.array_equal(out[:s.n], want[s.dst:s.dst + s.n]), s
        assert mask[s.dst:s.dst + s.n].all() and not mask[s.dst + s.n:s.dst + M.roundup16(s.n)].any()
    # all that is masked is the spans' tails; all that is not span bytes is canary
    assert int((~mask).sum()) == sum(M.roundup16(s.n) - s.n for s in spans)
    inside = np.zeros(size, dtype=bool)
    for s in spans:
        inside[s.dst:s.dst + s.n] = True
    assert (want[~inside] == M.CANARY).all()


def test_comparison_reports_wrong_bytes_and_stray_writes(arena):
    spans, size, _ = M.cases("B")
    want, mask = M.expected_image(arena, spans, size)
    assert M.compare("B", spans, want.copy(), want, mask) == []
    got = want.copy()
    s = spans[7]
    got[s.dst + s.n:s.dst + M.roundup16(s.n)] ^= 0xFF  # the room the contract leaves the kernel
    assert M.compare("B", spans, got, want, mask) == []
    got[s.dst + M.K_TILE + 5] ^= 1   # a byte of the span's second tile
    got[s.dst + M.K_TILE + 6] ^= 1   # the same span again: reported once
    got[s.dst + M.roundup16(s.n)] ^= 2  # the first canary byte after its room
    got[0] ^= 4                      # the buffer's first byte
    bad = M.compare("B", spans, got, want, mask)
    assert len(bad) == 3
    assert bad[0][0] == "B byte 0 outside every span (canary)" and bad[0][1] ^ bad[0][2] == 4
    assert f"r={s.src % 16} n={s.n} " in bad[1][0] and f"byte {M.K_TILE + 5} " in bad[1][0]
    assert "outside every span" in bad[2][0] and bad[2][1] ^ bad[2][2] == 2


def test_gather_spans_without_spans_and_without_pointers():
    assert lib.krk_gather_spans_dev(None, None, None, 0, None) == _capi.KRK_OK
    n = C.c_int(-1)
    _capi.check(lib.krk_device_count(C.byref(n)))
    p, one = np.zeros(1, dtype=np.uint64), np.ones(1, dtype=np.uint64)
    vpp = C.POINTER(C.c_void_p)
    rc = lib.krk_gather_spans_dev(p.ctypes.data_as(vpp), p.ctypes.data_as(vpp), one.ctypes.data_as(C.POINTER(C.c_uint64)),
                                  1, None)
    # one byte from NULL to NULL: refused for its pointers where a device is, for the device where none is
    assert rc == (_capi.KRK_EINVAL if n.value > 0 else _capi.KRK_ENODEV)
