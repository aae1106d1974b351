"""The conditions of tests/sha_share_matrix.py's cases, proved without a device: every case's
required plan is what the library's planners answer under its rates and threads, every named
edge of the host share and the tail handoff is present in the cases, the geometry getter answers,
and the sentinel-collision fixture is what tests/sha256_ref.py computes."""
import ctypes as C

import pytest

from kraken_amd import _capi
from kraken_amd import device as D
from kraken_amd._capi import lib
from tests import sha256_ref as R
from tests import sha_share_matrix as M


def test_geometry_getter():
    """krk_sha_offload_geometry: no device; the copy chunk is whole SHA-256 blocks, both rings have
    at least two buffers; NULL arguments are refused."""
    c, w, r = M.geometry()
    assert c > 0 and c % 64 == 0 and w >= 2 and r >= 2
    assert (M.CHUNK, M.DEPTH, M.RESUMER_DEPTH) == (c, w, r)
    a, b, d = C.c_uint64(), C.c_uint32(), C.c_uint32()
    for args in ((None, C.byref(b), C.byref(d)), (C.byref(a), None, C.byref(d)), (C.byref(a), C.byref(b), None)):
        assert lib.krk_sha_offload_geometry(*args) == _capi.KRK_EINVAL
    assert M.P_ODD not in (0, c) and c % M.P_ODD != 0 and c % M.MiB == 0


@pytest.mark.parametrize("case", M.ALL_CASES, ids=lambda c: c.name)
def test_case_plan(case):
    """plan_of: the library's planners, asked as offload_split asks them, give the case's plan --
    for a tail case that includes tails chosen over whole blobs (end_s < 0.95 x max(g, h))."""
    try:
        kind, plan = M.plan_of(case)
    finally:
        D.set_planner_rates(None), _capi.check(lib.krk_set_sha_plan(0))
    assert kind == ("tails" if case.tails is not None else "whole")
    assert D.planner_rates()["source"] != "set"  # the rates went back


def test_hand_checked_plans():
    """The plans checked by hand against planner_math.hpp with one thread, and the one where the
    whole-blob plan wins (a one-byte tail behind 256 bytes gains 3 of 260)."""
    for lens, t1 in (([300, 200, 64], (64, 136)), ([256, 119, 3], (64, 55)), ([256, 127, 3], (64, 63))):
        c = M.Case("hand", lens, 1, M.tail_rates(1), [(0, 0), (1, t1[0])], None, (64,), (0,))
        assert M.plan_of(c)[0] == "tails" and lens[1] - t1[0] == t1[1]
    c = M.Case("hand-whole", [256, 65, 0, 17], 1, M.tail_rates(1), None, {0}, (64,), (0,))
    assert M.plan_of(c) == ("whole", {0})


def _tails(cases, pred=lambda i, y, tau: True):
    return {tau for c in cases for i, y, tau in M.takeovers(c) if pred(i, y, tau)}


def test_block_edges_present():
    cases = M.BLOCK_EDGE_CASES
    assert all(c.threads == 1 for c in cases)
    assert _tails(cases, lambda i, y, tau: y > 0) >= {1, 55, 56, 63, 64, 65}
    starts = {y for c in cases for _, y, _ in M.takeovers(c)}
    assert 0 in starts and 64 in starts and any(y >= 128 for y in starts)
    for c in cases:
        taken = {i for i, _, _ in M.takeovers(c)}
        assert any(y == 0 for _, y, _ in M.takeovers(c)), c.name  # one chain starts at 0
        assert any(L > 1 and i not in taken for i, L in enumerate(c.lens)), c.name  # one stays on the GPU
        assert 0 in c.lens and 1 in c.lens, c.name
        assert c.piece_lengths == (64,)
    small = M.BY_NAME[M.SMALLEST_BLOCK_EDGE]
    assert sum(small.lens) == min(sum(c.lens) for c in cases)


def test_chunk_edges_present():
    Cb, cases = M.CHUNK, M.CHUNK_EDGE_CASES
    want = {Cb - 64, Cb - 1, Cb, Cb + 1, 2 * Cb, 2 * Cb + 1, 3 * Cb + 1}
    assert _tails(cases, lambda i, y, tau: y > 0) >= want
    assert {c.threads for c in cases} == {1, 2}
    assert -(-(3 * Cb + 1) // Cb) > M.DEPTH  # that tail's chunks wrap the copy ring
    for c in cases:
        assert M.MiB in c.piece_lengths and any(Cb % P for P in c.piece_lengths), c.name


def test_queue_cases_present():
    assert {c.threads for c in M.QUEUE_CASES} == {1, 2}
    for c in M.QUEUE_CASES:
        idx = [i for i, _, _ in M.takeovers(c)]
        assert len(idx) > c.threads and sum(1 for _, y, _ in M.takeovers(c) if y > 0) > c.threads, c.name
        assert idx != sorted(idx) and idx != sorted(idx, reverse=True), c.name  # the queue is not the slot order
        s = sorted(idx)
        assert all(b - a > 1 for a, b in zip(s, s[1:])), c.name  # not adjacent
        gaps = [L for a, b in zip(s, s[1:]) for L in c.lens[a + 1:b]]
        assert 0 in gaps and any(L > 0 for L in gaps), c.name  # empty blobs and GPU-only chains between


def test_alignment_fallback_and_whole_cases_present():
    assert [c.aligns for c in M.ALIGN_CASES] == [(a,) for a in range(16)]
    assert all(c.tails and any(y > 0 for _, y in c.tails) for c in M.ALIGN_CASES)
    for c in M.FALLBACK_CASES:  # threads at or above the chains a one-thread plan takes
        assert c.tails is None and c.threads >= len(M.BY_NAME[M.SENTINEL_CASE].tails)
    assert any(c.whole for c in M.FALLBACK_CASES) and any(not c.whole for c in M.FALLBACK_CASES)
    Cb = M.CHUNK
    big = [Cb - 1, Cb, Cb + 1, 2 * Cb - 1, 2 * Cb, 2 * Cb + 1, 3 * Cb, 3 * Cb + 1, 4 * Cb + 13]
    assert [c.threads for c in M.WHOLE_CASES] == [1, 3, len(big) + 3]
    for c in M.WHOLE_CASES:
        assert sorted(c.lens[i] for i in c.whole) == big
        rest = [L for i, L in enumerate(c.lens) if i not in c.whole]
        assert {0, 1, 63, 64} <= set(rest) and len(rest) == 204 and max(rest) < Cb - 1
    # shares of exactly DEPTH and DEPTH + 1 chunks: the ring filled once, and wrapped
    assert M.DEPTH * Cb in big and (M.DEPTH + 1) * Cb in big


def test_sentinel_fixture():
    """tests/golden/sha_sentinel_block.json recomputed: the collision block's midstate from the IV
    holds the note's fill in the recorded word, the control's holds it nowhere; both blocks are an
    8-byte little-endian counter and 56 zero bytes, and the control is the first such counter."""
    fx, fill = M.sentinel_fixture()
    assert fill == 0xFFFFFFFF
    for name, (block, word, mid, counter) in fx.items():
        assert len(block) == 64 and block == counter.to_bytes(8, "little") + bytes(56), name
        assert R.compress(R.IV, block) == mid, name
        assert word == (mid.index(fill) if fill in mid else -1), name
    assert fx["collision"][1] >= 0 and fx["control"][1] == -1 and fx["control"][3] == 0
    # the case the block goes into hands over a chain at 64 bytes: the block is its whole GPU prefix
    c = M.BY_NAME[M.SENTINEL_CASE]
    assert (1, 64) in [tuple(p) for p in c.tails] and c.threads == 1
