"""The window matrix harness (tests/window_matrix.py) checked where no GPU is: the restated schedule equals the
library's (krk_window_sched_*, no device needed) chunk for chunk on every list, every builder's lists hit the edges
they promise with the counts DESIGN.md section 6 quotes, and the comparison code finds and attributes one flipped
value, one stray store and one wrong gap word before any device is involved."""
import ctypes as C

import numpy as np
import pytest

from tests import window_matrix as M

MiB = M.MiB


def _all_cases():
    return [M.case_a(64), M.case_a(4096), M.case_a2(), M.case_a2(4096), M.case_a2x(), M.case_a2x(4096), M.case_b(),
            M.case_d(), M.case_d(65_537), M.case_e_single(), M.case_e_empty(), M.case_e_mixed(), M.case_f(16),
            M.case_f(4096)]


def _library_schedule(lens, W, cap):
    from kraken_amd._capi import check, lib
    L = np.asarray(lens, dtype=np.uint64)
    h = C.c_void_p()
    check(lib.krk_window_sched_new(L.ctypes.data_as(C.POINTER(C.c_uint64)), L.size, W, cap, C.byref(h)))
    room = max(1, min(cap, L.size))
    b, o, n = np.zeros(room, np.uint32), np.zeros(room, np.uint64), np.zeros(room, np.uint64)
    got, out = [], C.c_uint64()
    try:
        while True:
            check(lib.krk_window_sched_next(h, b.ctypes.data_as(C.POINTER(C.c_uint32)),
                                            o.ctypes.data_as(C.POINTER(C.c_uint64)),
                                            n.ctypes.data_as(C.POINTER(C.c_uint64)), room, C.byref(out)))
            if not out.value:
                return got
            k = out.value
            got.append(list(zip(b[:k].tolist(), o[:k].tolist(), n[:k].tolist())))
    finally:
        lib.krk_window_sched_free(h)


@pytest.mark.parametrize("case", _all_cases(), ids=lambda c: c.name)
def test_replay_equals_the_library_schedule(case):
    """align 64 (the C ABI's schedule has no other): chunk for chunk, every window."""
    cap = case.cap or 3  # group F's cases go through the packers; their lists are replayed here all the same
    assert M.replay(case.lens, case.W, cap)[0] == _library_schedule(case.lens, case.W, cap)


def test_replay_by_hand():
    """Three blobs, cap 2, W = 256: longest first, the third admitted when the shortest ends."""
    w, live = M.replay([100, 300, 0], 256, 2)
    assert w == [[(1, 0, 128), (0, 0, 100)], [(1, 128, 128), (2, 0, 0)], [(1, 256, 44)]] and live == 2
    assert M.replay([10_000], 256, 1, align=4096)[0] == [[(0, 0, 4096)], [(0, 4096, 4096)], [(0, 8192, 1808)]]
    assert M.replay([1000], 4096, 1, max_chunk=200)[0][0] == [(0, 0, 192)]
    p = M.pack_replay([20, 0, 300, 16], 256, 16)
    assert p == [[(0, 0, 20, 0), (2, 0, 224, 32)], [(2, 224, 76, 0), (3, 0, 16, 80)]]


def test_group_a_counts_and_edges():
    a = M.case_a(64)
    c = M.c_of(3)
    assert (c, M.c_of(3, 4096)) == (349_504, 348_160)
    windows, live = a.replay(64)
    assert (a.n, sum(a.counts), len(windows), live) == (126, 208_095, 100, 3)
    assert 66 * MiB < sum(a.lens) < 67 * MiB and max(a.counts) <= M.A_MAX_PIECES
    assert a.lens.count(0) == 11 and {(4 * c + 17, 65), (4 * c + 17, 64)}.isdisjoint(set(zip(a.lens, a.plens)))
    assert M.tags(windows, a.lens, a.plens) == M.ALL_TAGS - {"two chunk sizes in one chain"}
    d = M.case_a(4096)  # the O_DIRECT legs: the same edges 4 KiB apart
    windows, live = d.replay(4096)
    assert (d.n, len(windows), live) == (126, 100, 3)
    assert M.tags(windows, d.lens, d.plens, 4096) >= M.ALL_TAGS - {"two chunk sizes in one chain"}


def test_group_a2_chunk_sizes():
    c5 = M.c_of(5)
    assert c5 == 209_664
    for P in (None, 4096):
        a = M.case_a2(P)
        assert a.lens == (5 * c5 + 3, 4 * c5 + 1, 3 * c5, 2 * c5 + 64, c5 - 1) and set(a.plens) == {P or c5}
        windows, live = a.replay()
        assert [len(w) for w in windows] == [5, 4, 3, 2] and live == 5
        assert [ln for w in windows for b, _, ln in w if b == 0] == [209_664, 262_144, 349_504, 227_011]
        x = M.case_a2x(P)
        windows, live = x.replay()
        assert [len(w) for w in windows] == [5, 4, 3, 2, 1, 1] and live == 5
        assert [ln for w in windows for b, _, ln in w if b == 0] == [209_664, 262_144, 349_504, 524_288, MiB, 3]


def test_group_b_minimum_chunk():
    b = M.case_b()
    windows, live = b.replay()
    assert (b.n, live, len(windows)) == (17_084, 16_384, 8) and sum(b.counts) < 100_000
    assert set(b.lens) == set(M.B_LENGTHS) and {P for P in b.plens if P != MiB} == set(M.B_PIECES)
    assert [len(w) for w in windows][:2] == [16_384, 12_089]
    # c = 64 in the first windows: every SHA job there is one block, from state after window 0
    assert all(ln <= 64 for w in windows[:3] for _, _, ln in w)
    assert max(ln for w in windows for _, _, ln in w) > 64
    late = [b_ for b_, off, _ in windows[1] if off == 0]
    assert len(late) == b.n - M.B_CAP == 700
    assert sum(1 for w in windows if len(w) > M.DIRECT_MAX) == 8  # every window is wide: gathered, or staged
    # O_DIRECT: the 4 KiB minimum chunk carries every blob whole
    w4, live4 = b.replay(4096)
    assert [len(w) for w in w4] == [16_384, 700] and live4 == 16_384


def test_group_d_splits_inside_chunks():
    d = M.case_d()
    c9 = 3 * MiB
    assert d.lens == (3 * c9 + 4097, 2 * c9 + 5, c9 + 1, 70_001, 0) and d.W == 9 * MiB
    for align in (64, 4096):
        windows, live = d.replay(align)
        assert live == 3 and len(windows) == 4
        full = [w for w in windows if all(ln == c9 for _, _, ln in w) and len(w) == 3]
        assert full and all(sum(ln for _, _, ln in w) >= M.SPLIT_MIN for w in full)
        for T in range(2, 17):
            for padded, read in ((False, False), (False, True), (True, True)):
                spans = M.cut_spans([c9] * 3, T, padded, read)
                assert sum(b - a for s in spans for _, a, b in s) == 3 * c9
                # per-thread spans begin inside chunks (three threads alone cut on the chunk edges, and four
                # readers, whose 2.25 MiB spans round up to 3 MiB)
                inside = [s[0] for s in spans[1:] if s and s[0][1] != 0]
                assert inside or T == 3 or (read and T == 4), (T, padded, read)
    # O_DIRECT: a last chunk that is no 4 KiB multiple, followed by another chunk in its window
    windows = d.replay(4096)[0]
    assert any(off + ln == d.lens[b] and ln % 4096 and k + 1 < len(w) and w[k + 1][2]
               for w in windows for k, (b, off, ln) in enumerate(w))


def test_group_e_layouts():
    for base in (M.case_a2(4096), M.case_d(65_537)):
        e = M.case_e_layout(base)
        assert e.lens == base.lens and min(e.soff) == 1000 == e.span[0]
        order = sorted((i for i in range(e.n) if e.counts[i]), key=lambda i: e.soff[i])
        assert order == [i for i in reversed(range(e.n)) if e.counts[i]]
        for a, b in zip(order, order[1:]):
            assert e.soff[b] - (e.soff[a] + e.counts[a]) == 7
        img = M.sums_image(e, "zero")
        gap = np.ones(img.size, bool)
        gap[:M.CANARY_W + 1000] = gap[M.CANARY_W + e.span[1]:] = False
        for o, k in zip(e.soff, e.counts):
            gap[M.CANARY_W + o:M.CANARY_W + o + k] = False
        assert gap.sum() == 7 * (sum(1 for k in e.counts if k) - 1)
        assert (img[gap] == 0).all() and (M.sums_image(e, "keep")[gap] == 0xFFFFFFFF).all()
        assert (img[:M.CANARY_W + 1000] == 0xFFFFFFFF).all() and (img[M.CANARY_W + e.span[1]:] == 0xFFFFFFFF).all()
    m = M.case_e_mixed()
    longest = sorted(range(m.n), key=lambda i: -m.lens[i])[:3]
    assert sorted(longest) == list(M.E_HOST) and m.lens.count(0) == 1
    rest = [i for i in range(m.n) if i not in M.E_HOST]
    windows, live = m.replay(64, rest)
    assert live == 3 and {b for w in windows for b, _, _ in w} == set(rest)
    assert M.case_e_single().n == 1 and set(M.case_e_empty().lens) == {0}


def test_group_e_host_share_under_the_injected_rates():
    """offload_plan with e_rates on four threads takes exactly the three longest blobs, in every host mode (no device:
    the planner is arithmetic over the injected rates)."""
    from kraken_amd import device as D
    m = M.case_e_mixed()
    D.set_planner_rates(M.e_rates(D.planner_rates()))
    try:
        for mode in (D.OFFLOAD_HOST_SHA, D.OFFLOAD_HOST_WHOLE, D.OFFLOAD_HOST_FILES):
            assert sorted(D.sha_offload_plan(m.lens, 4, mode=mode)[0].tolist()) == list(M.E_HOST), mode
    finally:
        D.set_planner_rates(None)


@pytest.mark.parametrize("place", [16, 4096])
def test_group_f_packed_edges(place):
    f = M.case_f(place)
    windows = M.pack_replay(f.lens, M.W1, place)
    assert M.pack_tags(windows, f.lens, f.plens, place) == M.F_TAGS
    assert len(windows) >= 10 and set(f.plens) == set(M.F_PIECES) and sum(f.counts) < 10_000
    # every portion starts on a multiple of place, no window overflows, every byte is carried once and in order
    pos = [0] * f.n
    for w in windows:
        for b, boff, take, fill in w:
            assert fill % place == 0 and fill + take <= M.W1 and boff == pos[b] and take > 0
            pos[b] += take
    assert pos == list(f.lens)
    # the GPU shares: everything, half, and one that ends inside a blob at a piece edge
    assert M.gpu_share(f, 1)[0] == f.counts and M.gpu_share(f, 1)[1] == sum(f.lens)
    q, g = M.gpu_share(f, 0.5)
    assert 0 < g - sum(f.lens) / 2 <= max(f.plens) and q != f.counts
    q, g = M.gpu_share(f, M.f_mid_fraction(f))
    cut = [i for i in range(f.n) if 0 < q[i] < f.counts[i]]
    assert len(cut) == 1 and q[cut[0]] == 3 and all(q[i] == f.counts[i] for i in range(cut[0]))
    assert all(q[i] == 0 for i in range(cut[0] + 1, f.n))
    assert g == sum(f.lens[:cut[0]]) + 3 * f.plens[cut[0]]


def _filled(case, gaps="zero", crc=True):
    out = M.Outputs(case, crc=crc)
    if crc:
        out.sums[:] = M.sums_image(case, gaps)
    out.dig[:] = M.digests_image(case)
    return out


def test_references_are_hashlib_and_zlib():
    import hashlib
    import zlib
    a = M.case_a2x(4096)
    for i in (0, 4):
        data = M.blob_bytes(a, i).tobytes()
        assert len(data) == a.lens[i]
        assert bytes(M.ref_digests(a)[i]) == hashlib.sha256(data).digest()
        assert M.ref_sums(a)[i].tolist() == [zlib.crc32(data[k:k + 4096]) for k in range(0, len(data), 4096)]
    e = M.case_e_empty()
    assert all(bytes(d) == hashlib.sha256(b"").digest() for d in M.ref_digests(e)) and e.span == (0, 0)


def test_comparison_finds_and_attributes():
    case = M.case_e_layout(M.case_a2(4096))
    windows = case.replay()[0]
    assert M.mismatches(_filled(case), "zero", windows) == []
    assert M.mismatches(_filled(case, "keep"), "keep", windows) == []
    # one flipped sum: the blob, the piece and the window, slot and chunk that carried its bytes
    out = _filled(case)
    piece = (M.c_of(5) + 5000) // 4096  # in blob 0's second chunk (window 1, slot 1)
    out.sums[M.CANARY_W + case.soff[0] + piece] ^= 1
    bad = M.mismatches(out, "zero", windows)
    assert len(bad) == 1 and "blob 0 " in bad[0] and "piece %d " % piece in bad[0], bad
    assert "window 1 (slot 1) chunk 0 of 4" in bad[0] and "window 0" not in bad[0], bad
    # a piece cut by a window boundary names both windows
    out = _filled(case)
    out.sums[M.CANARY_W + case.soff[0] + M.c_of(5) // 4096] ^= 1 << 31
    bad = M.mismatches(out, "zero", windows)
    assert len(bad) == 1 and "window 0 (slot 0)" in bad[0] and "window 1 (slot 1)" in bad[0], bad
    # stray stores: a canary on each side, below the span, and a gap word under either rule
    for word, kind in ((M.CANARY_W - 1, "canary before"), (M.CANARY_W + case.span[1], "canary after"),
                       (M.CANARY_W + 999, "outside the span"),
                       (M.CANARY_W + case.soff[4] + case.counts[4], "gap word")):
        for gaps in ("zero", "keep"):
            out = _filled(case, gaps)
            out.sums[word] = 0x12345678
            bad = M.mismatches(out, gaps, windows)
            assert len(bad) == 1 and kind in bad[0], (kind, gaps, bad)
    assert len(M.mismatches(_filled(case, "keep"), "zero", windows)) >= 2  # the two rules differ on every gap word
    # digests: one flipped bit in one digest, one stray byte after the array
    out = _filled(case)
    out.dig[M.CANARY_B + 32 * 3 + 31] ^= 0x80
    bad = M.mismatches(out, "zero", windows)
    assert len(bad) == 1 and "digest of blob 3 " in bad[0] and "window 1 (slot 1) chunk 3 of 4" in bad[0], bad
    out = _filled(case)
    out.dig[-1] = 0
    assert len(M.mismatches(out, "zero", windows)) == 1
    # everything wrong: a bounded report, whatever the size of the batch (B: 17,084 digests, 35,619 sums)
    b = M.case_b()
    out = _filled(b)
    out.dig[M.CANARY_B:-M.CANARY_B] ^= 1
    out.sums[M.CANARY_W:-M.CANARY_W] ^= 1
    bad = M.mismatches(out, "zero", b.replay()[0])
    assert len(bad) == 2 * (6 + 1) and "17084 digests differ" in bad[-1] and "35619 sums words differ" in bad[6], bad[-1]
    # digests only (krk_sha256_host): no sums array to compare
    assert M.mismatches(_filled(case, crc=False), "zero", windows) == []


def test_piece_sums_host_on_host_threads_leaves_gap_words(monkeypatch):
    """No device: pageable blobs stay on the host threads, which write each blob's own words and nothing else --
    canaries, the words below the span and the gap words inside it keep what the caller had there."""
    monkeypatch.delenv("KRK_CRC_GPU_FRACTION", raising=False)
    case = M.case_e_layout(M.case_a2(4096))
    out = M.call("piece_sums_host", case, M.MemSource(case, misalign=3))
    assert M.GAPS["piece_sums_host"] == "keep" and M.mismatches(out, "keep") == []


def test_statistics_rule():
    a = M.case_a2x()
    st = {"windows": 6, "max_live": 5, "direct_windows": 0, "gather_windows": 0, "direct_reads": False, "host_blobs": 0}
    assert M.stats_mismatches(st, a, 64, False) == []
    assert M.stats_mismatches(dict(st, direct_windows=6), a, 64, True) == []
    assert len(M.stats_mismatches(dict(st, windows=5), a, 64, False)) == 1
    assert len(M.stats_mismatches(st, a, 64, True)) == 1
    assert len(M.stats_mismatches(dict(st, gather_windows=1), a, 64, False)) == 1
    assert M.stats_mismatches(dict(st, gather_windows=6), a, 64, False, registered=True) == []
    assert len(M.stats_mismatches(dict(st, gather_windows=7), a, 64, False, registered=True)) == 1
    assert len(M.stats_mismatches(st, a, 64, False, direct_reads=True)) == 1
    b = M.case_b()
    wide = {"windows": 8, "max_live": 16_384, "direct_windows": 0, "gather_windows": 8, "direct_reads": False,
            "host_blobs": 0}
    assert M.stats_mismatches(wide, b, 64, True, wide_gather=True) == []
    assert M.stats_mismatches(dict(wide, gather_windows=0), b, 64, True, wide_gather=False) == []
