"""The window matrix: the host-resident window passes pinned at their chunk, slot and transport edges.

What is pinned: `run_windows` (kraken_amd/csrc/window_pass.cpp) under both of its schedules -- WindowSched for the
digest calls of windows.cpp (krk_metainfo_digest_host, krk_sha256_host, krk_metainfo_digest_files), PackSched for the
CRC-only calls of crc_host.cpp (krk_piece_sums_host, krk_piece_sums_files) -- with its memory and file sources, and
the slot ring, par_copy and par_read of kraken_amd/csrc/staging.hpp.  That code decides what
the SHA-256 and CRC kernels are asked to do window by window: SHA jobs chained from midstates, CRC items for byte
ranges that start and end inside pieces, chunks placed 16 B or 4 KiB apart in a slot reused every third window, one of
four ways up (staged, a DMA a chunk, the gather over page-locked or over registered pageable memory) and three ways
to read a file (buffered, O_DIRECT by AIO, O_DIRECT by synchronous reads).

How: `replay` and `pack_replay` restate the two schedules in plain Python, `tags` / `pack_tags` name every edge a list
of lengths makes the schedule hit, and each builder asserts the tags it promises, so an edit of a list cannot lose an
edge unnoticed.  References are hashlib.sha256 of each blob and zlib.crc32 of each piece; nothing comes from the code
under test.  Every output array carries 16 canary words (sums) or 64 canary bytes (digests) on both sides, is
prefilled with 0xFF and compared WHOLE with a numpy image, and a mismatch is reported with the blob, the piece and the
windows, slots and chunk offsets its bytes went through.  After each call krk_windows_last_* must equal the replay.

Groups (W = 1 MiB unless said; c(k, align) = (W // k) // align * align):
  A   cuts against pieces and SHA blocks: 14 lengths x 9 piece lengths around c(3), KRK_LIVE_CAP=3
  A2  five blobs under KRK_LIVE_CAP=5: the live count falls 5 -> 2 and one chain sees four chunk sizes; A2x carries
      it to 5 -> 1 over six windows, five chunk sizes and a 3-byte last chunk
  B   the minimum chunk: 17,084 short blobs under KRK_LIVE_CAP=16384, c = 64, 700 admitted late
  C   A, A2 and B through every way up (LEGS), and A under ring depths 2 and 4 in child processes
  D   9 MiB windows under KRK_LIVE_CAP=3: par_copy / par_read cut the window into per-thread spans
  E   layout and mixing: permuted and gapped sums offsets from 1,000, n = 1, empty blobs only, a host-offload subset
  F   the CRC-only packers, lengths built against pack_replay, three GPU shares

Importing this module loads no library; the runners import kraken_amd._capi when called."""
import ctypes as C
import functools
import hashlib
import json
import os
import sys
import tempfile
import time
import zlib
from dataclasses import dataclass

import numpy as np

MiB = 1 << 20
W1 = MiB      # KRK_WINDOW_MB=1, the smallest window there is
RING = 3      # staging slots (KRK_STAGING_WINDOWS' default)
CANARY_W = 16  # canary words around a sums array
CANARY_B = 64  # canary bytes around a digests array
DIRECT_MAX = 64  # staging.hpp kDirectMaxCalls: page-locked windows of more chunks are gathered or staged
SPLIT_MIN = 8 * MiB  # window_math.hpp kSplitMinBytes: smaller fills run on one thread


def c_of(k, align=64, W=W1):
    """The chunk of a window with k blobs live."""
    return max(align, (W // k) // align * align)


# ------------------------------------------------------------------------------ the two schedules, restated
def replay(lens, W, cap, align=64, max_chunk=None, blobs=None):
    """WindowSched restated: (windows, max_live); a window is a list of (blob, off, len) in admission order.
    blobs: the indices that go through the windows (default all)."""
    align, cap = max(align, 64), max(cap, 1)
    order = sorted(range(len(lens)) if blobs is None else blobs, key=lambda i: -lens[i])  # stable
    q, live, windows, max_live = 0, [], [], 0
    while True:
        while len(live) < cap and q < len(order):
            live.append((order[q], 0))
            q += 1
        if not live:
            return windows, max_live
        max_live = max(max_live, len(live))
        c = W // len(live) if max_chunk is None else min(max_chunk, W // len(live))
        c = max(align, c // align * align)
        win, keep = [], []
        for b, pos in live:
            take = min(c, lens[b] - pos)  # an empty blob takes a 0-byte chunk
            win.append((b, pos, take))
            if pos + take < lens[b]:
                keep.append((b, pos + take))
        live = keep
        windows.append(win)


def pack_replay(lens, W, place):
    """PackSched (window_math.hpp, the CRC-only calls of crc_host.cpp) restated: windows of (blob, boff, take, fill),
    fill rounded up to `place` (16: memory, 4096: files) after every portion; a zero-length blob takes nothing."""
    windows, bi, boff, n = [], 0, 0, len(lens)
    while bi < n:
        fill, win = 0, []
        while bi < n and fill < W:
            take = min(lens[bi] - boff, W - fill)
            if take:
                win.append((bi, boff, take, fill))
            fill += take
            boff += take
            fill = -(-fill // place) * place
            if boff >= lens[bi]:
                bi, boff = bi + 1, 0
        windows.append(win)
    return windows


def cut_spans(task_lens, T, padded, read):
    """par_copy (read=False) / par_read (read=True) restated: the (task, a, b) pieces of each thread's span."""
    pad = (lambda n: (n + 4095) & ~4095) if padded else (lambda n: n)
    total = sum(pad(n) for n in task_lens)
    span = -(-total // T)
    if read:
        span = max(MiB, -(-span // MiB) * MiB)
    out = []
    for i in range(-(-total // span)):
        lo, hi, pos, pieces = i * span, min(total, (i + 1) * span), 0, []
        for t, n in enumerate(task_lens):
            if pos >= hi:
                break
            a, b = max(lo, pos), min(hi, pos + n)
            if a < b:
                pieces.append((t, a - pos, b - pos))
            pos += pad(n)
        out.append(pieces)
    return out


# ------------------------------------------------------------------------------ the edges a schedule hits
def _cls(r, P):
    return "0" if r == 0 else "1" if r == 1 else "P-1" if r == P - 1 else "other"


SHA_TAILS = (0, 1, 55, 56, 63)


def tags(windows, lens, plens, place=16, ring=RING):
    """Every edge the windows hit, as a set of names (the module docstring's list)."""
    out, sizes = set(), {}
    for win in windows:
        n = len(win)
        if n == 1:
            out.add("one-chunk window")
        chains = any(off > 0 or off + ln < lens[b] for b, off, ln in win)
        for k, (b, off, ln) in enumerate(win):
            L, P = lens[b], plens[b]
            end, final = off + ln, off + ln == L
            if L == 0:
                out.add("empty blob alone" if n == 1 else "empty blob among many")
                continue
            if P >= 3:
                if off:
                    out.add("off%P=" + _cls(off % P, P))
                if not final:
                    out.add("end%P=" + _cls(end % P, P))
            if off % P and end % P:
                if off // P == (end - 1) // P and not final:
                    out.add("chunk inside one piece")
                if -(-off // P) + 1 <= end // P:
                    out.add("partial, whole, partial")
            if final and off and ln % 64 in SHA_TAILS:
                out.add("final from state, len%%64=%d" % (ln % 64))
            if final and off == 0 and chains:
                out.add("whole blob beside chains")
            if ln % place and k + 1 < n:
                out.add("unplaced chunk followed")
            if not final:
                sizes.setdefault(b, set()).add(ln)
    if any(len(s) > 1 for s in sizes.values()):
        out.add("two chunk sizes in one chain")
    if len(windows) >= 3 * ring + 1:
        out.add("3 x ring + 1 windows")
    return out


ALL_TAGS = frozenset(
    ["off%P=" + c for c in ("0", "1", "P-1", "other")] + ["end%P=" + c for c in ("0", "1", "P-1", "other")] +
    ["chunk inside one piece", "partial, whole, partial", "whole blob beside chains", "unplaced chunk followed",
     "empty blob among many", "empty blob alone", "two chunk sizes in one chain", "one-chunk window",
     "3 x ring + 1 windows"] + ["final from state, len%%64=%d" % r for r in SHA_TAILS])


def pack_tags(windows, lens, plens, place, W=W1, ring=RING):
    """The edges of a packed schedule (group F)."""
    out = set()
    if len(windows) >= 10:
        out.add("ten windows")
    if len(windows) >= 3 * ring + 1:  # every slot of the ring refilled three times over
        out.add("3 x ring + 1 windows")
    prev_zero = False
    for L in lens:
        if L and prev_zero:
            out.add("empty blob between")
        prev_zero = L == 0
    for win in windows:
        for b, boff, take, fill in win:
            P, L = plens[b], lens[b]
            if boff and fill == 0:  # the window boundary fell inside blob b at boff
                for name, r in (("at", 0), ("one place before", P - place), ("one place after", place)):
                    if boff % P == r % P and P > 2 * place:
                        out.add("boundary %s a piece edge" % name)
            if boff + take == L and fill + take == W:
                out.add("blob ends at the window's end")
            if take < place:
                out.add("portion shorter than place")
    return out


F_TAGS = frozenset(["ten windows", "3 x ring + 1 windows", "empty blob between", "boundary at a piece edge",
                    "boundary one place before a piece edge", "boundary one place after a piece edge",
                    "blob ends at the window's end", "portion shorter than place"])


# ------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    name: str
    lens: tuple
    plens: tuple
    soff: tuple
    window_mb: int
    cap: int
    seed: int
    align: int = 64      # the alignment the lengths were built for (the replay takes the leg's)
    promised: frozenset = frozenset()

    @property
    def n(self):
        return len(self.lens)

    @property
    def W(self):
        return self.window_mb * MiB

    @property
    def counts(self):
        return [-(-L // P) for L, P in zip(self.lens, self.plens)]

    @property
    def span(self):
        """(lo, hi): the sums span the call owns."""
        r = [(o, o + k) for o, k in zip(self.soff, self.counts) if k]
        return (min(a for a, _ in r), max(b for _, b in r)) if r else (0, 0)

    def replay(self, align=64, blobs=None):
        return replay(self.lens, self.W, self.cap, align, blobs=blobs)

    def with_layout(self, name, soff):
        return Case(name, self.lens, self.plens, tuple(soff), self.window_mb, self.cap, self.seed, self.align,
                    self.promised)


def _dense(lens, plens):
    o, out = 0, []
    for L, P in zip(lens, plens):
        out.append(o)
        o += -(-L // P)
    return tuple(out)


def _case(name, lens, plens, window_mb, cap, seed, align=64, promised=(), place=None):
    case = Case(name, tuple(lens), tuple(plens), _dense(lens, plens), window_mb, cap, seed, align, frozenset(promised))
    got = tags(case.replay(align)[0], case.lens, case.plens, place or (16 if align == 64 else align))
    missing = case.promised - got
    assert not missing, (name, sorted(missing))
    return case


A_MAX_PIECES = 20_000


@functools.lru_cache(maxsize=None)
def case_a(align=64):
    """Group A: cuts against pieces and SHA blocks around c = c(3, align)."""
    c = c_of(3, align)
    lengths = [3 * c, 3 * c + 1, 2 * c + 55, 2 * c + 56, 2 * c + 63, 2 * c + 64, 2 * c + 65, c, c + 1, c - 1,
               4 * c + 17, 65, 1, 0]
    pieces = [c, c - 1, c + 1, 2 * c + 128, c // 2, 4096, 65, 64, 3 * c]
    pairs = [(L, P) for L in lengths for P in pieces if -(-L // P) <= A_MAX_PIECES] + [(0, 4096), (0, 65)]
    return _case("A/align%d" % align, [L for L, _ in pairs], [P for _, P in pairs], 1, 3, 101, align,
                 ALL_TAGS - {"two chunk sizes in one chain"})


@functools.lru_cache(maxsize=None)
def case_a2(P=None):
    """Group A2: five blobs under KRK_LIVE_CAP=5; P = c5 (default) or 4096.  The live count falls 5 -> 2 over four
    windows (c = 209,664, 262,144, 349,504, 524,288), so the longest chain sees three non-final chunk sizes and a
    fourth in its last chunk."""
    c5 = c_of(5)
    lens = [5 * c5 + 3, 4 * c5 + 1, 3 * c5, 2 * c5 + 64, c5 - 1]
    return _case("A2/P%d" % (P or c5), lens, [P or c5] * 5, 1, 5, 102, 64,
                 ["two chunk sizes in one chain", "final from state, len%64=1"])


@functools.lru_cache(maxsize=None)
def case_a2x(P=None):
    """Group A2, carried to the end: lengths on the running sums of c(5), c(4), ... c(1), so that one blob finishes in
    each of the first four windows and the live count falls 5 -> 1 over six windows: the longest chain sees all five
    chunk sizes before its 3-byte last chunk, alone in the last two windows."""
    s = [0]
    for k in (5, 4, 3, 2, 1):
        s.append(s[-1] + c_of(k))
    lens = [s[5] + 3, s[3] + 1, s[3], s[1] + 64, s[1] - 1]
    case = _case("A2x/P%d" % (P or c_of(5)), lens, [P or c_of(5)] * 5, 1, 5, 109, 64,
                 ["two chunk sizes in one chain", "one-chunk window"])
    windows = case.replay()[0]
    assert [len(w) for w in windows] == [5, 4, 3, 2, 1, 1]
    assert [ln for w in windows for b, _, ln in w if b == 0] == [c_of(k) for k in (5, 4, 3, 2, 1)] + [3]
    return case


B_LENGTHS = (0, 1, 55, 56, 63, 64, 65, 127, 128, 129, 191, 192, 193, 640, 641, 1023, 1024, 1025)
B_PIECES = (1, 3, 63, 64, 65, 128)
B_BLOBS, B_CAP = 17_084, 16_384


@functools.lru_cache(maxsize=None)
def case_b():
    """Group B: the minimum chunk -- c = 64 while 16,384 blobs are live, 700 admitted late."""
    rng = np.random.default_rng(103)
    lens = [B_LENGTHS[k] for k in rng.integers(0, len(B_LENGTHS), B_BLOBS)]
    plens = [B_PIECES[(i // 64) % len(B_PIECES)] if i % 64 == 0 else MiB for i in range(B_BLOBS)]
    return _case("B", lens, plens, 1, B_CAP, 103, 64,
                 ["final from state, len%%64=%d" % r for r in (0, 1, 63)] +  # 55 and 56 only as whole blobs
                 ["empty blob among many", "whole blob beside chains", "unplaced chunk followed",
                  "two chunk sizes in one chain", "off%P=0", "off%P=1", "off%P=P-1", "off%P=other"])


D_WINDOW_MB = 9


@functools.lru_cache(maxsize=None)
def case_d(P=MiB):
    """Group D: windows wide enough for par_copy / par_read to split (P = 1 MiB or 65,537)."""
    c9 = c_of(3, 4096, D_WINDOW_MB * MiB)
    assert c9 == c_of(3, 64, D_WINDOW_MB * MiB)
    lens = [3 * c9 + 4097, 2 * c9 + 5, c9 + 1, 70_001, 0]
    return _case("D/P%d" % P, lens, [P] * 5, D_WINDOW_MB, 3, 104, 64, ["empty blob among many", "unplaced chunk followed"])


def case_e_layout(base):
    """Group E: base's blobs with sums offsets permuted (reverse order), 7 words apart, from word 1,000."""
    o, soff = 1000, [0] * base.n
    for i in reversed(range(base.n)):
        soff[i] = o
        o += base.counts[i] + 7 if base.counts[i] else 0
    return base.with_layout("E/" + base.name, soff)


def case_e_single():
    c = c_of(3)
    return _case("E/n=1", [2 * c + 55], [4096], 1, 3, 105)


def case_e_empty():
    return _case("E/empty", [0] * 5, [4096, 65, 1, MiB, 64], 1, 3, 106)


E_HOST = (1, 4, 8)  # where case_e_mixed puts its three longest blobs


@functools.lru_cache(maxsize=None)
def case_e_mixed():
    """Group E: D's and A2's blobs in one batch, the three longest (the host offload's share under E_RATES on four
    threads) at indices E_HOST, so the windows run over a batch with holes."""
    d, a2 = case_d(65_537), case_a2(4096)
    small = [(a2.lens[k], 4096) for k in range(5)] + [(70_001, 65_537), (0, 65_537)]
    big = [(d.lens[k], 65_537) for k in range(3)]
    pairs, bi, si = [], 0, 0
    for i in range(10):
        if i in E_HOST:
            pairs.append(big[bi])
            bi += 1
        else:
            pairs.append(small[si])
            si += 1
    return _case("E/mixed", [L for L, _ in pairs], [P for _, P in pairs], 1, 3, 107)


def e_rates(rates):
    """Injected planner rates under which four host threads take exactly case_e_mixed's three longest blobs, in every
    host mode (planner_math.hpp offload_plan: with them on the host both sides end within a few ms of each other, and
    a fourth blob only lengthens the host side)."""
    return dict(rates, sha_stream_bps=[50e6, 50e6, 50e6], host_sha_bps=0.4e9, host_crc_bps=0.4e9, host_copy_bps=10e9,
                h2d_bps=50e9, d2h_bps=50e9, cus=256)


F_PIECES = (W1, W1 - 16, 65_536, 4096, 65)


@functools.lru_cache(maxsize=None)
def case_f(place):
    """Group F: lengths built against pack_replay so that a window boundary falls in a blob at a piece edge, one
    `place` before and one after it, a blob ends exactly at a window's end, portions are shorter than `place`,
    zero-length blobs sit between the others, and there are at least ten windows."""
    lens, plens = [], []

    def fill():
        w = pack_replay(lens, W1, place)
        if not w or not w[-1]:
            return 0
        _, _, take, at = w[-1][-1]
        return -(-(at + take) // place) * place % W1

    def add(L, P):
        lens.append(L)
        plens.append(P)

    def straddle(at, tail, P):
        """A blob the window boundary cuts at byte `at` (a multiple of place), `tail` bytes going on after it."""
        room = W1 - fill()
        if room < at:
            add(room, 4096)  # ends exactly at the window's end
            room = W1
        if room > at:
            add(room - at, 65_536)
        add(at + tail, P)

    add(1, 65)  # a portion shorter than place, first in its window
    add(0, 4096)
    add(200_000, 65)
    for P in (65_536, 4096):
        for at in (P, 2 * P - place, P + place):
            if at % P or P > 2 * place:
                straddle(at, 100_000 + 7, P)
            add(0, 65)
    straddle(65_536, 5, 65_536)  # the tail portion is shorter than place
    add(3, 65)
    add(W1 - fill(), W1 - 16)  # ends exactly at the window's end
    add(0, W1)
    add(3 * W1 + 17, W1)       # whole windows of one blob
    add(2 * W1, W1 - 16)
    add(0, 4096)
    add(70_001, 65)
    case = Case("F/place%d" % place, tuple(lens), tuple(plens), _dense(lens, plens), 1, 0, 108 + place, place, F_TAGS)
    got = pack_tags(pack_replay(case.lens, W1, place), case.lens, case.plens, place)
    assert not F_TAGS - got, (case.name, sorted(F_TAGS - got))
    return case


def gpu_share(case, fraction):
    """krk_piece_sums_host's split restated: (pieces of each blob the GPU takes, GPU bytes).  Whole pieces go to the
    GPU, in order, while its bytes are below fraction x the batch's (the same double arithmetic)."""
    quota, g, q = float(fraction) * float(sum(case.lens)), 0.0, []
    for L, P in zip(case.lens, case.plens):
        k, np_ = 0, -(-L // P)
        while k < np_ and g < quota:
            g += float(min(P, L - k * P))
            k += 1
        q.append(k)
    return q, int(g)


def f_mid_fraction(case):
    """A GPU share that ends inside a blob, at a piece edge: half a piece short of three pieces into the first blob of
    at least four pieces past the batch's first quarter."""
    before, total = 0, sum(case.lens)
    for L, P in zip(case.lens, case.plens):
        if before > total // 4 and -(-L // P) >= 4 and P >= 4096:
            return repr((before + 2.5 * P) / total)
        before += L
    raise AssertionError("no blob to end the share in")


# ------------------------------------------------------------------------------ bytes and references
@functools.lru_cache(maxsize=None)
def _content(seed, lens):
    off = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])
    data = np.frombuffer(np.random.default_rng(seed).bytes(int(off[-1]) or 1), dtype=np.uint8)
    return data, off


def blob_bytes(case, i):
    data, off = _content(case.seed, case.lens)
    return data[int(off[i]):int(off[i + 1])]


@functools.lru_cache(maxsize=None)
def _ref_digests(seed, lens):
    data, off = _content(seed, lens)
    mv = memoryview(data)
    out = np.empty((len(lens), 32), dtype=np.uint8)
    for i in range(len(lens)):
        out[i] = np.frombuffer(hashlib.sha256(mv[int(off[i]):int(off[i + 1])]).digest(), dtype=np.uint8)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _ref_sums(seed, lens, plens):
    data, off = _content(seed, lens)
    mv = memoryview(data)
    out = []
    for i, (L, P) in enumerate(zip(lens, plens)):
        base = int(off[i])
        a = np.array([zlib.crc32(mv[base + k:base + min(k + P, L)]) for k in range(0, L, P)], dtype=np.uint32)
        a.setflags(write=False)
        out.append(a)
    return out


def ref_digests(case):
    return _ref_digests(case.seed, case.lens)


def ref_sums(case):
    return _ref_sums(case.seed, case.lens, case.plens)


def sums_image(case, gaps):
    """The whole sums array a call must leave: canaries, the span's gap words zero (gaps="zero") or untouched
    (gaps="keep"), every blob's sums at its offset."""
    lo, hi = case.span
    img = np.full(CANARY_W + hi + CANARY_W, 0xFFFFFFFF, dtype=np.uint32)
    if gaps == "zero":
        img[CANARY_W + lo:CANARY_W + hi] = 0
    for o, a in zip(case.soff, ref_sums(case)):
        img[CANARY_W + o:CANARY_W + o + a.size] = a
    return img


def digests_image(case):
    img = np.full(CANARY_B + 32 * case.n + CANARY_B, 0xFF, dtype=np.uint8)
    img[CANARY_B:CANARY_B + 32 * case.n] = ref_digests(case).reshape(-1)
    return img


class Outputs:
    """The caller's arrays of one call: canaries on both sides, everything prefilled with 0xFF."""

    def __init__(self, case, crc=True, dig=True):
        self.case = case
        self.sums = np.full(CANARY_W + case.span[1] + CANARY_W, 0xFFFFFFFF, dtype=np.uint32) if crc else None
        self.dig = np.full(CANARY_B + 32 * case.n + CANARY_B, 0xFF, dtype=np.uint8) if dig else None

    @property
    def sums_p(self):
        return C.cast(self.sums.ctypes.data + 4 * CANARY_W, C.POINTER(C.c_uint32))

    @property
    def dig_p(self):
        return C.cast(self.dig.ctypes.data + CANARY_B, C.POINTER(C.c_uint8))


def _where(case, windows, b, lo, hi, place, ring):
    """The windows, slots and chunks that carried bytes [lo, hi) of blob b."""
    out = []
    for wi, win in enumerate(windows or ()):
        at = 0
        for k, ch in enumerate(win):
            blob, off, ln = ch[:3]
            pos = ch[3] if len(ch) > 3 else at
            if blob == b and (off < hi and off + ln > lo or (ln == 0 and lo == hi)):
                out.append("window %d (slot %d) chunk %d of %d at +%d: bytes [%d, %d)" %
                           (wi, wi % ring, k, len(win), pos, off, off + ln))
            at += -(-ln // place) * place
    return out[:6]


def mismatches(out, gaps="zero", windows=None, place=16, ring=RING, limit=6):
    """Every difference between a call's arrays and their images, each with where it came from."""
    case, bad = out.case, []
    if out.sums is not None:
        img = sums_image(case, gaps)
        lo, hi = case.span
        owner = {}
        for i, (o, k) in enumerate(zip(case.soff, case.counts)):
            owner[i] = (o, o + k)
        diff = np.flatnonzero(out.sums != img)
        for x in diff[:limit]:
            w = int(x) - CANARY_W
            who = next((i for i, (a, b) in owner.items() if a <= w < b), None)
            if who is None:
                kind = "canary before" if w < 0 else "canary after" if w >= hi else \
                    "outside the span" if w < lo else "gap word"
                bad.append("%s: sums word %d (%s) is %#x, want %#x" % (case.name, w, kind, out.sums[x], img[x]))
                continue
            p, P, L = w - case.soff[who], case.plens[who], case.lens[who]
            bad.append("%s: blob %d (L=%d P=%d) piece %d is %#x, want %#x; %s" %
                       (case.name, who, L, P, p, out.sums[x], img[x],
                        "; ".join(_where(case, windows, who, p * P, min(L, (p + 1) * P), place, ring))))
        if diff.size > limit:
            bad.append("%s: %d sums words differ in all" % (case.name, diff.size))
    if out.dig is None:
        return bad
    img = digests_image(case)
    end = CANARY_B + 32 * case.n
    diff = np.flatnonzero(out.dig != img)
    for x in diff[(diff < CANARY_B) | (diff >= end)][:limit]:
        bad.append("%s: digest byte %d (canary) is %#x" % (case.name, int(x) - CANARY_B, out.dig[x]))
    blobs = np.flatnonzero((out.dig[CANARY_B:end] != img[CANARY_B:end]).reshape(-1, 32).any(axis=1))
    for i in blobs[:limit]:
        i = int(i)
        bad.append("%s: digest of blob %d (L=%d) is %s, want %s; %s" % (
            case.name, i, case.lens[i], bytes(out.dig[CANARY_B + 32 * i:CANARY_B + 32 * i + 32]).hex()[:16],
            bytes(img[CANARY_B + 32 * i:CANARY_B + 32 * i + 32]).hex()[:16],
            "; ".join(_where(case, windows, i, 0, case.lens[i], place, ring)[-3:])))
    if blobs.size > limit:
        bad.append("%s: %d digests differ in all" % (case.name, blobs.size))
    return bad


# ------------------------------------------------------------------------------ sources
class MemSource:
    """The case's blobs in one buffer, each at src % 16 == misalign: pageable memory, or one krk_host_alloc arena."""

    def __init__(self, case, arena=False, misalign=0):
        from kraken_amd._capi import check, lib
        self.arena, self._lib = None, lib
        offs, o = [], 0
        for L in case.lens:
            offs.append(o + misalign)
            o += (misalign + L + 15) // 16 * 16 + 16
        total = o + 4096
        if arena:
            p = C.c_void_p()
            check(lib.krk_host_alloc(total, C.byref(p)))
            self.arena = p
            self.buf = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(total,))
            base = 0
        else:
            self.buf = np.empty(total + 4096, dtype=np.uint8)
            base = -self.buf.ctypes.data % 4096
        assert (self.buf.ctypes.data + base) % 16 == 0
        self.ptrs = []
        for i, L in enumerate(case.lens):
            a = base + offs[i]
            self.buf[a:a + L] = blob_bytes(case, i)
            self.ptrs.append(self.buf.ctypes.data + a if L else None)
            assert not L or self.ptrs[-1] % 16 == misalign

    def close(self):
        if self.arena is not None:
            self.buf = None
            self._lib.krk_host_free(self.arena)
            self.arena = None


class FileSource:
    """The case's blobs as files of one directory."""

    def __init__(self, case, directory):
        self.paths = []
        for i in range(case.n):
            p = os.path.join(str(directory), "w%05d" % i)
            with open(p, "wb") as f:
                f.write(memoryview(blob_bytes(case, i)))
            self.paths.append(p)

    def close(self):
        pass


# ------------------------------------------------------------------------------ calls through the C ABI
def _blobs(case, ptrs):
    from kraken_amd._capi import krk_blob
    return (krk_blob * max(case.n, 1))(*[krk_blob(ptrs[i], case.lens[i], case.plens[i], case.soff[i])
                                          for i in range(case.n)])


def _files(case, paths):
    from kraken_amd._capi import krk_file_blob
    enc = [p.encode() for p in paths]
    arr = (krk_file_blob * max(case.n, 1))(*[krk_file_blob(enc[i], case.lens[i], case.plens[i], case.soff[i])
                                              for i in range(case.n)])
    arr._keep = enc
    return arr


def call(entry, case, src):
    """One call of `entry` over the case from `src`; the Outputs it left."""
    from kraken_amd._capi import check, lib
    out = Outputs(case, crc=entry != "sha256_host", dig=not entry.startswith("piece_sums"))
    if entry == "metainfo_digest_host":
        check(lib.krk_metainfo_digest_host(_blobs(case, src.ptrs), case.n, out.sums_p, out.dig_p))
    elif entry == "sha256_host":
        ptrs = (C.c_void_p * max(case.n, 1))(*src.ptrs)
        lens = (C.c_uint64 * max(case.n, 1))(*case.lens)
        check(lib.krk_sha256_host(ptrs, lens, case.n, out.dig_p))
    elif entry == "metainfo_digest_files":
        check(lib.krk_metainfo_digest_files(_files(case, src.paths), case.n, out.sums_p, out.dig_p))
    elif entry == "piece_sums_host":
        check(lib.krk_piece_sums_host(_blobs(case, src.ptrs), case.n, out.sums_p))
    elif entry == "piece_sums_files":
        check(lib.krk_piece_sums_files(_files(case, src.paths), case.n, out.sums_p))
    else:
        raise ValueError(entry)
    return out


# What each host entry point leaves in a gap inside its sums span (include/kraken_hip.h, "Host forms"):
GAPS = {"metainfo_digest_host": "zero", "metainfo_digest_files": "zero", "piece_sums_files": "zero",
        "piece_sums_host": "keep"}


def last_call():
    from kraken_amd import device as D
    return D.windows_last_call()


def stats_mismatches(st, case, align, page_locked, registered=False, wide_gather=None, direct_reads=None, blobs=None,
                     host_blobs=0):
    """krk_windows_last_* against the replay of the blobs the call put through the windows."""
    windows, max_live = case.replay(align, blobs)
    narrow = sum(1 for w in windows if len(w) <= DIRECT_MAX)
    bad = []
    if (st["windows"], st["max_live"]) != (len(windows), max_live):
        bad.append("windows / max_live %d / %d, replay %d / %d" % (st["windows"], st["max_live"], len(windows), max_live))
    if st["direct_windows"] != (narrow if page_locked else 0):
        bad.append("direct_windows %d, want %d" % (st["direct_windows"], narrow if page_locked else 0))
    if registered:
        if not 0 <= st["gather_windows"] <= st["windows"]:
            bad.append("gather_windows %d outside [0, windows]" % st["gather_windows"])
    else:
        want = len(windows) - narrow if wide_gather else 0
        if st["gather_windows"] != want:
            bad.append("gather_windows %d, want %d" % (st["gather_windows"], want))
    if direct_reads is not None and st["direct_reads"] != direct_reads:
        bad.append("direct_reads %s, want %s" % (st["direct_reads"], direct_reads))
    if st["host_blobs"] != host_blobs:
        bad.append("host_blobs %d, want %d" % (st["host_blobs"], host_blobs))
    return [case.name + ": " + b + " (" + json.dumps({k: st[k] for k in (
        "windows", "max_live", "direct_windows", "gather_windows", "direct_reads", "host_blobs")}) + ")" for b in bad]


# ------------------------------------------------------------------------------ group C: every way up
LEGS = ("staged", "registered", "arena0", "arena1", "arena8", "arena15", "arena1_nogather", "files", "files_aio",
        "files_sync")
DIRECT_LEGS = ("files_aio", "files_sync")


def leg_align(leg):
    """The schedule's alignment on a leg: 4 KiB chunks for O_DIRECT reads, SHA-256 blocks otherwise."""
    return 4096 if leg in DIRECT_LEGS else 64


def run_leg(case, leg, directory, setenv, ring=RING, lower_cap_ok=False):
    """`case` through one way up: every entry point of that way, whole-array comparison and the call statistics.
    setenv(name, value) sets the environment for the calls (read per call).  Returns the mismatches.
    lower_cap_ok: a file batch may run under a lower live cap than KRK_LIVE_CAP (the descriptor lease caps it by the
    process's descriptor budget); the replay then takes the cap the call reports."""
    from kraken_amd._capi import check, lib
    setenv("KRK_WINDOW_MB", str(case.window_mb))
    setenv("KRK_LIVE_CAP", str(case.cap))
    align, bad = leg_align(leg), []
    place = 16 if align == 64 else align
    windows = case.replay(align)[0]
    if leg.startswith("files"):
        setenv("KRK_FILE_DIRECT", "0" if leg == "files" else "1")
        setenv("KRK_FILE_AIO", "0" if leg == "files_sync" else "1")
        src = FileSource(case, directory)
        out = call("metainfo_digest_files", case, src)
        st = last_call()
        if lower_cap_ok and st["max_live"] < min(case.cap, case.n):
            assert st["max_live"] >= 16, st
            case = Case(case.name, case.lens, case.plens, case.soff, case.window_mb, st["max_live"], case.seed)
            windows = case.replay(align)[0]
        bad += mismatches(out, "zero", windows, place, ring)
        bad += stats_mismatches(st, case, align, False, direct_reads=leg != "files")
        return [leg + ": " + b for b in bad]
    arena = leg.startswith("arena")
    misalign = int(leg[5:].split("_")[0]) if arena else 0
    mode = 1 if leg == "registered" else 0 if leg.endswith("nogather") else -1
    src = MemSource(case, arena, misalign)
    try:
        check(lib.krk_set_host_gather(mode))
        for entry in ("metainfo_digest_host", "sha256_host"):
            out = call(entry, case, src)
            st = last_call()
            bad += [entry + ": " + b for b in mismatches(out, "zero", windows, place, ring)]
            bad += [entry + ": " + b for b in stats_mismatches(
                st, case, align, arena, registered=leg == "registered", wide_gather=arena and mode != 0)]
            if leg == "registered" and st["live_registered_at_copyout"]:
                bad.append("%s: %d segments registered at the copy-out" % (entry, st["live_registered_at_copyout"]))
    finally:
        check(lib.krk_set_host_gather(-1))
        src.close()
    return [leg + ": " + b for b in bad]


# ------------------------------------------------------------------------------ groups E and F
def run_sums_host(case, fraction, arena, setenv, misalign=1):
    """krk_piece_sums_host at W = 1 MiB with the GPU's share forced: whole array, and krk_crc_host_split."""
    from kraken_amd import device as D
    setenv("KRK_WINDOW_MB", "1")
    setenv("KRK_CRC_GPU_FRACTION", str(fraction))
    q, g = gpu_share(case, fraction)
    windows = pack_replay([min(L, k * P) for L, k, P in zip(case.lens, q, case.plens)], W1, 16)
    src = MemSource(case, arena, misalign)
    try:
        out = call("piece_sums_host", case, src)
        split = D.crc_host_split()[:2]
    finally:
        src.close()
    bad = mismatches(out, GAPS["piece_sums_host"], windows, 16)
    if sum(case.lens) and split != (g, sum(case.lens) - g):
        bad.append("%s: krk_crc_host_split %r, the share %s implies %r" % (case.name, split, fraction,
                                                                           (g, sum(case.lens) - g)))
    return bad


def run_sums_files(case, directory, direct, setenv):
    """krk_piece_sums_files at W = 1 MiB on the session's placement (KRK_PLACE_GPU)."""
    from kraken_amd import device as D
    setenv("KRK_WINDOW_MB", "1")
    setenv("KRK_FILE_DIRECT", "1" if direct else "0")
    out = call("piece_sums_files", case, FileSource(case, directory))
    bad = mismatches(out, GAPS["piece_sums_files"], pack_replay(case.lens, W1, 4096), 4096)
    if sum(case.lens) and D.crc_host_split()[:2] != (sum(case.lens), 0):
        bad.append("%s: krk_crc_host_split %r, want every byte on the GPU" % (case.name, D.crc_host_split()[:2]))
    return bad


def run_entries(case, directory, setenv, page_locked_if_empty=False):
    """Every host entry point over one small case (group E): pageable memory staged, buffered files, and the CRC-only
    calls with the whole batch on the GPU; each array against the image its gap rule (GAPS) gives."""
    setenv("KRK_WINDOW_MB", str(case.window_mb))
    setenv("KRK_LIVE_CAP", str(case.cap))
    setenv("KRK_FILE_DIRECT", "0")
    windows, bad = case.replay()[0], []
    mem, files = MemSource(case), FileSource(case, directory)
    for entry in ("metainfo_digest_host", "sha256_host", "metainfo_digest_files"):
        out = call(entry, case, files if entry.endswith("files") else mem)
        st = last_call()
        bad += [entry + ": " + b for b in mismatches(out, GAPS.get(entry, "zero"), windows)]
        # a batch of empty blobs has no pageable byte: its windows count as page-locked
        locked = page_locked_if_empty and not entry.endswith("files")
        bad += [entry + ": " + b for b in stats_mismatches(
            st, case, 64, locked, direct_reads=False if entry.endswith("files") else None)]
    bad += ["piece_sums_host: " + b for b in run_sums_host(case, 1, True, setenv)]
    bad += ["piece_sums_files: " + b for b in run_sums_files(case, directory, False, setenv)]
    return bad


def run_mixed(case, directory, setenv):
    """case_e_mixed with four host threads under e_rates: the host takes E_HOST (asserted through the planner before
    each call and through host_blobs after), the windows run over the rest, both sides' results meet in one array."""
    from kraken_amd import device as D
    setenv("KRK_WINDOW_MB", str(case.window_mb))
    setenv("KRK_LIVE_CAP", str(case.cap))
    setenv("KRK_FILE_DIRECT", "0")
    rest = [i for i in range(case.n) if i not in E_HOST]
    windows, bad = case.replay(64, rest)[0], []
    mem, files = MemSource(case), FileSource(case, directory)
    D.set_sha_host_offload(4)
    D.set_planner_rates(e_rates(D.planner_rates()))
    try:
        for entry, mode in (("metainfo_digest_host", D.OFFLOAD_HOST_WHOLE), ("sha256_host", D.OFFLOAD_HOST_SHA),
                            ("metainfo_digest_files", D.OFFLOAD_HOST_FILES)):
            plan = sorted(D.sha_offload_plan(case.lens, 4, mode=mode)[0].tolist())
            if plan != list(E_HOST):
                bad.append("%s: the planner gives the host %r, not %r" % (entry, plan, E_HOST))
                continue
            out = call(entry, case, files if entry.endswith("files") else mem)
            bad += [entry + ": " + b for b in mismatches(out, "zero", windows)]
            bad += [entry + ": " + b for b in stats_mismatches(
                last_call(), case, 64, False, blobs=rest, host_blobs=len(E_HOST),
                direct_reads=False if entry.endswith("files") else None)]
    finally:
        D.set_sha_host_offload(0)
        D.set_planner_rates(None)
    return bad


def main(argv):
    """python -m tests.window_matrix LEG [LEG ...]: group A through the legs in this process (the ring depth is
    fixed per process: KRK_STAGING_WINDOWS), one JSON line a leg; exit status 1 on a mismatch."""
    from kraken_amd import device as D
    from kraken_amd._capi import check, lib
    D.set_device(0)
    check(lib.krk_set_sha_host_offload(0))
    ring = min(4, max(2, int(os.environ.get("KRK_STAGING_WINDOWS", RING))))
    status = 0
    for leg in argv:
        with tempfile.TemporaryDirectory() as d:
            t0 = time.perf_counter()
            bad = run_leg(case_a(leg_align(leg)), leg, d, os.environ.__setitem__, ring)
            print(json.dumps({"leg": leg, "ring": ring, "seconds": round(time.perf_counter() - t0, 3),
                              "n_mismatches": len(bad), "mismatches": bad[:8]}), flush=True)
            status |= bool(bad)
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
