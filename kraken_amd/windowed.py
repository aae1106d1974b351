"""Larger-than-HBM batches (config C3: 20k blobs of 100 MiB-1 GiB, ~1.47 TB per GPU
against 288 GB of HBM): every live blob advances by one chunk per device window
through krk_metainfo_digest_chunks_dev -- SHA-256 from per-blob midstates in HBM,
piece CRCs XOR-accumulated by byte range -- while the next window is generated
(synthetic data) on its own stream.

This is the machinery bench.py's C3 line runs and tests/test_gpu_windowed.py checks
against the oracle and the one-shot path.
"""
from __future__ import annotations

import ctypes as C
import threading
import time

import numpy as np

from ._capi import check, lib

GAMMA = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
LAUNCH_S = 0.0005  # a window's modelled launch overhead


def mix64(z: int) -> int:
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def c3_lengths(n_total=20000, scale: int = 1):
    """L_i = 104,857,600 + (rng_i mod 968,884,225), rng_i = mix64(0xC3 + i*gamma)
    (SURVEY.md 8(d) C3); `scale` > 1 divides every length (same law, smaller bytes)."""
    return [(104_857_600 + mix64((0xC3 + i * GAMMA) & M64) % 968_884_225) // scale for i in range(n_total)]


class _Sched:
    """The library's window schedule (krk_window_sched_*, kraken_amd/csrc/windows.cpp; the same
    one its host-resident batch calls run) over a subset of the batch: `idx` are indices into
    the full batch, and so are the blobs of the windows next() returns."""

    def __init__(self, lens, idx, W, cap, max_chunk=0):
        self.idx = np.asarray(idx, dtype=np.int64)
        L = np.ascontiguousarray(np.asarray(lens, dtype=np.uint64)[self.idx])
        self.cap = max(1, min(int(cap), max(1, L.size)))
        self.h = C.c_void_p()
        if L.size:
            check(lib.krk_window_sched_new(L.ctypes.data_as(C.POINTER(C.c_uint64)), L.size, int(W), self.cap,
                                           C.byref(self.h)))
            if max_chunk:
                check(lib.krk_window_sched_set_chunk_cap(self.h, int(max_chunk)))
        self.sub = {int(b): k for k, b in enumerate(self.idx)}
        self._b = np.zeros(self.cap, dtype=np.uint32)
        self._o = np.zeros(self.cap, dtype=np.uint64)
        self._t = np.zeros(self.cap, dtype=np.uint64)

    def next(self):
        """The next window (blob indices, offsets, chunk lengths), None after the last."""
        if not self.h.value:
            return None
        k = C.c_uint64(0)
        check(lib.krk_window_sched_next(self.h, self._b.ctypes.data_as(C.POINTER(C.c_uint32)),
                                        self._o.ctypes.data_as(C.POINTER(C.c_uint64)),
                                        self._t.ctypes.data_as(C.POINTER(C.c_uint64)), self.cap, C.byref(k)))
        m = k.value
        if not m:
            return None
        return self.idx[self._b[:m].astype(np.int64)], self._o[:m].copy(), self._t[:m].copy()

    def drop(self, b):
        """Blob b leaves the schedule; returns the bytes of it the windows have queued."""
        off = C.c_uint64(0)
        check(lib.krk_window_sched_drop(self.h, self.sub[int(b)], C.byref(off)))
        return off.value

    def close(self):
        if self.h.value:
            lib.krk_window_sched_free(self.h)
            self.h = C.c_void_p()


def window_plan(lens, W, cap):
    """Windows: [(blob indices, offsets, chunk lengths)] -- the library's window schedule,
    drained.  Every live blob advances by the same 64-multiple chunk per window (about W
    bytes a window).  Admission: at most `cap` blobs are live, admitted longest first, so the
    longest chain starts in window 0 and every window stays on a multi-lane SHA plan (eight
    lanes a stream up to 16 x CUs live streams, two up to 64 x CUs; a launch of more streams
    falls back to one lane per stream, ~0.7x per stream); a finished blob's
    slot goes to the next-longest waiting blob."""
    sched = _Sched(lens, np.arange(len(lens)), W, cap)
    try:
        wins = []
        win = sched.next()
        while win is not None:
            wins.append(win)
            win = sched.next()
        return wins
    finally:
        sched.close()


def two_lane_stream_cap(D, n):
    """Largest stream count <= n whose SHA launch plan runs a stream on more than one
    lane (eight or two lanes per stream; the one-lane plan's chain is the slowest)."""
    if n == 0 or D.sha_lanes_per_stream(n) >= 2:
        return max(n, 1)
    lo, hi = 1, n  # several lanes at lo, one at hi
    if D.sha_lanes_per_stream(lo) < 2:
        return n
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if D.sha_lanes_per_stream(mid) >= 2 else (lo, mid)
    return lo


def window_stream_cap(D, n):
    """Live streams per window: at most 7/8 of the largest multi-lane stream count (a
    multiple of the two-pair workgroup's 64; krk_window_stream_cap, the cap the library's
    host-resident windows use too).  At the full two-lane count (64 x CUs) every CU holds a
    128 KiB SHA workgroup and the window's piece-CRC launch (144 KiB workgroups) waits for
    the SHA launch to end; with an eighth of the CUs left free it runs inside it, and the
    chain of the longest blob -- not the live count -- still sets the run time.  C3 on one
    MI355X (bench --live-cap): 16,384 live 494 GB/s, 15,360 522, 14,336 524, 13,824 523,
    13,312 522, 12,288 509 (profiles/r02/c3_live_cap.jsonl)."""
    v = C.c_uint64(0)
    D.check(D.lib.krk_window_stream_cap(C.byref(v)))
    return max(1, min(n, v.value))


def stream_rate(rates, n_streams):
    """One SHA-256 stream's rate (B/s) in a launch of n_streams: the planner rate of the
    AUTO tier the launch falls in (eight lanes up to 16 x CUs streams, two lanes up to
    64 x CUs, one lane beyond; krk_planner_rates)."""
    cus = max(1, int(rates["cus"]))
    return rates["sha_stream_bps"][0 if n_streams <= 16 * cus else 1 if n_streams <= 64 * cus else 2]


def window_seconds(rates, take, live, launch_s=LAUNCH_S):
    """Modelled seconds of one window of `live` streams with chunk lengths `take`: its largest
    chunk at the per-stream rate of its launch plan (the chain of the window's longest chunk
    sets it), plus a launch overhead."""
    return float(take.max()) / stream_rate(rates, live) + launch_s


def windows_seconds(rates, lens, W, cap, launch_s=LAUNCH_S):
    """Modelled run time of the windows over `lens`: the sum of window_seconds."""
    t = 0.0
    for blobs, _, take in window_plan(lens, W, cap):
        t += window_seconds(rates, take, blobs.size, launch_s)
    return t


def host_lane_plan(D, lens, W, cap, threads, rates=None, min_gain=0.02):
    """How many of the longest blobs the host lane takes: K (a multiple of `threads`, the
    lane hashes one group of `threads` blobs at a time) minimising max(GPU windows over the
    rest, host groups), from the planner rates (krk_planner_rates: per-stream rates
    measured on the device, one host thread's SHA-256 rate, the D2H rate shared by the
    threads).  0 unless it shortens the modelled run by min_gain.  Returns (K, modelled
    seconds with it, modelled seconds without)."""
    rates = rates or D.planner_rates()
    T = max(1, int(threads))
    L = np.asarray(lens, dtype=np.int64)
    order = np.argsort(-L, kind="stable")
    per_thread = min(rates["host_sha_bps"], rates["d2h_bps"] / T)

    def cost(m):  # m groups of T on the host
        k = min(m * T, L.size)
        host = sum(float(L[order[g * T]]) / per_thread for g in range(m))  # a group lasts its longest blob
        rest = L[order[k:]]
        gpu = windows_seconds(rates, rest, W, min(cap, max(1, rest.size))) if rest.size else 0.0
        return max(gpu, host), k

    base, _ = cost(0)
    lo, hi = 0, (L.size + T - 1) // T
    while hi - lo > 2:  # max(decreasing, increasing): ternary search on the group count
        m1, m2 = lo + (hi - lo) // 3, hi - (hi - lo) // 3
        if cost(m1)[0] <= cost(m2)[0]:
            hi = m2
        else:
            lo = m1
    best, k = min(cost(m) for m in range(lo, hi + 1))
    if best > base * (1 - min_gain):
        return 0, base, base
    return k, best, base


def lane_groups(lens, k, threads):
    """The host lane's blobs: the K longest (sorted indices) and the groups of `threads`
    of them it hashes one after the other, longest first.  The last group stops at K (it
    once ran on into the window blobs, hashing them too and zeroing the piece sums the
    windows had accumulated for them)."""
    L = np.asarray(lens, dtype=np.int64)
    k = int(min(max(k, 0), L.size))
    T = max(1, int(threads))
    order = np.argsort(-L, kind="stable")
    blobs = np.sort(order[:k]) if k else np.zeros(0, dtype=np.int64)
    return blobs, [order[g:min(g + T, k)] for g in range(0, k, T)]


def _new_stream(D, prio=None):
    s = C.c_void_p()
    if prio is None:
        D.check(D.lib.krk_stream_create(C.byref(s)))
    else:
        D.check(D.lib.krk_stream_create_prio(int(prio), C.byref(s)))
    return s


def _new_event(D, polling=False):
    e = C.c_void_p()
    D.check((D.lib.krk_event_create_polling if polling else D.lib.krk_event_create)(C.byref(e)))
    return e


def _event_done(D, ev):
    done = C.c_int(0)
    D.check(D.lib.krk_event_query(ev, C.byref(done)))
    return bool(done.value)


def _pack(base_ptr, lengths, align):
    """Device addresses of spans of `lengths` bytes packed from base_ptr (itself aligned) on,
    each at a multiple of `align`."""
    a = np.uint64(align)
    dev = np.zeros(len(lengths), dtype=np.uint64)
    dev[1:] = np.cumsum((np.asarray(lengths, dtype=np.uint64) + (a - np.uint64(1))) // a * a)[:-1]
    return dev + np.uint64(base_ptr)


def _write_digests(D, cb, dig, blobs):
    """Host-computed digests (rows of `dig`) into the batch's device digest rows."""
    for b in blobs:
        row = np.ascontiguousarray(dig[b])
        D.check(D.lib.krk_memcpy_h2d(C.c_void_p(cb.digests.ptr + 32 * int(b)), row.ctypes.data_as(C.c_void_p), 32))


class _DeviceWindows:
    """What the two runners share: the batch's blob ids, two device windows (`bufs`) filled by
    the generator on `gen_s`, and the streams and events the runner created."""

    def __init__(self, D, ids):
        self.D = D
        self.ids = np.asarray(ids, dtype=np.uint64)
        self._streams, self._events = [], []

    def _stream(self, prio=None):
        self._streams.append(_new_stream(self.D, prio))
        return self._streams[-1]

    def _event(self, polling=False):
        self._events.append(_new_event(self.D, polling))
        return self._events[-1]

    def _items(self, win, k):
        """Window k's chunks at 16-byte aligned addresses in buffer k & 1."""
        blobs, offs, take = win
        return blobs, _pack(self.bufs[k & 1].ptr, take, 16), offs, take

    def _gen(self, items):
        """Queue the generation of a window's bytes on gen_s (the caller waits its own way)."""
        blobs, dev, offs, take = items
        self.D.synth_fill_chunk_arrays(self.ids[blobs], dev, offs, take, stream=self.gen_s)

    def _close(self, bufs):
        """Every stream synced (nothing in flight), then the buffers freed, the events
        destroyed, the streams destroyed."""
        lib = self.D.lib
        for s in self._streams:
            lib.krk_stream_sync(s)
        for b in bufs:
            b.free()
        for e in self._events:
            lib.krk_event_destroy(e)
        for s in self._streams:
            lib.krk_stream_destroy(s)
        self._events, self._streams = [], []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WindowedRun(_DeviceWindows):
    """One batch of synthetic blobs (ids, lens, piece length P) streamed through two
    device windows of W bytes: window k+1 is generated on `gen` while window k's
    kernels run on `run`.  After run(): cb.sums / cb.digests hold every blob's piece
    sums and digest (device).

    host_lane=(K, threads): the K longest blobs skip the windows; a host-lane thread
    generates them `threads` at a time into a device buffer of their own, queues their
    piece CRCs on the GPU (krk_piece_sums_dev, into cb.sums) and hashes them on `threads`
    host threads (krk_sha256_dev_on_host: each reads a blob out of HBM through pinned
    double buffers), while the windows run the rest; their digests go into cb.digests at
    the end of run()."""

    def __init__(self, D, ids, lens, P, W, cap=None, host_lane=None, device=0, sha_priority=None):
        super().__init__(D, ids)
        self.lens = list(lens)
        self.P = P
        self.W = int(W)
        self.device = device
        n = len(self.lens)
        L = np.asarray(self.lens, dtype=np.int64)
        k, self.lane_threads = (host_lane or (0, 0))
        self.lane_blobs, self.lane_groups = lane_groups(L, k, self.lane_threads)
        gpu = np.setdiff1d(np.arange(n), self.lane_blobs) if k else np.arange(n)
        self.cap = window_stream_cap(D, gpu.size) if cap is None else int(cap)
        self.wins = [(gpu[b], o, t) for b, o, t in window_plan(L[gpu], self.W, self.cap)]
        wb = self.W + 16 * max(gpu.size, 1)
        self.bufs = [D.DeviceBuffer(wb), D.DeviceBuffer(wb)] if self.wins else []
        self.lane_bufs = []
        if k:  # two buffers of a group each (the first group holds the longest blobs)
            nb = (int(L.max()) + 256) * len(self.lane_groups[0])
            self.lane_bufs = [D.DeviceBuffer(nb) for _ in range(min(2, len(self.lane_groups)))]
        self.lane_digests = None
        self.lane_seconds = 0.0
        self.cb = D.ChunkedBatch(self.lens, P)
        self.run_s = self._stream()
        self.gen_s = self._stream()
        # With the host lane, the windows' SHA-256 launches (up to ~0.6 s each) go on a
        # high-priority stream, i.e. hardware queues of their own: normal-priority streams
        # share GPU_MAX_HW_QUEUES queues, and the lane's D2H copies and generator / CRC
        # launches queued on a stream sharing the SHA launch's queue wait behind it.  Rank
        # 0's shard of an 8-GPU C3 (tools/lane_probe.py, 480 blobs on 15 threads): lane 24.3
        # s on the shared queues, 15.75 s with the SHA launches apart.  Without the lane they
        # stay on the library's stream (a C3 N=1 run measured 553 GB/s there, 499 with its
        # SHA launches at high priority).
        if sha_priority is None:
            sha_priority = -1 if k else 0
        self.sha_s = self._stream(sha_priority) if sha_priority else None
        self.lane_ss = [self._stream() for _ in self.lane_bufs]

    def _gen_window(self, k):
        items = self._items(self.wins[k], k)
        self._gen(items)
        self.D.check(self.D.lib.krk_stream_sync(self.gen_s))
        return items

    def _lane(self, err):
        """The host lane's thread: group by group (longest first), generate the group's
        blobs into one of two lane buffers and queue their piece CRCs on that buffer's
        stream, then hash the previous group on the host threads -- group g+1 is
        generated and CRC'd on the device while group g is hashed."""
        D = self.D
        try:
            t0 = time.perf_counter()
            D.set_device(self.device)
            dig = np.zeros((len(self.lens), 32), dtype=np.uint8)
            L = np.asarray(self.lens, dtype=np.uint64)

            def place(g, b):
                ln = L[g]
                dev = _pack(self.lane_bufs[b].ptr, ln, 256)
                s = self.lane_ss[b]
                D.synth_fill_chunk_arrays(self.ids[g], dev, np.zeros(g.size, np.uint64), ln, stream=s)
                for j in range(g.size):  # one call a blob: a call zeroes the whole sums span it covers
                    D.piece_sums_dev_arrays(dev[j:j + 1], ln[j:j + 1], self.cb.piece_lengths[g[j:j + 1]],
                                            self.cb.sums_off[g[j:j + 1]], self.cb.sums.ptr, stream=s)
                return dev, ln

            groups = self.lane_groups
            cur = place(groups[0], 0)
            for k, g in enumerate(groups):
                # buffer (k+1)&1 last held group k-1: hashed (the call below is synchronous)
                # and CRC'd (same stream, earlier) before the next fill is queued behind them
                nxt = place(groups[k + 1], (k + 1) & 1) if k + 1 < len(groups) else None
                dig[g] = D.sha256_dev_on_host(cur[0], cur[1], self.lane_threads, stream=self.lane_ss[k & 1])
                cur = nxt
            for s in self.lane_ss:  # the last groups' CRCs
                D.check(D.lib.krk_stream_sync(s))
            self.lane_digests = dig
            self.lane_seconds = time.perf_counter() - t0
        except BaseException as e:  # re-raised on the caller's thread
            err.append(e)

    def run(self):
        """Window k's kernels are queued before the host waits for window k-1's (an
        event after each window), so the device goes from one window to the next with
        no host round trip; window k+1 is generated into k-1's buffer once k-1 is done.
        The host lane (if any) runs on its own thread meanwhile."""
        lane, err = None, []
        if self.lane_groups:
            lane = threading.Thread(target=self._lane, args=(err,), name="krk-host-lane")
            lane.start()
        try:
            if self.wins:
                self._run_windows()
        finally:
            if lane is not None:
                lane.join()
        if err:
            raise err[0]
        if lane is not None:
            _write_digests(self.D, self.cb, self.lane_digests, self.lane_blobs)

    def _run_windows(self):
        D = self.D
        cur = self._gen_window(0)
        evs = [_new_event(D), _new_event(D)]  # window k's kernels done: evs[k & 1]
        try:
            for k in range(len(self.wins)):
                self.cb.step_arrays(*cur, stream=self.run_s, sha_stream=self.sha_s)
                D.check(D.lib.krk_event_record(evs[k & 1], self.run_s))
                if k + 1 < len(self.wins):
                    if k:  # window k-1 read buffer (k+1) & 1
                        D.check(D.lib.krk_event_sync(evs[(k - 1) & 1]))
                    cur = self._gen_window(k + 1)
            D.check(D.lib.krk_stream_sync(self.run_s))
        finally:
            for e in evs:
                D.lib.krk_event_destroy(e)

    def close(self):
        self._close(self.bufs + self.lane_bufs)
        self.bufs, self.lane_bufs = [], []


# ---------------------------------------------------------------------------------------
# Tail handoff of the windowed chains.  A windowed batch whose longest
# chain outlasts the GPU's aggregate work -- every shard of an 8-GPU C3, whose 1.07 GB blob
# takes ~18 s at ~58 MB/s a stream while the shard's 1.47 TB would take ~2 s -- ends when
# that chain ends.  Host threads (SHA-NI, ~2.3 GB/s, 40x a GPU stream) steal chains instead:
# at each window boundary every thread that will be free before the next window ends takes
# the chain with the most bytes left (earliest deadline first, as planner_math.hpp tail_plan does
# for batches in HBM), from the midstate the windows keep in HBM (ChunkedBatch.state); the
# chain leaves the window schedule (krk_window_sched_drop), its remaining bytes are
# generated on the device in 64 MiB pieces, their piece CRCs run on the GPU
# (krk_chunks_crc_dev, XOR-accumulated into the same sums), and the thread hashes them out
# of HBM (krk_sha256_resume_dev_on_host).  The threads start on the longest chains whole.
# The same policy is simulated on the planner's rates (simulate_tail_handoff): the bench
# reports that model beside the measured run.

_IV = np.array([0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19],
               dtype=np.uint32)
TAIL_PIECE = 64 << 20  # device bytes a tail thread generates, CRCs and hashes at a time
# Window chunk cap of the tail handoff: ~70 ms of a chain at eight lanes a window, so a
# chain is handed over within a short window of a thread becoming free, however few chains
# are left live (modelled on rank 0's shard of an 8-GPU C3: 1/2/4/8 MiB end at 11.7 / 11.7
# / 12.0 / 12.7 s with 0.5 ms a launch, 12.7 / 12.2 / 12.3 / 12.9 s with 3 ms).
TAIL_CHUNK = 4 << 20
# A thread gets its next chain while it is expected to be free within this many windows
# after the queued one ends: a chain handed over early idles on the GPU side (r/h ~ 2.4 % of
# the idle time in extra host bytes), a thread that finishes before the window holding its
# next chain's midstate ends waits for it (all of that time lost).
TAIL_HORIZON = 2.5
TAIL_RING = 8  # device slots a tail thread's pieces cycle through (generated / hashed / waiting for their CRC)
TAIL_FIRST_PIECE = 8 << 20  # a stolen chain's first piece (a multiple of 64)


def tail_thread_rate(rates, threads):
    """One tail thread's bytes/s: its SHA-NI rate (the planner's figure is derated 15 % for a
    loaded socket; a tail thread alone on its buffers loses ~2 %, planner_math.hpp tail_plan),
    capped by its share of the device-to-host copy rate."""
    return min(rates["host_sha_bps"] * (0.98 / 0.85), rates["d2h_bps"] / max(1, int(threads)))


def chain_pieces(y, L, piece):
    """A chain's bytes [y, L) as the (offset, bytes) pieces its thread hashes: a short first
    one (the thread starts hashing after one short copy, not behind a burst of whole-piece
    copies at a window boundary), then whole pieces; one empty piece when y == L."""
    out, o = [], y
    while True:
        m = min(TAIL_FIRST_PIECE if o == y else piece, piece, L - o)
        out.append((o, m))
        o += m
        if o >= L:
            return out


class TailPolicy:
    """Which chains the host threads take, and when (shared by the run and its model).
    A chain is a candidate while it has more bytes left than the window after the queued one
    would give it; candidates go longest-remaining first.  Waiting (not yet admitted) blobs
    are candidates too, with all their bytes left."""

    def __init__(self, lens, threads):
        self.L = np.asarray(lens, dtype=np.int64)
        self.H = max(1, int(threads))
        self.pos = np.zeros(self.L.size, dtype=np.int64)  # bytes the windows queued so far
        self.on_gpu = np.ones(self.L.size, dtype=bool)    # not (yet) taken by a host thread

    def initial(self):
        """The chains the threads take whole before the first window (the H longest)."""
        k = min(self.H, self.L.size)
        first = np.argsort(-self.L, kind="stable")[:k]
        self.on_gpu[first] = False
        return [int(b) for b in first]

    def queued(self, blobs, offs, takes):
        self.pos[blobs] = (offs + takes).astype(np.int64)

    def pick(self, n, min_left):
        """Up to n chains for threads about to be free, most bytes left first; min_left: a
        chain the next window would finish anyway stays on the GPU."""
        if n <= 0:
            return []
        left = np.where(self.on_gpu, self.L - self.pos, -1)
        if n < left.size:
            cand = np.argpartition(-left, n)[:n]
        else:
            cand = np.arange(left.size)
        cand = cand[np.argsort(-left[cand], kind="stable")]
        out = [int(b) for b in cand if left[b] > min_left]
        self.on_gpu[out] = False
        return out

    def handover(self, sched, free_at, horizon, min_left, may_take=None):
        """The chains that change hands at a window boundary.  free_at[i]: when thread i is
        expected to be free (the caller's estimate); every thread free by `horizon` (and, if
        given, with may_take[i]) takes a chain, the earliest-free thread the one with the most
        bytes left (pick), and the chain leaves the window schedule.  Returns [(thread, chain,
        bytes of the chain the windows have queued)]."""
        ready = [i for i, t in enumerate(free_at) if t <= horizon and (may_take is None or may_take[i])]
        ready.sort(key=lambda i: free_at[i])
        return [(i, b, sched.drop(b)) for i, b in zip(ready, self.pick(len(ready), min_left))]


def simulate_tail_handoff(lens, W, cap, threads, rates, launch_s=LAUNCH_S, max_chunk=0):
    """The tail handoff on the planner's rates, window by window, with the policy the run uses:
    window k lasts its largest chunk over the per-stream rate of its live count's tier plus a
    launch; at the start of window k (the end of k-1) every thread free within TAIL_HORIZON
    windows after window k takes a chain, whose midstate is ready when window k ends.  Returns the
    modelled end (s), the GPU windows' end, the host bytes and the takeovers."""
    L = np.asarray(lens, dtype=np.int64)
    H = max(0, int(threads))  # 0: the windows alone (the GPU-only model)
    h = tail_thread_rate(rates, max(H, 1))
    pol = TailPolicy(L, max(H, 1))
    first = pol.initial() if H else []
    if not H:
        pol.on_gpu[:] = True
    free = [float(L[b]) / h for b in first] + [0.0] * (H - len(first))
    host_bytes = int(L[first].sum()) if H else 0
    takes = 0
    sched = _Sched(L, np.nonzero(pol.on_gpu)[0], W, cap, max_chunk)
    t = 0.0  # end of the previous window = start of this one
    try:
        win = sched.next()
        while win is not None:
            blobs, offs, tk = win
            pol.queued(blobs, offs, tk)
            dur = window_seconds(rates, tk, blobs.size, launch_s)
            end_k = t + dur
            horizon = end_k + TAIL_HORIZON * dur  # later windows modelled like k
            for i, b, y in pol.handover(sched, free, horizon, stream_rate(rates, blobs.size) * dur):
                start = max(free[i], end_k if y else free[i])
                free[i] = start + float(L[b] - y) / h
                host_bytes += int(L[b] - y)
                takes += 1
            t = end_k
            win = sched.next()
    finally:
        sched.close()
    return {"end_s": max([t] + free), "gpu_end_s": t, "host_bytes": host_bytes, "takeovers": takes + len(first),
            "thread_rate_Bps": h}


def _wait_summary(ws):
    """The tail threads' midstate waits: how many, how many found the window already done,
    wait and assignment-to-start percentiles (ms)."""
    if not ws:
        return {"n": 0}
    w = np.array([x[0] for x in ws]) * 1e3
    a = np.array([x[2] for x in ws]) * 1e3
    return {"n": len(ws), "window_already_done": int(sum(x[1] for x in ws)), "over_5ms": int((w > 5).sum()),
            "wait_ms_p50_p90_max": [round(float(np.percentile(w, q)), 2) for q in (50, 90, 100)],
            "since_assigned_ms_p10_p50_p90": [round(float(np.percentile(a, q)), 1) for q in (10, 50, 90)]}


_CRC_UNQUEUED = object()  # a ring slot whose piece's CRC has not been flushed to the device yet


class _Rings:
    """The tail threads' rings of device slots, as bookkeeping: thread i's pieces go through
    its slots in order, and a slot is free again once its thread has hashed the piece (copied
    down) AND the piece's CRC has been queued and its event is done.  No device call and no
    lock of its own: every method is called with the run's lock held."""

    def __init__(self, threads, slots):
        self.slots = slots
        self.to_gen = [[] for _ in range(threads)]  # pieces still to generate, in order: (blob, offset, bytes,
        #                                             leading bytes a window has already summed)
        self.ready = [[] for _ in range(threads)]   # generated pieces a thread may hash, in order: (slot, blob,
        #                                             offset, bytes)
        self.slot_used = [[False] * slots for _ in range(threads)]
        self.slot_crc = [[None] * slots for _ in range(threads)]  # the event after the slot's last CRC
        self.next_slot = [0] * threads
        self.pending = []  # generated pieces whose CRC is not queued yet

    def claim(self, crc_done):
        """Every free slot to its thread's next piece: [(thread, slot, blob, offset, bytes,
        summed bytes)], the slots now in use.  crc_done(event): has that event completed."""
        gen = []
        for i, todo in enumerate(self.to_gen):
            while todo:
                k = self.next_slot[i]
                if self.slot_used[i][k]:
                    break
                ev = self.slot_crc[i][k]
                if ev is _CRC_UNQUEUED:  # its piece's CRC is not even queued yet
                    break
                if ev is not None:
                    if not crc_done(ev):
                        break
                    self.slot_crc[i][k] = None
                b, o, m, c0 = todo.pop(0)
                self.slot_used[i][k] = True
                self.slot_crc[i][k] = _CRC_UNQUEUED if m > c0 else None  # until release()
                self.next_slot[i] = (k + 1) % self.slots
                gen.append((i, k, b, o, m, c0))
        return gen

    def publish(self, gen):
        """Claimed pieces, now generated: to their threads, and their CRCs (of the bytes no
        window has summed) to the next flush."""
        for i, k, b, o, m, c0 in gen:
            self.ready[i].append((k, b, o, m))
            if m > c0:
                self.pending.append((i, k, b, o + c0, m - c0, c0))

    def take_pending(self):
        take, self.pending = self.pending, []
        return take

    def release(self, take, ev):
        """The CRCs of `take` are queued, `ev` recorded behind them: their slots wait for it."""
        for t in take:
            self.slot_crc[t[0]][t[1]] = ev


class _TailState:
    """One TailHandoffRun.run()'s mutable state.  `cv` is the run's only lock: the rings and
    the per-thread lists below are read and written under it by the loop and the threads
    (but a thread's own phase times, which only it writes); the rest is the loop's alone."""

    def __init__(self, threads, slots, n):
        H = threads
        self.cv = threading.Condition(threading.Lock())
        self.rings = _Rings(H, slots)
        self.jobs = [[] for _ in range(H)]  # a thread's chains: (blob, from byte, window of its midstate, midstate)
        self.left = [0] * H                 # bytes of them it has not hashed yet
        self.t_last = [0.0] * H
        self.busy_s = [0.0] * H
        self.done_bytes = [0] * H
        self.phase = [{"midstate": 0.0, "device": 0.0, "hash": 0.0, "copy_wait": 0.0} for _ in range(H)]
        self.mwaits = [[] for _ in range(H)]  # (wait s, event already done, s since assignment)
        self.t_assigned = {}
        self.done = self.abort = False
        self.win_done = -1  # the last window the loop has seen end
        self.alive = H
        self.err = []
        self.dig = np.zeros((n, 32), dtype=np.uint8)  # the threads' digests, by blob
        # the loop's own
        self.events = []  # every event of this run, the windows' (wev) among them
        self.wev = []
        self.host_blobs = set()
        self.host_bytes = self.takes = self.resumed = self.early = self.tail_pieces = 0
        self.gen_wait = [0.0, 0.0]  # the loop's seconds generating: tail pieces, windows
        self.wait_win_s = self.gpu_end = 0.0
        self.scale = 1.0  # measured / modelled window time (EMA)
        self.t_prev_end, self.last_model = 0.0, 1.0


class TailHandoffRun(_DeviceWindows):
    """A windowed batch (the WindowedRun layout: synthetic blobs generated window by window on
    the device, two device windows, one ChunkedBatch) with the tail handoff: `threads` host
    threads steal chains at window boundaries (TailPolicy).  After run(): cb.sums / cb.digests
    hold every blob's piece sums and digest (device); `stats` the run's takeovers and timing.

    Who does what.  The window loop (the calling thread) owns every device call: the
    windows, and the stolen chains' remaining bytes, generated piece by piece (64 MiB) into
    each thread's ring of device slots on the window generator's stream as slots come free
    and copied down, whole, on one copy stream into a pinned twin of the slot; the pieces'
    CRCs are queued into the window stream after each window's step; each window's midstates
    are mirrored to host memory.  The host threads only wait for their pieces' copies and hash
    them (krk_sha256_resume_host), in order, from the chain's midstate.  Queues: a packet that
    cannot start blocks every later packet of its hardware queue, and normal-priority streams
    share four of them (GPU_MAX_HW_QUEUES; 16 or 32 measured slower, profiles/r06): so the
    windows' step and SHA-256 streams are high priority, the CRC launches (144 KiB-LDS
    workgroups, which wait for CUs the window's SHA workgroups leave room on) go only there,
    and the normal queues carry the copies and the generator's launches (no LDS, never
    blocked, waited for by the host)."""

    def __init__(self, D, ids, lens, P, W, threads, cap=None, device=0, max_chunk=TAIL_CHUNK, piece=TAIL_PIECE,
                 ring=TAIL_RING, crc_after_sha=None, from_previous="auto"):
        super().__init__(D, ids)
        self.lens = np.asarray(lens, dtype=np.int64)
        self.P = P
        self.W = int(W)
        self.H = max(1, int(threads))
        self.device = device
        self.max_chunk = int(max_chunk)
        self.piece = int(piece)  # a multiple of 64
        assert self.piece > 0 and self.piece % 64 == 0, piece
        n = self.lens.size
        self.cap = window_stream_cap(D, n) if cap is None else int(cap)
        self.rates = D.planner_rates()
        self.h = tail_thread_rate(self.rates, self.H)
        wb = self.W + 16 * max(min(self.cap, n), 1)
        self.bufs = [D.DeviceBuffer(wb), D.DeviceBuffer(wb)]
        self.cb = D.ChunkedBatch(self.lens, P)
        self.ring = max(2, int(ring))
        self.tbuf = [[D.DeviceBuffer(self.piece) for _ in range(self.ring)] for _ in range(self.H)]
        self.run_s = self._stream(-1)
        self.gen_s = self._stream()
        self.sha_s = self._stream(-1)
        # every window's midstates, copied down after its step on the window stream (window k
        # into mirror k & 1): a stolen chain's midstate is read there once the window is done
        # (a synchronous copy would queue behind other streams' packets in a shared hardware
        # queue)
        self.state_host = [D.PinnedArray((n, 8), np.uint32, dma_target=True) for _ in range(2)]
        # a window's CRC after its SHA launch, or beside it when the windows are full (every
        # stream the cap allows live: throughput-bound windows, where a serialised CRC costs
        # ~13 %; measured beside / after: 1 GPU 537 / 503, 2 GPUs 615 / 586-613, 4 GPUs
        # 720-740 / 746-762, 8 GPUs 946 / 933-954 GB/s, profiles/r06/c3_tail_crc_placement_ab.jsonl)
        if crc_after_sha is None:
            crc_after_sha = min(self.cap, n) < window_stream_cap(D, 1 << 62)  # the device's cap
        self.crc_after_sha = bool(crc_after_sha)
        # "auto": a thread predicted free before the queued window ends takes its chain from the
        # previous window's midstate; "always" / "never": every takeover does / none does (tests)
        assert from_previous in ("auto", "always", "never"), from_previous
        self.from_previous = from_previous
        # the loop copies each generated piece down, whole, on one stream into a pinned twin of
        # its slot (an event a slot); the threads only hash host memory
        self.copy_s = self._stream()
        # the stolen chains' pieces are generated on a stream of their own (the loop waits for
        # them), the windows' bytes on gen_s behind an event the loop polls while it keeps the
        # threads' rings full (a blocking wait there left the rings unserviced for most of each
        # window: 10.5 of 12.5 s on the 8-GPU shard, 19.2 of 21.7 at N=1)
        self.piece_s = self._stream()
        self.gen_ev = [self._event(polling=True) for _ in range(2)]
        self.hbuf = [[D.PinnedArray((self.piece,), np.uint8, dma_target=True) for _ in range(self.ring)]
                     for _ in range(self.H)]
        self.slot_ev = [[self._event(polling=True) for _ in range(self.ring)] for _ in range(self.H)]
        # every twin written once by DMA before the run (a page's first device write runs at
        # about half the rate: 30 vs 56 GB/s measured), then the twins' copy rate, a record
        # beside the run's copy waits
        for _ in range(2):
            t0 = time.perf_counter()
            for i in range(self.H):
                for k in range(self.ring):
                    D.check(D.lib.krk_memcpy_d2h_async(C.c_void_p(self.hbuf[i][k].ptr),
                                                       C.c_void_p(self.tbuf[i][k].ptr), self.piece, self.copy_s))
            D.check(D.lib.krk_stream_sync(self.copy_s))
            self.twin_GBps = self.H * self.ring * self.piece / (time.perf_counter() - t0) / 1e9
        self.stats = {}
        self._st = None  # the run in progress (_TailState)

    # ---- the host threads: copy and hash
    def _job(self, i, b, y, win, h0):
        """Chain b from byte y: its pieces as the loop generates them into this thread's ring,
        SHA-256 continued from `h0` (a midstate the loop read at hand-over), else from the
        midstate window `win` left (mirrored to host memory; the loop announces each window's
        end in win_done, so a worker makes no HIP call to learn it), or from the IV when
        y == 0."""
        D, st = self.D, self._st
        pieces = chain_pieces(y, int(self.lens[b]), self.piece)
        nch = len(pieces)
        ph = st.phase[i]
        clk = time.perf_counter
        h = _IV.copy()
        if h0 is not None:
            h = h0
        elif y:
            tw = clk()
            with st.cv:
                done = st.win_done >= win
                while st.win_done < win and not st.abort:  # the window that last advanced b
                    st.cv.wait()
                if st.abort:
                    return
            h = self.state_host[win & 1].a[b].copy()  # copied down before that window's event
            dt = clk() - tw
            ph["midstate"] += dt
            st.mwaits[i].append((dt, done, tw - st.t_assigned.get((i, b), tw)))
        out = np.zeros(32, dtype=np.uint8)
        for c in range(nch):
            t1 = clk()
            with st.cv:  # the next piece of this thread, generated by the loop
                while not st.rings.ready[i] and not st.abort:
                    st.cv.wait()
                if st.abort:
                    return
                k, pb, po, pm = st.rings.ready[i].pop(0)
            assert pb == b and (po, pm) == pieces[c], (pb, po, pm, b, y, c)
            t2 = clk()
            if pm:
                D.check(D.lib.krk_event_sync(self.slot_ev[i][k]))  # the loop's copy of the piece
            ph["copy_wait"] += clk() - t2
            D.check(D.lib.krk_sha256_resume_host(h.ctypes.data_as(C.POINTER(C.c_uint32)), po,
                                                 C.c_void_p(self.hbuf[i][k].ptr), pm, int(c + 1 == nch),
                                                 out.ctypes.data_as(C.POINTER(C.c_uint8))))
            t3 = clk()
            ph["device"] += t2 - t1
            ph["hash"] += t3 - t2
            with st.cv:
                st.rings.slot_used[i][k] = False  # copied down: the loop may refill it once its CRC ran
                st.left[i] -= pm
                st.t_last[i] = t3
                st.done_bytes[i] += pm
                st.cv.notify_all()
        st.dig[b] = out

    def _worker(self, i):
        st = self._st
        try:
            self.D.set_device(self.device)
            w, hh = C.c_double(), C.c_double()
            self.D.check(self.D.lib.krk_sha256_resume_stats(C.byref(w), C.byref(hh)))
            h0 = hh.value  # this thread's SHA-NI seconds so far
            while True:
                with st.cv:
                    while not st.jobs[i] and not st.done and not st.abort:
                        st.cv.wait()
                    if not st.jobs[i] or st.abort:
                        break
                    job = st.jobs[i][0]
                t0 = time.perf_counter()
                self._job(i, *job)
                with st.cv:
                    st.jobs[i].pop(0)
                    st.busy_s[i] += time.perf_counter() - t0
                    st.cv.notify_all()
            self.D.check(self.D.lib.krk_sha256_resume_stats(C.byref(w), C.byref(hh)))
            st.phase[i]["sha"] = hh.value - h0
        except BaseException as e:  # re-raised on the caller's thread
            st.err.append(e)
            with st.cv:
                st.abort = True
                st.cv.notify_all()
        finally:
            with st.cv:
                st.alive -= 1
                st.cv.notify_all()

    def _free_at(self, i, now):
        """When thread i is expected to be done with its queued chains, at the rate its pieces
        have been copied and hashed so far (not counting its waits for midstates: a thread
        predicted late gets its next chain late and then waits for it)."""
        st = self._st
        t = st.phase[i]["hash"]
        rate = st.done_bytes[i] / t if t > 0.3 else self.h
        return (st.t_last[i] if st.jobs[i] else now) + max(0, st.left[i]) / max(rate, 1e6)

    # ---- the loop's side: generate pieces into free slots, queue their CRCs
    def _assign(self, i, b, y, win, h0=None, crc_from=None):
        """Chain b from byte y (its midstate after window `win`, or h0) becomes thread i's
        next job (caller holds the lock).  Its pieces' CRCs cover bytes from crc_from (y
        unless a window already summed [y, crc_from))."""
        st = self._st
        st.jobs[i].append((b, y, win, h0))
        st.t_assigned[(i, b)] = time.perf_counter()
        L = int(self.lens[b])
        cf = y if crc_from is None else int(crc_from)
        for o, m in chain_pieces(y, L, self.piece):
            st.rings.to_gen[i].append((b, o, m, min(m, max(0, cf - o))))
        st.left[i] += L - y

    def _service(self):
        """Every free ring slot (copied down, its CRC queued and done) refilled with its thread's next
        piece: generated on the generator stream, waited for, handed to the thread; their CRCs
        go with the next flush.  Returns the pieces generated."""
        D, st = self.D, self._st
        with st.cv:  # krk_event_query is the only device call made under the lock
            gen = st.rings.claim(lambda ev: _event_done(D, ev))
        if not gen:
            return gen
        live = [g for g in gen if g[4] > 0]
        if live:
            ptr = np.array([self.tbuf[i][k].ptr for i, k, _, _, _, _ in live], dtype=np.uint64)
            bl = np.array([g[2] for g in live], dtype=np.int64)
            tg = time.perf_counter()
            D.synth_fill_chunk_arrays(self.ids[bl], ptr, np.array([g[3] for g in live], np.uint64),
                                      np.array([g[4] for g in live], np.uint64), stream=self.piece_s)
            D.check(D.lib.krk_stream_sync(self.piece_s))
            st.gen_wait[0] += time.perf_counter() - tg
            for i, k, _, _, m, _ in live:  # each piece down into its slot's pinned twin, then its event
                D.check(D.lib.krk_memcpy_d2h_async(C.c_void_p(self.hbuf[i][k].ptr), C.c_void_p(self.tbuf[i][k].ptr),
                                                   m, self.copy_s))
                D.check(D.lib.krk_event_record(self.slot_ev[i][k], self.copy_s))
        with st.cv:
            st.rings.publish(gen)
            st.cv.notify_all()
        st.tail_pieces += len(gen)
        return gen

    def _flush_crcs(self, mirror=None):
        """Queue on run_s (the tail CRCs go nowhere else) the CRCs of the pieces generated since
        the last flush, record an event behind them and hold their slots until it is done.
        mirror=j: the flush after a window's step -- the midstates' copy into host mirror j goes
        between the CRCs and the event, and the event is recorded even with no CRC to queue (it
        is the window's).  Returns the event, None if none was needed."""
        D, st = self.D, self._st
        with st.cv:
            take = st.rings.take_pending()
        if take:
            ptr = np.array([self.tbuf[i][k].ptr + c0 for i, k, _, _, _, c0 in take], dtype=np.uint64)
            bl = np.array([t[2] for t in take], dtype=np.int64)
            arr = D.chunk_array(ptr, np.array([t[3] for t in take], np.uint64),
                                np.array([t[4] for t in take], np.uint64), self.cb.lengths[bl],
                                self.cb.piece_lengths[bl], self.cb.sums_off[bl], bl.astype(np.uint64))
            D.check(D.lib.krk_chunks_crc_dev(arr.ctypes.data_as(C.POINTER(D.krk_chunk)), len(take),
                                             self.cb.sums.ptr, self.run_s))
        if mirror is not None:
            D.check(D.lib.krk_memcpy_d2h_async(C.c_void_p(self.state_host[mirror].ptr), C.c_void_p(self.cb.state.ptr),
                                               32 * self.lens.size, self.run_s))
        elif not take:
            return None
        ev = _new_event(D)
        st.events.append(ev)
        D.check(D.lib.krk_event_record(ev, self.run_s))
        with st.cv:
            st.rings.release(take, ev)
        return ev

    def _wait_window(self, ev):
        """Until window event `ev` completes, keep the threads' rings full."""
        st = self._st
        while not _event_done(self.D, ev):
            if not self._service():
                with st.cv:
                    st.cv.wait(0.002)

    def _gen_window(self, win, k):
        """Window k's bytes generated on gen_s; gen_ev[k & 1] marks them done."""
        items = self._items(win, k)
        self._gen(items)
        self.D.check(self.D.lib.krk_event_record(self.gen_ev[k & 1], self.gen_s))
        return items

    # ---- run(), step by step
    def _start_workers(self, pol, t0):
        """The threads, each with one of the longest chains whole."""
        st = self._st
        with st.cv:
            for i, b in enumerate(pol.initial()):
                self._assign(i, b, 0, None)
                st.t_last[i] = t0
                st.host_blobs.add(b)
                st.host_bytes += int(self.lens[b])
        workers = [threading.Thread(target=self._worker, args=(i,), name=f"krk-tail-{i}") for i in range(self.H)]
        for w in workers:
            w.start()
        return workers

    def _queue_window(self, pol, win, items, k):
        """Window k, once its bytes are there: its step, the tail CRCs generated so far, its
        midstates' mirror copy and its event, all on run_s.  Returns its modelled seconds."""
        st = self._st
        blobs, offs, tk = win
        tg = time.perf_counter()
        self._wait_window(self.gen_ev[k & 1])  # window k's bytes
        st.gen_wait[1] += time.perf_counter() - tg
        pol.queued(blobs, offs, tk)
        self.cb.step_arrays(*items, stream=self.run_s, sha_stream=self.sha_s, crc_after_sha=self.crc_after_sha)
        st.wev.append(self._flush_crcs(mirror=k & 1))
        return window_seconds(self.rates, tk, blobs.size)

    def _window_ended(self, k):
        """Wait for window k (the rings serviced meanwhile), then tell the threads."""
        st = self._st
        self._wait_window(st.wev[k])
        with st.cv:
            st.win_done = k
            st.cv.notify_all()

    def _wait_previous(self, k):
        """Window k is queued: wait for window k-1, and update the measured / modelled scale."""
        st = self._st
        tw = time.perf_counter()
        self._window_ended(k - 1)
        now = time.perf_counter()
        st.wait_win_s += now - tw
        st.scale = 0.7 * st.scale + 0.3 * max(0.2, min(5.0, (now - st.t_prev_end) / max(st.last_model, 1e-6)))
        st.t_prev_end = now

    def _hand_over(self, pol, sched, win, k, model):
        """The boundary before window k (queued, `model` seconds long) ends: TailPolicy.handover
        over the threads' expected free times, among the threads with at most their current
        chain; each chain becomes its thread's next job."""
        st = self._st
        blobs, offs, _ = win
        now = time.perf_counter()
        end_k = now + model * st.scale
        horizon = end_k + TAIL_HORIZON * model * st.scale  # later windows modelled like k
        with st.cv:
            free_at = [self._free_at(i, now) for i in range(self.H)]
            one_chain = [len(j) <= 1 for j in st.jobs]
        moves = pol.handover(sched, free_at, horizon, stream_rate(self.rates, blobs.size) * model, one_chain)
        with st.cv:
            for i, b, y in moves:
                if not st.jobs[i]:
                    st.t_last[i] = now
                before_k = self.from_previous == "always" or (self.from_previous == "auto" and free_at[i] < end_k)
                if y and before_k:
                    # free before window k ends: start from the midstate window k-1 left
                    # (done, mirrored, read now), hashing window k's chunk of b again on
                    # the host; the window keeps that chunk's CRC, the thread's pieces
                    # sum from y on
                    j = np.flatnonzero(blobs == b)
                    yp = int(offs[j[0]]) if j.size else y
                    h0 = self.state_host[(k - 1) & 1].a[b].copy() if yp else _IV.copy()
                    self._assign(i, b, yp, -1, h0=h0, crc_from=y)
                    st.early += 1
                else:
                    yp = y
                    self._assign(i, b, y, k if y else -1)
                st.host_blobs.add(b)
                st.host_bytes += int(self.lens[b]) - yp
                st.takes += 1
                st.resumed += yp > 0
            st.cv.notify_all()

    def _run_windows(self, pol, sched):
        """Window k's step is queued before the host waits for window k-1; chains change hands
        after that wait; window k+1 is generated meanwhile."""
        st = self._st
        self._service()
        win, k = sched.next(), 0
        if win is not None:
            items = self._gen_window(win, 0)
        st.t_prev_end = time.perf_counter()
        while win is not None and not st.err:
            model = self._queue_window(pol, win, items, k)
            if k:
                self._wait_previous(k)
            st.last_model = model
            self._hand_over(pol, sched, win, k, model)
            self._service()
            win, k = sched.next(), k + 1
            if win is not None:
                items = self._gen_window(win, k)
        if st.wev:
            self._window_ended(len(st.wev) - 1)

    def _drain(self):
        """The windows are done: keep the rings full and the pieces' CRCs flushed until every
        thread is done."""
        st = self._st
        with st.cv:
            st.done = True
            st.cv.notify_all()
        while not st.err:
            with st.cv:
                if st.alive == 0:
                    break
            self._service()
            self._flush_crcs()
            with st.cv:
                st.cv.wait(0.002)
        self._flush_crcs()  # the last pieces (every thread is done)

    def _stats(self):
        st = self._st
        return {"windows": len(st.wev), "gpu_windows_end_s": round(st.gpu_end, 3),
                "takeovers": st.takes, "resumed_from_midstate": st.resumed, "from_previous_window": st.early,
                "host_chains": len(st.host_blobs),
                "host_bytes": st.host_bytes, "tail_pieces": st.tail_pieces,
                "thread_busy_s": [round(x, 3) for x in st.busy_s],
                "thread_GBps": [round(st.done_bytes[i] / max(st.busy_s[i], 1e-9) / 1e9, 3) for i in range(self.H)],
                "thread_phases_s": {k: round(sum(p.get(k, 0.0) for p in st.phase), 3)
                                    for k in ("midstate", "device", "hash", "copy_wait", "sha")},
                "loop_wait_s": round(st.wait_win_s, 3), "window_time_scale": round(st.scale, 3),
                "midstate_waits": _wait_summary([w for ws in st.mwaits for w in ws]),
                "twin_copy_GBps_before_run": round(self.twin_GBps, 2), "crc_after_sha": self.crc_after_sha,
                "loop_generate_s": {"tail_pieces": round(st.gen_wait[0], 3), "windows": round(st.gen_wait[1], 3)}}

    def run(self):
        D = self.D
        st = self._st = _TailState(self.H, self.ring, self.lens.size)
        pol = TailPolicy(self.lens, self.H)
        t0 = time.perf_counter()
        workers = self._start_workers(pol, t0)
        sched = _Sched(self.lens, np.nonzero(pol.on_gpu)[0], self.W, self.cap, self.max_chunk)
        try:
            self._run_windows(pol, sched)
            st.gpu_end = time.perf_counter() - t0
            self._drain()
        except BaseException:  # the loop failed: the threads must not wait for it
            with st.cv:
                st.abort = True
                st.cv.notify_all()
            raise
        finally:
            with st.cv:
                st.done = True
                if st.err:
                    st.abort = True
                st.cv.notify_all()
            for w in workers:
                w.join()
            sched.close()
        try:
            if st.err:
                raise st.err[0]
            D.check(D.lib.krk_stream_sync(self.run_s))  # the last tail CRCs
            _write_digests(D, self.cb, st.dig, sorted(st.host_blobs))
        finally:
            D.lib.krk_stream_sync(self.run_s)
            for e in st.events:
                D.lib.krk_event_destroy(e)
        self.stats = self._stats()

    def close(self):
        self._close(self.bufs + [x for ring in self.tbuf for x in ring])
        self.bufs, self.tbuf, self.hbuf = [], [], []
