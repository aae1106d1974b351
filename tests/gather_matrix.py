"""The host gather kernel (gather.hip) at its funnel, lane, unroll, stride and tile edges: the
cases, the expected image of the destination and the comparison, shared by
tests/test_gpu_gather_matrix.py (krk_gather_spans_dev on the production library) and
tests/test_gather_matrix_cpu.py (the case lists and the image builder, no device).  A helper
module, not a test file.

Sources are views into ONE page-locked arena (krk_host_alloc, 2 MiB of seeded random bytes),
each placed so that src % 16 is the wanted residue r; views overlap freely (the kernel only
reads).  Destinations are packed into ONE device buffer prefilled with a canary byte: a span's
dst is the running offset rounded up to 16, and 16 canary bytes follow every span's room.  The
expected image of the WHOLE buffer is built with numpy -- canary everywhere, then each span's
bytes -- and compared in one array_equal under a mask that leaves out only bytes
[n, roundup16(n)) of each span, the room the kernel's contract gives it: a stray write
anywhere else fails.

Groups (kGatherTile 65536, 16-byte words, 64 lanes x kUnroll 4 x 4 waves of gather.hip):
 A  every r x out_words around 64 (lane 63 loads the next word itself), 256 (a wave's unroll),
    1024 (the workgroup's stride) and 4096 (the tile) x last-word byte counts either side of
    in_words == out_words + 1, in ONE call: more tiles than a grid, so the tile stride runs;
 B  spans of three and four tiles: a source residue must survive every tile of a span;
 C  group A's spans over three calls on one stream with no synchronisation between, with
    zero-length spans (src NULL) mixed in and sources that end at the arena's last byte.

`python -m tests.gather_matrix` runs every group on the device and prints one JSON line a
group (spans, bytes, tiles, mismatches, seconds); it exits 1 on any mismatch."""
import ctypes as C
import json
import sys
import time
from collections import namedtuple

import numpy as np

from kraken_amd import device as D
from kraken_amd._capi import check, lib

K_TILE = 65536
ARENA_BYTES = 2 << 20
SEED = 20261019
CANARY = 0xA7
GAP = 16
GROUPS = ("A", "B", "C")

OUT_WORDS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097)
B_RESIDUES = (0, 1, 4, 7, 8, 15)
B_TILES = (2, 3)  # whole tiles before the last, short one
C_ZERO_EVERY = 50  # a zero-length span after every 50th span of group C
C_END_WORDS = (1, 64, 257)  # out_words of the spans that end at the arena's last byte

# One span: n bytes from arena offset `src` (None: a NULL source, n == 0) to byte `dst` of the
# destination buffer.
Span = namedtuple("Span", "src n dst")


def roundup16(x):
    return (x + 15) & ~15


def tails(r):
    """Byte counts of a span's last word: 1, 8, 15, 16 and, for r > 0, the two either side of
    in_words growing by one (r + t > 16)."""
    t = {1, 8, 15, 16}
    if r:
        t |= {16 - r, min(16, 17 - r)}
    return sorted(t)


def out_words(s):
    return (s.n + 15) // 16


def in_words(s):
    return ((s.src % 16) + s.n + 15) // 16 if s.n else 0


def n_tiles(spans):
    return sum((s.n + K_TILE - 1) // K_TILE for s in spans)


def _place(rng, n, r):
    """A seeded arena offset with off % 16 == r whose view lies inside the arena."""
    top = (ARENA_BYTES - n - r) // 16
    assert top >= 0, "the arena is too small for this view"
    return 16 * int(rng.integers(0, top + 1)) + r


def layout(sized):
    """[(src, n)] -> spans packed into the destination buffer, and the buffer's size: GAP bytes
    of canary, then every span at the running offset rounded up to 16 with GAP bytes after its
    room (a zero-length span takes no room and shares the next span's dst)."""
    out, o = [], GAP
    for src, n in sized:
        o = roundup16(o)
        out.append(Span(src, n, o))
        if n:
            o += roundup16(n) + GAP
    return out, roundup16(o)


def sized_a():
    rng = np.random.default_rng(SEED + 1)
    out = []
    for r in range(16):
        for w in OUT_WORDS:
            for t in tails(r):
                n = 16 * (w - 1) + t
                out.append((_place(rng, n, r), n))
    return out


def sized_b():
    rng = np.random.default_rng(SEED + 2)
    out = []
    for r in B_RESIDUES:
        for k in B_TILES:
            for t in tails(r):
                n = k * K_TILE + t
                out.append((_place(rng, n, r), n))
    return out


def sized_c_extra():
    """Sources that end at the arena's last byte, one a residue and C_END_WORDS entry: n is
    chosen so that (ARENA_BYTES - n) % 16 == r."""
    out = []
    for r in range(16):
        for w in C_END_WORDS:
            n = 16 * w - r
            out.append((ARENA_BYTES - n, n))
    return out


def sized_c():
    """Group A's spans with a zero-length span after every C_ZERO_EVERY-th and the arena-end
    spans spread among them."""
    a, extra = sized_a(), sized_c_extra()
    step = len(a) // len(extra)
    out = []
    for k, s in enumerate(a):
        out.append(s)
        if k % C_ZERO_EVERY == C_ZERO_EVERY - 1:
            out.append((None, 0))
        if k % step == step - 1 and k // step < len(extra):
            out.append(extra[k // step])
    return out


def cases(group):
    """(spans, destination bytes, the calls as lists of span indices) of a group."""
    if group == "A":
        spans, size = layout(sized_a())
        return spans, size, [list(range(len(spans)))]
    if group == "B":
        spans, size = layout(sized_b())
        return spans, size, [list(range(len(spans)))]
    spans, size = layout(sized_c())
    idx = list(range(len(spans)))
    return spans, size, [idx[0::3], idx[1::3], idx[2::3]]


def make_arena_bytes():
    return np.random.default_rng(SEED).integers(0, 256, size=ARENA_BYTES, dtype=np.uint8)


def expected_image(arena, spans, size):
    """(image, mask): the destination buffer after the gather -- canary everywhere, then each
    span's bytes -- and the bytes that are compared: all but [n, roundup16(n)) of each span."""
    want = np.full(size, CANARY, dtype=np.uint8)
    mask = np.ones(size, dtype=bool)
    for s in spans:
        if not s.n:
            continue
        want[s.dst:s.dst + s.n] = arena[s.src:s.src + s.n]
        mask[s.dst + s.n:s.dst + roundup16(s.n)] = False
    return want, mask


def disjoint(spans, size):
    """No two spans' rooms (n rounded up to 16) overlap, each has GAP bytes before and after it
    that belong to no span, and all lie inside the buffer."""
    rooms = sorted((s.dst, s.dst + roundup16(s.n)) for s in spans if s.n)
    if not rooms or rooms[0][0] < GAP or rooms[-1][1] + GAP > size:
        return False
    return all(b0 - a1 >= GAP for (_, a1), (b0, _) in zip(rooms[:-1], rooms[1:]))


def compare(label, spans, got, want, mask):
    """Mismatches of the whole destination buffer as (description, got, want): one entry a span
    with a wrong byte (its first), one for each stray byte outside every span's room (the first
    ten)."""
    if got.size == want.size and np.array_equal(got[mask], want[mask]):
        return []
    if got.size != want.size:
        return [(f"{label}: {got.size} bytes read back, {want.size} expected", 0, 0)]
    bad = np.nonzero((got != want) & mask)[0]
    live = [s for s in spans if s.n]
    starts = np.array([s.dst for s in live], dtype=np.int64)
    ends = starts + np.array([s.n for s in live], dtype=np.int64)
    k = np.searchsorted(starts, bad, side="right") - 1
    inside = (k >= 0) & (bad < ends[np.maximum(k, 0)])
    firsts = bad[inside][np.unique(k[inside], return_index=True)[1]]  # the first wrong byte of each span
    out = []
    for i in np.sort(np.concatenate([firsts, bad[~inside][:10]])):
        j = int(np.searchsorted(starts, i, side="right")) - 1
        if j >= 0 and i < ends[j]:
            s = live[j]
            desc = (f"{label} span r={s.src % 16} n={s.n} out_words={out_words(s)} in_words={in_words(s)} "
                    f"byte {int(i - s.dst)} (word {int(i - s.dst) // 16})")
        else:
            desc = f"{label} byte {int(i)} outside every span (canary)"
        out.append((desc, int(got[i]), int(want[i])))
    return out


# ------------------------------------------------------------------ the device side
def gather_call(arena_ptr, dst_ptr, spans, stream=None):
    """One krk_gather_spans_dev call over `spans`; the return code."""
    n = len(spans)
    src = np.array([arena_ptr + s.src if s.src is not None else 0 for s in spans], dtype=np.uint64)
    dst = np.array([dst_ptr + s.dst for s in spans], dtype=np.uint64)
    ln = np.array([s.n for s in spans], dtype=np.uint64)
    vpp = C.POINTER(C.c_void_p)
    return lib.krk_gather_spans_dev(src.ctypes.data_as(vpp), dst.ctypes.data_as(vpp),
                                    ln.ctypes.data_as(C.POINTER(C.c_uint64)), n, stream)


class DeviceBackend:
    """The arena in page-locked host memory and one destination buffer a group."""

    def __init__(self):
        self.arena = D.PinnedArray((ARENA_BYTES,), np.uint8)
        assert self.arena.ptr % 16 == 0
        self.arena.a[:] = make_arena_bytes()
        self.host = self.arena.a
        self._want = {}

    def close(self):
        self.arena = None

    def want(self, group):
        """(spans, size, calls, image, mask) of a group, computed once and left unchanged."""
        v = self._want.get(group)
        if v is None:
            spans, size, calls = cases(group)
            assert disjoint(spans, size)
            image, mask = expected_image(self.host, spans, size)
            image.setflags(write=False)
            mask.setflags(write=False)
            v = self._want[group] = (spans, size, calls, image, mask)
        return v

    def run(self, group):
        """The destination buffer after the group's calls."""
        spans, size, calls, _, _ = self.want(group)
        buf = D.DeviceBuffer(size)
        stream = C.c_void_p()
        try:
            assert buf.ptr % 16 == 0
            buf.from_host(np.full(size, CANARY, dtype=np.uint8))
            if len(calls) > 1:
                check(lib.krk_stream_create(C.byref(stream)))
            for call in calls:  # no synchronisation between the calls
                check(gather_call(self.arena.ptr, buf.ptr, [spans[i] for i in call], stream if stream.value else None))
            check(lib.krk_stream_sync(stream if stream.value else None))
            return buf.to_host(np.uint8, size)
        finally:
            if stream.value:
                lib.krk_stream_destroy(stream)
            buf.free()


def run_group_counted(group, backend):
    """(spans, mismatches) of a group on the device."""
    spans, _, _, image, mask = backend.want(group)
    return len(spans), compare(group, spans, backend.run(group), image, mask)


def main(argv):
    backend = DeviceBackend()
    failed = False
    try:
        for g in GROUPS:
            t0 = time.perf_counter()
            n, bad = run_group_counted(g, backend)
            failed |= bool(bad)
            spans = backend.want(g)[0]
            print(json.dumps({"group": g, "spans": n, "bytes": sum(s.n for s in spans), "tiles": n_tiles(spans),
                              "n_mismatches": len(bad), "mismatches": bad[:10],
                              "seconds": round(time.perf_counter() - t0, 3)}), flush=True)
    finally:
        backend.close()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
