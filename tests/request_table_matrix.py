"""Request table rounds (request_table.hip, request_table_math.hpp) at the kernel's chunk, word and
launch edges: cases, expectations and comparison shared by tests/test_gpu_request_table_matrix.py
(the device form), tests/test_request_table_matrix_cpu.py (the host form) and
tests/test_request_table_math_native.py (the header alone).  A helper module, not a test file.
Shapes come from krk_request_table_geometry; a torrent's expectation is tests/request_table_ref.py,
never the library, and the named cases carry hand-worked values too.  Arrays start at non-zero
offsets with SPARE elements past their ends, outputs are prefilled with 0xA5 and blocked rows with
noise: every whole buffer is compared, state and outputs."""
import ctypes as C
import functools

import numpy as np

from kraken_amd import _capi
from kraken_amd._capi import check, lib
from kraken_amd.device import RT_ENTRY
from tests import request_table_ref as R

SEED, SPARE, NONE = 20261126, 4, 0xFFFFFFFF
DUP, EXPIRED, UNSENT, INVALID = R.ALLOW_DUPLICATES, R.EXPIRED, R.UNSENT, R.INVALID
_c, _t = C.c_uint64(), C.c_uint64()
check(lib.krk_request_table_geometry(C.byref(_c), C.byref(_t)))
CHUNK, CAP = int(_c.value), int(_t.value)
assert CAP == _capi.KRK_RT_MAX_ENTRIES
ENTRIES = (0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, CAP)
NS, PS, LIMITS = (1, 63, 64, 65, 4097), (0, 1, 2, 10, 300), (1, 3, 16)
LISTS = ("arrived", "gone", "marks", "holds", "records")
WIDTH = {"arrived": 1, "gone": 1, "marks": 3, "holds": 2, "records": 2}  # uint32 words an element
NOW, TIMEOUT = 1000, 50
OUTPUTS = ("bits", "entries", "n_entries", "quota", "failed", "n_failed", "n_dropped")


def row(pieces, W):
    x = 0
    for i in pieces:
        x |= 1 << i
    return np.frombuffer(x.to_bytes(8 * W, "little"), dtype=np.uint64)


class Torrent:
    """have / held[p]: sets of bits; table: [(piece, peer, status, sent_at)]; picks: a list a peer or None."""

    def __init__(self, label, n, P, flags=0, have=(), held=None, table=(), cap=None, picks=None, **ev):
        self.label, self.n, self.P, self.flags, self.have = label, n, P, flags, set(have)
        self.held = [set(h) for h in (held or [()] * P)]
        self.table, self.cap, self.picks = list(table), len(table) if cap is None else cap, picks
        self.ev = {k: list(ev.get(k, ())) for k in LISTS}


def random_torrent(n_entries, n, P, flags, limit, salt=0, cap=None):
    rng = np.random.default_rng([SEED, n_entries, n, P, flags, limit, salt])
    W = (n + 63) // 64
    pick = lambda k, hi: sorted(int(x) for x in rng.choice(hi, size=min(k, hi), replace=False)) if hi else []  # noqa: E731
    held = [set(np.flatnonzero(rng.random(64 * W) < 0.4).tolist()) for _ in range(P)]  # tail bits included
    sent = [NOW - TIMEOUT - 1, NOW - TIMEOUT, NOW]
    table = [(int(rng.integers(n)), int(rng.integers(P)), int(rng.choice([0, 0, 0, 1, 2, 3])), sent[rng.integers(3)])
             for _ in range(n_entries if P else 0)]
    for k in range(0, len(table), 37):  # entries no valid round wrote: dropped with the removed
        table[k] = [(n, 0, 0, NOW), (0, P, 0, NOW), (0, 0, 4, NOW)][k % 3]
    if not P:
        table = [(0, 0, 0, NOW)] * n_entries
    ev = {"arrived": pick(3, n), "gone": pick(2, P) if salt % 2 else [],
          "marks": [(e[0], e[1], UNSENT + k % 2) for k, e in enumerate(table[::29]) if e[0] < n and e[1] < P],
          "holds": sorted({(int(rng.integers(n)), int(rng.integers(P))) for _ in range(5 if P else 0)}, key=lambda h: h[::-1]),
          "records": [(int(rng.integers(n)), int(rng.integers(P))) for _ in range(3 if P else 0)]}
    picks = [[int(x) if x <= n else NONE - 1 for x in rng.integers(n + 2, size=rng.integers(limit + 1))] for _ in range(P)]
    return Torrent(f"random E={n_entries} n={n} P={P} flags={flags:#x} L={limit} salt={salt}", n, P, flags,
                   np.flatnonzero(rng.random(64 * W) < 0.25).tolist(), held, table,
                   max(n_entries, 8) if cap is None else cap, picks if salt % 3 else None, **ev)


class Batch:
    """Torrents packed back to back from non-zero offsets, in the order given; one round's scalars."""

    def __init__(self, torrents, limit=3, now=NOW, timeout=TIMEOUT, label=None):
        self.torrents, self.limit, self.now, self.timeout = list(torrents), limit, now, timeout
        self.label = label or " | ".join(t.label for t in self.torrents)
        k = len(self.torrents)
        self.structs = (_capi.krk_request_torrent * max(k, 1))()
        self.tables = (_capi.krk_table_torrent * max(k, 1))()
        at = {"w": 3, "p": 5, "e": 7, **{name: 2 for name in LISTS}}
        self.offs, lists = [], {name: [9] * 2 * WIDTH[name] for name in LISTS}  # two elements nobody owns
        for j, t in enumerate(self.torrents):
            self.offs.append(dict(at))
            W = (t.n + 63) // 64
            self.structs[j] = _capi.krk_request_torrent(t.n, t.P, t.flags | (j & 1), 77 * j, at["w"], at["p"], 1 << 40)
            self.tables[j] = _capi.krk_table_torrent(at["e"], t.cap, 0, *(x for name in LISTS for x in (at[name], len(t.ev[name]))))
            for name in LISTS:
                lists[name] += [int(x) for e in t.ev[name] for x in (e if WIDTH[name] > 1 else (e,))]
                at[name] += len(t.ev[name])
            at["w"], at["p"], at["e"] = at["w"] + (1 + 2 * t.P) * W, at["p"] + t.P, at["e"] + t.cap
        rng = np.random.default_rng([SEED, k, at["w"]])
        a = self.arrays = {name: np.full(size, 0xA5A5A5A5, dtype=np.uint32) for name, size in
                           (("n_entries", k + SPARE), ("quota", at["p"] + SPARE), ("failed", 3 * (at["e"] + SPARE)),
                            ("n_failed", k + SPARE), ("n_dropped", k + SPARE), ("n_picked", at["p"] + SPARE),
                            ("picks", (at["p"] + SPARE) * limit))}
        a["bits"] = rng.integers(1 << 63, size=at["w"] + SPARE, dtype=np.uint64)  # noise where the blocked rows are
        a["entries"] = np.full(at["e"] + SPARE, 0xA5, dtype=np.uint8).repeat(24).view(RT_ENTRY)
        self.has_picks = any(t.picks is not None for t in self.torrents)
        for j, (t, o) in enumerate(zip(self.torrents, self.offs)):
            W = (t.n + 63) // 64
            rows = a["bits"][o["w"]:o["w"] + (1 + 2 * t.P) * W].reshape(1 + 2 * t.P, W)
            rows[0] = row(t.have, W)
            for p in range(t.P):
                rows[1 + 2 * p] = row(t.held[p], W)
                pk = (t.picks[p] if t.picks is not None else [])
                a["n_picked"][o["p"] + p] = len(pk)
                a["picks"][(o["p"] + p) * limit:(o["p"] + p + 1) * limit] = pk + [NONE] * (limit - len(pk))
            a["entries"][o["e"]:o["e"] + len(t.table)] = [(e[0], e[1], e[2], 0, e[3]) for e in t.table]
            a["n_entries"][j] = len(t.table)
        self.lists = {name: np.asarray(lists[name], dtype=np.uint32) for name in LISTS}
        self._want = None

    def want(self):
        """Every buffer of OUTPUTS after the call."""
        if self._want is None:
            w = {name: self.arrays[name].copy() for name in OUTPUTS}
            for j, (t, o) in enumerate(zip(self.torrents, self.offs)):
                W = (t.n + 63) // 64
                have, held, table, blocked, quota, failed, dropped = R.round_torrent(
                    t.n, t.P, t.flags, t.have, t.held, t.table, t.cap, picks=t.picks if self.has_picks else None,
                    now=self.now, timeout=self.timeout, limit=self.limit, **t.ev)
                rows = w["bits"][o["w"]:o["w"] + (1 + 2 * t.P) * W].reshape(1 + 2 * t.P, W)
                rows[0] = row(have, W)
                for p in range(t.P):
                    rows[1 + 2 * p], rows[2 + 2 * p] = row(held[p], W), row(blocked[p], W)
                w["entries"][o["e"]:o["e"] + len(table)] = [(e[0], e[1], e[2], 0, e[3]) for e in table]
                w["failed"][3 * o["e"]:3 * (o["e"] + len(failed))] = np.asarray(failed, dtype=np.uint32).reshape(-1)
                w["quota"][o["p"]:o["p"] + t.P] = quota
                w["n_entries"][j], w["n_failed"][j], w["n_dropped"][j] = len(table), len(failed), dropped
            self._want = w
        return self._want

    def args(self, ptr, failed=True):
        """The argument list of a round call (without the stream); ptr: {array name: address}."""
        lp = [self.lists[name].ctypes.data for name in LISTS]
        pk = [ptr["picks"], ptr["n_picked"]] if self.has_picks else [None, None]
        return [self.structs, self.tables, len(self.torrents), ptr["bits"], ptr["entries"], ptr["n_entries"], *lp, *pk,
                self.now, self.timeout, self.limit, ptr["quota"], ptr["failed"] if failed else None,
                ptr["n_failed"] if failed else None, ptr["n_dropped"]]


class Backend:
    """The host form over copies of the batch's arrays, or (dev) the device form over uploads of them."""

    def __init__(self, dev=False, pinned=False):
        self.dev, self.pinned = dev, pinned

    def run(self, b, failed=True, change=None):
        from kraken_amd import device as D
        if not self.dev:
            got = {k: v.copy() for k, v in b.arrays.items()}
            args = b.args({k: v.ctypes.data for k, v in got.items()}, failed)
            change and change(args)
            return lib.krk_request_table_round(*args), got
        bufs = {k: D.PinnedArray((v.nbytes,), np.uint8) if self.pinned else D.DeviceBuffer(v.nbytes) for k, v in b.arrays.items()}
        for k, v in b.arrays.items():
            raw = v.view(np.uint8).reshape(-1)
            bufs[k].a.__setitem__(slice(None), raw) if self.pinned else bufs[k].from_host(raw)
        args = b.args({k: v.ptr for k, v in bufs.items()}, failed)
        change and change(args)
        rc = lib.krk_request_table_round_dev(*args, None)
        check(lib.krk_stream_sync(None))
        return rc, {k: (bufs[k].a.copy() if self.pinned else bufs[k].to_host(np.uint8, v.nbytes)).view(v.dtype)
                    for k, v in b.arrays.items()}


def compare(b, got, failed=True, want=None):
    """Mismatches of one call's whole buffers against the restatement's (or `want`), as text."""
    bad, want = [], want or b.want()
    for name in OUTPUTS:
        w, g = want[name], got[name]
        if not failed and name in ("failed", "n_failed"):
            w = b.arrays[name]  # not asked for: not touched
        if g.tobytes() != w.tobytes():
            k = int(np.flatnonzero(g != w)[0])
            bad.append(f"{b.label}: {name}[{k}] is {g[k]}, want {w[k]} ({int((g != w).sum())} differ)")
    return bad


def run_cases(backend, batches):
    """Mismatches of every batch, with and without the failed list."""
    bad = []
    for b in batches:
        for failed in (True, False):
            rc, got = backend.run(b, failed)
            bad += [f"{b.label}: rc {rc}: {lib.krk_last_error()}"] if rc else compare(b, got, failed)
    return bad


def hand_mismatches(b, got, hand):
    """Mismatches of torrent 0's outputs against the values worked out by hand."""
    o, t = b.offs[0], b.torrents[0]
    nf = int(got["n_failed"][0])
    out = {"quota": got["quota"][o["p"]:o["p"] + t.P].astype(np.int32).tolist(), "n_entries": int(got["n_entries"][0]),
           "n_dropped": int(got["n_dropped"][0]),
           "failed": [tuple(x) for x in got["failed"][3 * o["e"]:3 * (o["e"] + nf)].reshape(-1, 3).tolist()]}
    return [f"{b.label}: {k} is {out[k]}, by hand {v}" for k, v in hand.items() if out[k] != v]


@functools.lru_cache(None)
def cases():
    """The matrix (built once): entries x N x P, the limit and the duplicates flag taking turns."""
    return [Batch([random_torrent(e, n, p, (0, DUP)[(k // 3) % 2], LIMITS[k % 3], salt=k)], limit=LIMITS[k % 3])
            for k, (e, n, p) in enumerate((e, n, p) for e in ENTRIES for n in NS for p in PS)]


def batch(k):
    """k torrents that mix the matrix's shapes, an empty and a peerless torrent in the middle."""
    ts = []
    for j in range(k):
        e, n, p = ENTRIES[(2 * j + 1) % 8], NS[(3 * j + 1) % 5], PS[1 + j % 4]
        e, p = (0 if k >= 3 and j == k // 2 else e), (0 if k >= 3 and j == k // 2 + 1 else p)
        ts.append(random_torrent(e, n, p, (0, DUP)[j % 2], 3, salt=100 + j))
    return Batch(ts, label=f"batch of {k}")


def named():
    """[(Batch, {output: torrent 0's values worked out by hand})]: one property a case."""
    out, live, old = [], NOW - TIMEOUT, NOW - TIMEOUT - 1
    T9, T4 = [(i, i % 3, 0, NOW) for i in range(9)], [(i, i % 2, 0, NOW) for i in range(4)]

    def add(hand, label, *a, limit=3, **kw):
        out.append((Batch([Torrent(label, *a, **kw)], limit=limit), hand))

    add({"quota": [2, 3], "failed": [(5, 1, EXPIRED)]}, "sent_at + timeout == now is live, a tick later expired", 65, 2,
        table=[(5, 0, 0, live), (5, 1, 0, old)])
    for flags in (0, DUP):
        add({"quota": [0, 5]}, f"two and three live entries a word, across the 64-bit edge {flags:#x}", 129, 2, flags,
            table=[(i, 0, 0, NOW) for i in (62, 63, 64, 65, 127)], limit=5)
    add({"quota": [2]}, "the last piece's bit: the tail stays clear", 65, 1, held=[range(65, 128)], table=[(64, 0, 0, NOW)])
    add({"quota": [0, 1], "n_entries": 5}, "more live entries than the limit", 65, 2, table=[(i, 0, 0, NOW) for i in range(5)],
        limit=1)
    add({"n_entries": 0}, "everything removed", 65, 3, table=T9, arrived=range(9))
    add({"n_entries": 9}, "nothing removed", 65, 3, table=T9, arrived=[9, 64])
    add({"n_entries": 7}, "the first and the last entry removed", 65, 3, table=T9, arrived=[0, 8])
    add({"n_entries": 6, "quota": [0, 3, 0]}, "a peer gone, and holds on its zeroed row at bits 0, 63 and 64", 65, 3,
        held=[range(70)] * 3, table=T9, gone=[1], holds=[(0, 1), (63, 1), (64, 1)])
    add({"failed": [(3, 0, UNSENT), (3, 0, UNSENT), (4, 0, INVALID)], "quota": [3, 2]},
        "a mark that hits two entries, one that hits none, the later of two wins", 65, 2,
        table=[(3, 0, 0, NOW), (4, 0, 0, NOW), (3, 0, 1, old), (3, 1, 0, NOW)],
        marks=[(3, 0, UNSENT), (9, 1, INVALID), (4, 0, UNSENT), (4, 0, INVALID)])
    add({"failed": [(2, 1, EXPIRED), (7, 2, EXPIRED), (7, 0, INVALID), (7, 1, UNSENT)]}, "the failed list: equal pieces in table order",
        65, 3, table=[(7, 2, 0, old), (2, 1, 0, old), (7, 0, 3, NOW), (1, 0, 0, NOW), (7, 1, 2, NOW)])
    for extra in (0, 1):  # 4 entries in a table of 8
        add({"n_entries": 8, "n_dropped": extra}, f"the explicit list fills cap, overflow {extra}, no picks", 65, 2, table=T4, cap=8,
            records=[(1, 0), (2, 1), (3, 0), (4, 1)] + [(5, 1)] * extra)
        add({"n_entries": 8, "n_dropped": extra + 3}, f"the explicit list fills cap, overflow {extra}, every pick dropped", 65, 2,
            table=T4, cap=8, records=[(1, 0), (2, 1), (3, 0), (4, 1)] + [(5, 1)] * extra, picks=[[10, 11], [12]])
        add({"n_entries": 8, "n_dropped": extra}, f"the picks fill cap, overflow {extra}", 65, 2, table=T4, cap=8,
            records=[(1, 0)], picks=[[10, 11], [12] + [13] * extra])
    add({"n_entries": 2, "n_dropped": 1}, "a pick >= n_pieces", 65, 2, cap=4, picks=[[64, 65], [0]])
    return out


def count_above_cap():
    """A count of 9 in a table of 4: the device form reads it as 4 (the host form refuses it)."""
    b = Batch([Torrent("n_entries above cap", 65, 2, table=[(i, i % 2, 0, NOW) for i in range(4)], arrived=[1])])
    b.want()["n_entries"][0] = 3  # from the table's 4, one arrived
    b.arrays["n_entries"][0] = 9
    return b


def check_refusals(backend):
    """Mismatches: every invalid call is KRK_EINVAL and leaves state and outputs as they were."""
    b = Batch([random_torrent(9, 65, 3, 0, 3, salt=1), Torrent("lists", 65, 3, table=[(1, 1, 0, NOW)], cap=4, arrived=[1, 2],
               gone=[0, 1], marks=[(1, 1, UNSENT)], holds=[(1, 0), (2, 0), (0, 1)], records=[(3, 2)], picks=[[1], [], []])],
              label="refusals")
    structs, tables, keep = type(b.structs)(), type(b.tables)(), []

    def field(k, j, name, v):
        return lambda a: setattr(a[k][j], name, v)

    def elem(name, j, v):  # word j of torrent 1's list
        def change(a):
            keep.append(b.lists[name].copy())
            keep[-1][b.offs[1][name] * WIDTH[name] + j] = v
            a[6 + LISTS.index(name)] = keep[-1].ctypes.data
        return change

    def arg(k, v):
        return lambda a: a.__setitem__(k, v)

    calls = [("n_pieces 2^32", field(0, 1, "n_pieces", 1 << 32)), ("unknown flag bit", field(0, 0, "flags", 0x200)),
             ("cap above the maximum", field(1, 1, "cap", CAP + 1)), ("reserved", field(1, 0, "reserved", 1)),
             ("arrived equal", elem("arrived", 1, 1)), ("arrived = n_pieces", elem("arrived", 1, 65)),
             ("gone descends", elem("gone", 0, 2)), ("gone = n_peers", elem("gone", 1, 3)),
             ("mark status expired", elem("marks", 2, EXPIRED)), ("mark status 0", elem("marks", 2, 0)),
             ("mark peer", elem("marks", 1, 3)), ("holds descend in a peer", elem("holds", 2, 0)),
             ("holds descend by peer", elem("holds", 5, 0)), ("hold piece", elem("holds", 0, 65)),
             ("record peer", elem("records", 1, 3)), ("record piece", elem("records", 0, 65)),
             ("now < 0", arg(13, -1)), ("timeout < 0", arg(14, -1)), ("now + timeout overflows", arg(14, (1 << 63) - 1)),
             ("limit 0", arg(15, 0)), ("limit 17", arg(15, 17)), ("picks without n_picked", arg(12, None)),
             ("failed without n_failed", arg(18, None))]
    calls += [(f"NULL argument {k}", arg(k, None)) for k in (0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 16, 19)]
    bad = []
    for label, change in calls:
        C.memmove(structs, b.structs, C.sizeof(structs))
        C.memmove(tables, b.tables, C.sizeof(tables))
        rc, got = backend.run(b, change=lambda a: (a.__setitem__(slice(0, 2), [structs, tables]), change(a)))
        bad += [f"{label}: rc {rc}"] * (rc != _capi.KRK_EINVAL) + [f"{label}: {m}" for m in compare(b, got, want=b.arrays)]
    return bad
