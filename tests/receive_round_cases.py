"""Receive rounds (receive_round.hip, receive_round_math.hpp): the cases
tests/test_receive_round_cpu.py (the host form) and tests/test_gpu_receive_round.py (the device
form) share.  A helper module, not a test file.  A torrent's expectation is
tests/receive_round_ref.py, never the library.  Every output and `received` is prefilled with 0xA5
and has a margin, the rows hold noise (the have row's tail bits and the peers' rows included), a
dummy torrent, three unused payloads and one unused expected sum lead every batch so that no array
of a case starts at 0, and every whole buffer is compared: the complete bits array, received and
the twelve outputs."""
import ctypes as C
import functools

import numpy as np

from kraken_amd import _capi
from kraken_amd import device as D
from kraken_amd._capi import check, lib
from tests import receive_round_ref as R

SEED, MARGIN, NOW = 20261129, 8, 77
CHUNK, TILE = D.receive_round_geometry()
N_PAYS = (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, TILE - 1, TILE)
NS, SLOTS = (0, 1, 63, 64, 65, 129), (0, 1, 64, 65, 300)
OUTPUTS = ("bits", "received") + D.ReceiveOutputs.NAMES


def words(bools):
    return np.packbits(np.asarray(bools, dtype=bool), bitorder="little").view(np.uint64)


class T:
    """One torrent of a case: n pieces of 10 bytes (the last one 7 when not `exact`), `slots` peer
    slots, piece i's expected sum 1000 + i.  have is 64 W random bools, the tail included; pays is
    given as (slot, index, offset, length, sum) or n_pays random payloads, most of them full-shaped
    and two in three of those good-summed, one sender in ten gone (all with no slot)."""

    def __init__(self, n, slots, n_pays=0, exact=True, pays=None, length=None, piece_length=10, have=0.4, salt=0):
        rng = np.random.default_rng([SEED, n, slots, n_pays, salt])
        self.n, self.slots, self.piece_length = n, slots, piece_length
        self.length = (max(piece_length * n - (0 if exact else 3), 0) if length is None else length)
        self.have = (rng.random(64 * ((n + 63) // 64)) < have).tolist()
        self.expected = [1000 + i for i in range(n)]
        if pays is None:
            pays = []
            for _ in range(n_pays):
                i = int(rng.choice([int(rng.integers(0, max(n, 1))), -1, n, n + 5], p=[0.91, 0.03, 0.03, 0.03]))
                good = R.plen(i, n, self.length, piece_length)
                ln = int(rng.choice([good, good - 1, good + 1, 0], p=[0.91, 0.03, 0.03, 0.03]))
                p = int(rng.integers(0, slots)) if slots and rng.random() < 0.9 else R.NONE
                pays.append((p, i, int(rng.random() < 0.03), ln, 1000 + i + int(rng.random() < 0.33)))
        self.pays, self.sums = [q[:4] for q in pays], [q[4] & 0xFFFFFFFF for q in pays]


def plan(ts):
    """The layout, a dummy torrent first: (batch, receive, the two struct arrays without the dummy,
    bits, sums, expected, received)."""
    ts = [T(3, 1)] + list(ts)
    batch = D.RequestBatch([t.n for t in ts], [t.slots for t in ts])
    receive = D.ReceiveBatch(batch, [t.length for t in ts], [t.piece_length for t in ts], 1 + batch.piece_off[:-1])
    receive.plan({j: t.pays if j else [(0, 0, 0, 0)] * 3 for j, t in enumerate(ts)})  # the dummy's three are never read
    structs = [(type(a[0]) * (len(ts) - 1)).from_buffer(a, C.sizeof(a[0])) for a in (batch.structs, receive.structs)]
    bits = np.random.default_rng([SEED, len(ts)]).integers(1 << 63, size=batch.total_words + MARGIN, dtype=np.uint64)
    for j, t in enumerate(ts):
        if t.n:
            batch.rows(bits, j)[0] = words(t.have)
    sums = np.array([0] * 3 + [s for t in ts[1:] for s in t.sums], dtype=np.uint32)
    expected = np.array([0] + [s for t in ts for s in t.expected], dtype=np.uint32)
    received = np.frombuffer(b"\xA5" * (8 * (batch.total_peers + MARGIN)), dtype=np.int64).copy()
    return batch, receive, structs, bits, sums, expected, received


def want(ts):
    """Every buffer of OUTPUTS after the call."""
    batch, receive, _, bits, _, _, received = plan(ts)
    w = {name: np.frombuffer(b"\xA5" * ((k + MARGIN) * np.dtype(dt).itemsize), dtype=dt).copy()
         for name, dt, k in zip(D.ReceiveOutputs.NAMES, D.ReceiveOutputs.DTYPES, receive.sizes)}
    w["bits"], w["received"] = bits, received
    for j, t in enumerate(ts):
        have, touched = list(t.have), {}
        out, arrived, marks, good, dup, totals = R.round_torrent(have, t.n, t.length, t.piece_length, t.pays, t.sums, t.expected, NOW, touched)
        at, pat = receive.pay_off[j + 1], int(batch.peer_off[j + 1])
        for r, (st, off) in enumerate(out):
            w["status"][at + r], w["file_off"][at + r] = st, off
        for k, (i, p) in enumerate(arrived):
            w["arrived"][at + k], w["arrived_from"][at + k] = i, p
        for k, m in enumerate(marks):
            w["marks"][at + k] = m
        for p in range(t.slots):
            w["n_good"][pat + p], w["n_duplicate"][pat + p] = good.get(p, 0), dup.get(p, 0)
            w["received"][pat + p] = touched.get(p, w["received"][pat + p])
        if t.n:
            batch.rows(bits, j + 1)[0] = words(have)
        for name, v in zip(("n_arrived", "n_marks", "n_complete", "bytes", "flags"), (len(arrived), len(marks)) + totals):
            w[name][j] = v
    return w


def run(ts, dev=False, pinned=False, now=NOW, change=None):
    """(rc, every array after the call): the host form over numpy arrays, or the device form over uploads."""
    batch, receive, structs, bits, sums, expected, received = plan(ts)
    head = [*structs, len(ts)]
    if not dev:
        out = [np.frombuffer(b"\xA5" * ((k + MARGIN) * np.dtype(dt).itemsize), dtype=dt).copy()
               for dt, k in zip(D.ReceiveOutputs.DTYPES, receive.sizes)]
        args = head + [bits.ctypes.data, receive.payloads.ctypes.data, sums.ctypes.data, expected.ctypes.data, now,
                       *D._receive_args([a.ctypes.data for a in out], received.ctypes.data)]
        change and change(args)
        return lib.krk_receive_round(*args), dict(zip(OUTPUTS, [bits, received] + out))
    bufs = [D.DeviceBuffer(a.nbytes) for a in (bits, received, sums, expected)]
    for b, a in zip(bufs, (bits, received, sums, expected)):
        b.from_host(a)
    out = D.ReceiveOutputs(receive, pinned=pinned, margin=MARGIN)
    out.fill(0xA5)
    args = head + [bufs[0].ptr, receive.payloads.ctypes.data, bufs[2].ptr, bufs[3].ptr, now,
                   *D._receive_args([getattr(out, n).ptr for n in out.NAMES], bufs[1].ptr)]
    change and change(args)
    rc = lib.krk_receive_round_dev(*args, None)
    check(lib.krk_stream_sync(None))
    return rc, dict(zip(OUTPUTS, (bufs[0].to_host(np.uint64, bits.size), bufs[1].to_host(np.int64, received.size)) + out.to_host()))


def mismatches(label, rc, got, w):
    """What differs between one call's whole buffers and `w`, as text."""
    bad = [f"{label}: rc {rc}: {lib.krk_last_error()}"] * (rc != 0)
    for name in OUTPUTS:
        if got[name].tobytes() != w[name].tobytes():
            k = int(np.flatnonzero(got[name] != w[name])[0])
            bad.append(f"{label}: {name}[{k}] is {got[name][k]}, want {w[name][k]} ({int((got[name] != w[name]).sum())} differ)")
    return bad


def check_case(ts, dev, pinned=False):
    rc, got = run(ts, dev, pinned)
    return mismatches("case", rc, got, want(ts))


@functools.lru_cache(maxsize=None)
def cases():
    """{label: torrents}: one property a case."""
    out = {}
    for k, q in enumerate(N_PAYS):  # every list length over every N, the slot counts and both length laws in turn
        out[f"n_pays={q}"] = [T(n, SLOTS[(j + k) % 5], q, exact=bool((j + k) % 2), salt=k) for j, n in enumerate(NS)]
    for k, s in enumerate(SLOTS):
        out[f"slots={s}"] = [T(n, s, 3 * CHUNK + 7, exact=bool(j % 2), salt=k) for j, n in enumerate(NS)]
    for b in (1, 3, 70):  # several torrents of different shapes, an empty list in the middle
        out[f"batch of {b}"] = [T(NS[j % 6], SLOTS[j % 5], 0 if j == b // 2 else 40 + j, exact=bool(j % 2), salt=j) for j in range(b)]
    g, b = 1007, 1  # piece 7 of 10 from slots 0, 1, 2: its good sum and a bad one
    for name, pat in (("bad-good-good", ((0, 10, b), (1, 10, g), (2, 10, g))), ("good-chunk", ((0, 10, g), (1, 9, g))),
                      ("good-bad", ((0, 10, g), (1, 10, b))), ("all bad", ((0, 10, b), (1, 10, b), (2, 10, b)))):
        out[name] = [T(10, 3, pays=[(p, 7, 0, ln, s) for p, ln, s in pat], have=0.0)]
    out["held before the round"] = [T(10, 3, pays=[(0, 7, 0, 10, g), (1, 7, 0, 10, b)], have=1.0)]
    every = [(i % 65, i, 0, 10, 1000 + i) for i in (*range(128, -1, -1), 5, 64)]  # descending: one word's bits from many threads
    out["every piece in one round"] = [T(129, 65, pays=every, have=0.0), T(129, 65, pays=every[1:-2], have=0.0)]
    out["already complete"] = [T(65, 2, CHUNK + 1, have=1.0), T(0, 2, 5)]
    return out


def hand(dev):
    """Mismatches against values worked out by hand: 3 pieces of 100, 100 and 50 bytes with sums 10,
    11, 12, piece 0 held (and the row's tail set), two slots."""
    pays = [(0, 1, 0, 100, 99), (1, 1, 0, 100, 11), (0, 1, 0, 100, 99), (0, 0, 0, 100, 10), (1, 2, 0, 100, 12),
            (R.NONE, 2, 0, 50, 12), (0, 3, 0, 0, 0), (1, -1, 1, 0, 0), (R.NONE, 1, 1, 100, 11)]
    a = T(3, 2, length=250, piece_length=100, pays=pays)
    a.have, a.expected = [True, False, False] + [True] * 61, [10, 11, 12]
    batch, receive = plan([a])[:2]
    _, got = run([a], dev)
    at, pat = receive.pay_off[1], int(batch.peer_off[1])
    mine = {"status": got["status"][at:at + 9].tolist(), "file_off": got["file_off"][at:at + 9].tolist(),
            "arrived": got["arrived"][at:at + 2].tolist(), "arrived_from": got["arrived_from"][at:at + 2].tolist(),
            "marks": got["marks"][at:at + 2].tolist(), "n_good": got["n_good"][pat:pat + 2].tolist(),
            "n_duplicate": got["n_duplicate"][pat:pat + 2].tolist(), "received": got["received"][pat:pat + 2].tolist(),
            "totals": [int(got[k][0]) for k in ("n_arrived", "n_marks", "n_complete", "bytes", "flags")],
            "have": int(batch.rows(got["bits"], 1)[0][0])}
    by_hand = {"status": [4, 0, 3, 3, 1, 0, 2, 1, 1], "file_off": [0, 100, 0, 0, 0, 200, 0, 0, 0], "arrived": [1, 2],
               "arrived_from": [1, R.NONE], "marks": [(1, 0, 3), (2, 1, 3)], "n_good": [0, 1], "n_duplicate": [2, 0],
               "received": [int.from_bytes(b"\xA5" * 8, "little", signed=True), NOW], "totals": [2, 2, 3, 250, 3],
               "have": (1 << 64) - 1}
    return [f"{k}: {mine[k]!r}, by hand {v!r}" for k, v in by_hand.items() if mine[k] != v]


def refusals(dev=False):
    """Mismatches: every invalid call is KRK_EINVAL and leaves the rows, received and the outputs as they were."""
    ts = [T(65, 10, 5), T(10, 2, 3, exact=False)]
    p = plan(ts)
    before = {**{n: np.frombuffer(b"\xA5" * a.nbytes, dtype=a.dtype) for n, a in want(ts).items()}, "bits": p[3], "received": p[6]}

    def field(k, j, name, v):  # argument k: a copy of the structs with one field changed
        def change(a):
            a[k] = type(a[k]).from_buffer_copy(a[k])
            setattr(a[k][j], name, v)
        return change

    pays = p[1].payloads.copy()
    pays["peer"][p[1].pay_off[2]] = 2  # the first payload of the second torrent names a slot it does not have

    def many(a):  # 2^20 copies of the first torrent with a full list: 2^32 payloads, refused before any is read
        full = type(a[1]).from_buffer_copy(a[1])
        full[0].n_pays = TILE
        tiled = [np.tile(np.frombuffer(x, dtype=np.uint8)[:C.sizeof(x[0])], (1 << 32) // TILE) for x in (a[0], full)]
        a[:3] = [C.cast(y.ctypes.data, C.POINTER(type(x[0]))) for x, y in zip((a[0], full), tiled)] + [(1 << 32) // TILE]
        keep.extend(tiled)

    keep = []
    calls = [("2^32 payloads in one call", many), ("n_pays above the maximum", field(1, 0, "n_pays", TILE + 1)),
             ("more than 2^30 slots", field(0, 0, "n_peers", (1 << 30) + 1)), ("negative length", field(1, 0, "length", -1)),
             ("inconsistent length", field(1, 1, "length", 101)), ("piece_length 0", field(1, 0, "piece_length", 0)),
             ("negative piece_length", field(1, 1, "piece_length", -10)), ("n_pieces off by one", field(0, 0, "n_pieces", 66)),
             ("reserved", field(1, 0, "reserved", 1)), ("negative now", lambda a: a.__setitem__(7, -1)),
             ("a peer that is no slot", lambda a: a.__setitem__(4, pays.ctypes.data))]
    calls += [(f"{name} 2^48", field(k, 1, name, 1 << 48)) for k, name in ((0, "bits_off"), (0, "peer_off"), (1, "sum_off"), (1, "pay_off"))]
    calls += [(f"NULL argument {k}", lambda a, k=k: a.__setitem__(k, None)) for k in (0, 1, 3, 4, 5, 6, *range(8, 21))]
    bad, texts = [], {"piece_length 0": b"piece length must be positive", "2^32 payloads in one call": b"(2^32 or more)"}
    for label, change in calls:
        rc, got = run(ts, dev, change=change)
        bad += [f"{label}: rc {rc}"] * (rc != _capi.KRK_EINVAL) + mismatches(label, 0, got, before)
        if texts.get(label, b"") not in lib.krk_last_error():
            bad.append(f"{label}: {lib.krk_last_error()}")
    return bad
