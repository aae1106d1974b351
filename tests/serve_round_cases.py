"""Serve rounds (serve_round.hip, serve_round_math.hpp): the cases tests/test_serve_round_cpu.py
(the host form) and tests/test_gpu_serve_round.py (the device form) share.  A helper module, not a
test file.  Shapes come from krk_serve_round_geometry; a torrent's expectation is
tests/serve_round_ref.py, never the library.  Every output and `sent` is prefilled with 0xA5 and
has a margin, the rows hold noise (tail bits and blocked rows included), a dummy torrent and three
unused requests lead every batch so that no array of a case starts at 0, and every whole buffer is
compared: the complete bits array, sent and the ten outputs."""
import ctypes as C
import functools

import numpy as np

from kraken_amd import _capi
from kraken_amd import device as D
from kraken_amd._capi import check, lib
from tests import serve_round_ref as R

SEED, MARGIN, NOW = 20261128, 8, 77
CHUNK, TILE = D.serve_round_geometry()
N_REQS = (0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, TILE - 1, TILE)
NS, SLOTS, TOKEN_SIZES = (0, 1, 63, 64, 65, 130), (1, 2, 10, 70), (0, 1, 1000)
OUTPUTS = ("bits", "sent") + D.ServeOutputs.NAMES


def words(bools):
    return np.packbits(np.asarray(bools, dtype=bool), bitorder="little").view(np.uint64)


class T:
    """One torrent of a case: n pieces of 10 bytes (the last one 7 when not `exact`), `slots` peer
    slots, slots 63 and 64 (or the last of fewer than 64, never the only one) dead.  have and the
    peers' rows are 64 W random bools; reqs is given or n_reqs random requests, most of them good."""

    def __init__(self, n, slots, n_reqs=0, exact=True, reqs=None, length=None, piece_length=10, have=0.7, dead=None, salt=0):
        rng = np.random.default_rng([SEED, n, slots, n_reqs, salt])
        L = 64 * ((n + 63) // 64)
        self.n, self.slots, self.piece_length = n, slots, piece_length
        self.length = (max(piece_length * n - (0 if exact else 3), 0) if length is None else length)
        self.have = (rng.random(L) < have).tolist()
        self.rows = {p: (rng.random(L) < 0.3).tolist() for p in range(slots)}
        dead = ((63, 64) if slots > 64 else (slots - 1,) if slots > 1 else ()) if dead is None else dead
        self.live = [p not in dead for p in range(slots)]
        if reqs is None:
            reqs = []
            for _ in range(n_reqs):
                i = int(rng.choice([int(rng.integers(0, max(n, 1))), -1, n, n + 5], p=[0.85, 0.05, 0.05, 0.05]))
                good = R.plen(i, n, self.length, piece_length)
                ln = int(rng.choice([good, good - 1, 0, piece_length], p=[0.85, 0.05, 0.05, 0.05]))
                reqs.append((int(rng.integers(0, slots)), i, int(rng.random() < 0.05), ln))
        self.reqs = reqs


def plan(ts):
    """The layout, a dummy torrent first: (batch, serve, the two struct arrays without the dummy,
    bits, live, sent)."""
    ts = [T(3, 1)] + list(ts)
    batch = D.RequestBatch([t.n for t in ts], [t.slots for t in ts])
    live_off = np.cumsum([1] + [(t.slots + 63) // 64 for t in ts])  # one unused word leads
    serve = D.ServeBatch(batch, [t.length for t in ts], [t.piece_length for t in ts], live_off[:-1])
    serve.plan({j: t.reqs if j else [(0, 0, 0, 0)] * 3 for j, t in enumerate(ts)})  # the dummy's three are never read
    structs = [(type(a[0]) * (len(ts) - 1)).from_buffer(a, C.sizeof(a[0])) for a in (batch.structs, serve.structs)]
    bits = np.random.default_rng([SEED, len(ts)]).integers(1 << 63, size=batch.total_words + MARGIN, dtype=np.uint64)
    live = np.zeros(int(live_off[-1]), dtype=np.uint64)
    for j, t in enumerate(ts):
        live[int(live_off[j]):int(live_off[j + 1])] = words(t.live + [False] * (-t.slots % 64))
        if t.n:
            batch.rows(bits, j)[0] = words(t.have)
            for p in range(t.slots):
                batch.rows(bits, j)[1 + 2 * p] = words(t.rows[p])
    sent = np.frombuffer(b"\xA5" * (8 * (batch.total_peers + MARGIN)), dtype=np.int64).copy()
    return batch, serve, structs, bits, live, sent


def want(ts, token_size):
    """Every buffer of OUTPUTS after the call."""
    batch, serve, _, bits, _, sent = plan(ts)
    w = {name: np.frombuffer(b"\xA5" * ((k + MARGIN) * np.dtype(dt).itemsize), dtype=dt).copy()
         for name, dt, k in zip(D.ServeOutputs.NAMES, D.ServeOutputs.DTYPES, serve.sizes)}
    w["bits"], w["sent"] = bits, sent
    for j, t in enumerate(ts):
        rows, touched = {p: list(r) for p, r in t.rows.items()}, {}
        out, received, n_sent, totals = R.round_torrent(t.have, rows, t.live, t.n, t.length, t.piece_length, t.reqs, NOW, token_size, touched)
        at, pat = serve.req_off[j + 1], int(batch.peer_off[j + 1])
        for r, o in enumerate(out):
            for name, v in zip(("status", "file_off", "len", "send_off", "token_off")[:5 if token_size else 4], o):
                w[name][at + r] = v
        for p in range(t.slots):
            w["n_received"][pat + p], w["n_sent"][pat + p] = received.get(p, 0), n_sent.get(p, 0)
            w["sent"][pat + p] = touched.get(p, w["sent"][pat + p])
            if t.n:
                batch.rows(bits, j + 1)[1 + 2 * p] = words(rows[p])
        for name, v in zip(("n_ok", "bytes", "tokens")[:3 if token_size else 2], totals):
            w[name][j] = v
    return w


def run(ts, dev=False, token_size=0, pinned=False, now=NOW, change=None):
    """(rc, every array after the call): the host form over numpy arrays, or the device form over uploads."""
    batch, serve, structs, bits, live, sent = plan(ts)
    head = [*structs, len(ts)]
    if not dev:
        out = [np.frombuffer(b"\xA5" * ((k + MARGIN) * np.dtype(dt).itemsize), dtype=dt).copy()
               for dt, k in zip(D.ServeOutputs.DTYPES, serve.sizes)]
        args = head + [bits.ctypes.data, live.ctypes.data, serve.requests.ctypes.data, now, token_size,
                       *D._serve_args([a.ctypes.data for a in out], sent.ctypes.data)]
        change and change(args)
        return lib.krk_serve_round(*args), dict(zip(OUTPUTS, [bits, sent] + out))
    bufs = [D.DeviceBuffer(a.nbytes) for a in (bits, sent)]
    for b, a in zip(bufs, (bits, sent)):
        b.from_host(a)
    out = D.ServeOutputs(serve, pinned=pinned, margin=MARGIN)
    out.fill(0xA5)
    args = head + [bufs[0].ptr, live.ctypes.data, serve.requests.ctypes.data, now, token_size,
                   *D._serve_args([getattr(out, n).ptr for n in out.NAMES], bufs[1].ptr)]
    change and change(args)
    rc = lib.krk_serve_round_dev(*args, None)
    check(lib.krk_stream_sync(None))
    return rc, dict(zip(OUTPUTS, (bufs[0].to_host(np.uint64, bits.size), bufs[1].to_host(np.int64, sent.size)) + out.to_host()))


def mismatches(label, rc, got, w):
    """What differs between one call's whole buffers and `w`, as text."""
    bad = [f"{label}: rc {rc}: {lib.krk_last_error()}"] * (rc != 0)
    for name in OUTPUTS:
        if got[name].tobytes() != w[name].tobytes():
            k = int(np.flatnonzero(got[name] != w[name])[0])
            bad.append(f"{label}: {name}[{k}] is {got[name][k]:#x}, want {w[name][k]:#x} ({int((got[name] != w[name]).sum())} differ)")
    return bad


def check_case(ts, token_size, dev, pinned=False):
    rc, got = run(ts, dev, token_size, pinned)
    return mismatches(f"token_size {token_size}", rc, got, want(ts, token_size))


@functools.lru_cache(maxsize=None)
def cases():
    """{label: (torrents, token_size)}: one property a case."""
    out = {}
    for k, q in enumerate(N_REQS):  # every list length over every N, the slot counts and both length laws in turn
        out[f"n_reqs={q}"] = ([T(n, SLOTS[(j + k) % 4], q, exact=bool((j + k) % 2), salt=k) for j, n in enumerate(NS)], TOKEN_SIZES[k % 3])
    for k, s in enumerate(SLOTS):
        out[f"slots={s}"] = ([T(n, s, 3 * CHUNK + 7, exact=bool(j % 2), salt=k) for j, n in enumerate(NS)], TOKEN_SIZES[k % 3])
    for k, b in enumerate((1, 3, 70)):  # an empty torrent in the middle
        out[f"batch of {b}"] = ([T(NS[j % 6], SLOTS[j % 4], 0 if j == b // 2 else 40 + j, exact=bool(j % 2), salt=j) for j in range(b)], TOKEN_SIZES[k])
    out["every request refused"] = ([T(65, 10, CHUNK + 1, have=0.0), T(65, 2, 65, dead=(0, 1), have=1.0)], 1)
    out["every piece to every peer"] = ([T(130, 2, reqs=[(p, i, 0, 10) for i in range(130) for p in (0, 1)], have=1.0, dead=())], 1000)
    return out


def hand(dev):
    """Mismatches of three small torrents against values worked out by hand: 3 pieces of 100, 100
    and 50 bytes with piece 1 missing and slot 2 gone, 2 pieces of 2^31 and 5 bytes, and pieces 63,
    64 and 65 of 66 asked by one peer (two words, two bits in the second)."""
    a = T(3, 3, length=250, piece_length=100, dead=(2,),
          reqs=[(0, 2, 0, 100), (0, 2, 0, 50), (0, 0, 1, 100), (1, -1, 0, 0), (1, -1, 0, 5), (1, 3, 0, 0), (1, 3, 0, 100),
                (1, 1, 0, 100), (2, 0, 0, 100), (1, 0, 0, 100), (0, 0, 0, 100), (0, 0, 0, 100), (0, 0, 0, 100)])
    a.have, a.rows = [True, False, True] + [True] * 61, {p: [False] * 3 + [True] * 61 for p in range(3)}  # the tails set
    b = T(2, 1, length=(1 << 31) + 5, piece_length=1 << 31, reqs=[(0, 0, 0, (1 << 31) - 1), (0, 1, 0, 5)])
    b.have, b.rows = [True] * 64, {0: [False] * 64}
    c = T(66, 1, reqs=[(0, 64, 0, 10), (0, 63, 0, 10), (0, 65, 0, 10)], have=1.0)
    c.rows = {0: [False] * 128}
    bad = []
    for ts_, by_hand in ((0, ([0] * 13, [0] * 2, [0, 0], [0, 0])), (64, ([0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 18, 30, 42], [0, 0], [54, 1], [54, 1]))):
        batch, serve = plan([a, b, c])[:2]
        _, got = run([a, b, c], dev, ts_)
        ra, rb, pa = serve.req_off[1], serve.req_off[2], int(batch.peer_off[1])
        tail = ((1 << 64) - 1) ^ 7
        mine = {"status": got["status"][ra:rb + 2].tolist(), "file_off": got["file_off"][ra:rb + 2].tolist(),
                "len": got["len"][ra:rb + 2].tolist(), "send_off": got["send_off"][ra:rb + 2].tolist(),
                "n_received": got["n_received"][pa:pa + 4].tolist(), "n_sent": got["n_sent"][pa:pa + 4].tolist(),
                "sent": got["sent"][pa:pa + 2].tolist(), "n_ok": got["n_ok"][:2].tolist(), "bytes": got["bytes"][:2].tolist(),
                "rows": [int(batch.rows(got["bits"], 1)[1 + 2 * p][0]) for p in range(3)] + [int(batch.rows(got["bits"], 2)[1][0])],
                "edge": batch.rows(got["bits"], 3)[1].tolist() + got["send_off"][rb + 2:rb + 5].tolist()}
        want_ = {"status": [1, 0, 1, 2, 1, 2, 1, 3, 4, 0, 0, 0, 0, 1, 0], "file_off": [0, 200] + [0] * 7 + [0, 0, 0, 0, 0, 1 << 31],
                 "len": [0, 50] + [0] * 7 + [100] * 4 + [0, 5], "send_off": [0] * 9 + [50, 150, 250, 350, 0, 0],
                 "n_received": [6, 6, 1, 2], "n_sent": [4, 1, 0, 1], "sent": [NOW, NOW], "n_ok": [5, 1], "bytes": [450, 5],
                 "rows": [tail | 5, tail | 1, tail, 2], "edge": [1 << 63, 3, 0, 10, 20]}
        if ts_:
            mine.update(token_off=got["token_off"][ra:rb + 2].tolist(), tokens=got["tokens"][:2].tolist())
            want_.update(token_off=by_hand[0] + by_hand[1], tokens=by_hand[2])
        bad += [f"token_size {ts_}: {k}: {mine[k]!r}, by hand {v!r}" for k, v in want_.items() if mine[k] != v]
    return bad


def refusals(dev=False):
    """Mismatches: every invalid call is KRK_EINVAL and leaves the rows, sent and the outputs as they were."""
    ts = [T(65, 10, 5), T(10, 2, 3, exact=False)]
    p = plan(ts)
    before = {**{n: np.frombuffer(b"\xA5" * a.nbytes, dtype=a.dtype) for n, a in want(ts, 1).items()}, "bits": p[3], "sent": p[5]}

    def field(k, j, name, v):  # argument k: a copy of the structs with one field changed
        def change(a):
            a[k] = type(a[k]).from_buffer_copy(a[k])
            setattr(a[k][j], name, v)
        return change

    reqs = p[1].requests.copy()
    reqs["peer"][p[1].req_off[2]] = 2  # the first request of the second torrent names a slot it does not have

    def many(a):  # 2^20 copies of the first torrent with a full list: 2^32 requests, refused before any is read
        full = type(a[1]).from_buffer_copy(a[1])
        full[0].n_reqs = TILE
        tiled = [np.tile(np.frombuffer(x, dtype=np.uint8)[:C.sizeof(x[0])], (1 << 32) // TILE) for x in (a[0], full)]
        a[:3] = [C.cast(y.ctypes.data, C.POINTER(type(x[0]))) for x, y in zip((a[0], full), tiled)] + [(1 << 32) // TILE]
        keep.extend(tiled)

    keep = []
    calls = [("2^32 requests in one call", many), ("n_reqs above the maximum", field(1, 0, "n_reqs", TILE + 1)), ("negative length", field(1, 0, "length", -1)),
             ("inconsistent length", field(1, 1, "length", 101)), ("piece_length 0", field(1, 0, "piece_length", 0)),
             ("negative piece_length", field(1, 1, "piece_length", -10)), ("n_pieces off by one", field(0, 0, "n_pieces", 66)),
             ("reserved", field(1, 0, "reserved", 1)), ("negative now", lambda a: a.__setitem__(6, -1))]
    calls += [(f"{name} 2^48", field(k, 1, name, 1 << 48)) for k, name in ((0, "bits_off"), (0, "peer_off"), (1, "live_off"), (1, "req_off"))]
    calls += [(f"NULL argument {k}", lambda a, k=k: a.__setitem__(k, None)) for k in (0, 1, 3, 4, 5, *range(8, 19))]
    bad, texts = [], {"piece_length 0": b"piece length must be positive", "2^32 requests in one call": b"(2^32 or more)"}
    for label, change in calls + [("a peer that is no slot", lambda a: a.__setitem__(5, reqs.ctypes.data))]:
        rc, got = run(ts, dev, 1, change=change)
        bad += [f"{label}: rc {rc}"] * (rc != _capi.KRK_EINVAL) + mismatches(label, 0, got, before)
        if texts.get(label, b"") not in lib.krk_last_error():
            bad.append(f"{label}: {lib.krk_last_error()}")
    return bad
