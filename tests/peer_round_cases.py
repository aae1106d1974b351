"""Peer rounds (peer_round.hip, peer_round_math.hpp): the cases tests/test_peer_round_cpu.py (the
host form) and tests/test_gpu_peer_round.py (the device form) share.  A helper module, not a test
file.  Shapes come from krk_peer_round_geometry; a torrent's expectation is tests/peer_round_ref.py,
never the library.  No array starts at offset 0, the outputs are prefilled with 0xA5 and the
blocked rows with noise: every whole buffer is compared, the rows and the five outputs."""
import ctypes as C
import functools

import numpy as np

from kraken_amd import _capi
from kraken_amd._capi import check, lib
from kraken_amd.device import PE_JOIN
from tests import peer_round_ref as R

SEED, SPARE = 20261126, 4
_c, _s = C.c_uint64(), C.c_uint64()
check(lib.krk_peer_round_geometry(C.byref(_c), C.byref(_s)))
UNIT_CAP, S = int(_c.value), 64 * int(_s.value)  # S: the words a wave covers in a step
NS, PS = (0, 1, 63, 64, 65, 64 * S - 1, 64 * S, 64 * S + 1, 4097), (0, 1, 3, 4, 5, 300)
OUTPUTS = ("bits", "remaining", "tflags", "held", "wanted", "status")
HAND = bytes.fromhex("000000000000000A 0000000000000201")  # bits {0, 9} of 10 pieces


def words(bools):
    return np.packbits(np.asarray(bools, dtype=bool), bitorder="little").view(np.uint64)


def bools(n, *on, fill=False):
    """64 W bools (n pieces and the tail): `fill` everywhere below n, and the bits of `on` flipped."""
    b = [fill] * n + [False] * (-n % 64)
    for i in on:
        b[i] = not b[i]
    return b


class Torrent:
    """have, rows[p]: 64 W bools; live: a bool a slot; joins: [(slot, wire)]; fulls: [slot]."""

    def __init__(self, label, n, have, rows, live=None, joins=(), fulls=(), threshold=0, flags=0):
        self.label, self.n, self.have, self.rows, self.P = label, n, have, rows, len(rows)
        self.live, self.joins, self.fulls = [True] * self.P if live is None else live, list(joins), list(fulls)
        self.threshold, self.flags = threshold, flags


def random_torrent(n, P, salt=0):
    rng = np.random.default_rng([SEED, n, P, salt])
    L = 64 * ((n + 63) // 64)
    draw = lambda p: (rng.random(L) < p).tolist()  # noqa: E731  (tail bits included)
    have = draw(rng.choice([0.5, 0.98, 1.0]))
    slots = sorted({0, P - 1, *rng.choice(P, size=min(P, 6), replace=False).tolist()}) if P else []
    joins = [(p, R.marshal(draw(0.5), n)) for p in slots]
    if len(joins) > 2:  # one of them malformed: the row keeps its noise
        joins[1] = (joins[1][0], joins[1][1] + b"\0")
    return Torrent(f"random n={n} P={P} salt={salt}", n, have, [draw(0.6) for _ in range(P)], (rng.random(P) < 0.7).tolist(),
                   joins, slots[1::2], max(0, n - sum(have[:n]) - salt % 2), salt // 2 % 2)


class Batch:
    """Torrents packed back to back from non-zero offsets; the wire spans back to back from byte wire_at."""

    def __init__(self, torrents, wire_at=1, label=None):
        self.torrents, self.label = list(torrents), label or " | ".join(t.label for t in torrents)
        k = len(self.torrents)
        self.structs, self.peers = (_capi.krk_request_torrent * max(k, 1))(), (_capi.krk_peer_torrent * max(k, 1))()
        at = {"w": 3, "p": 5, "l": 2, "j": 2, "f": 2}
        joins, fulls, wire, self.offs = [(9, 9, 9, 9)] * 2, [9] * 2, bytearray(b"\xEE" * wire_at), []
        for j, t in enumerate(self.torrents):
            self.offs.append(dict(at))
            W = (t.n + 63) // 64
            self.structs[j] = _capi.krk_request_torrent(t.n, t.P, 0x7777, 77 * j, at["w"], at["p"], 1 << 60)  # flags, seed, piece_off: not read
            self.peers[j] = _capi.krk_peer_torrent(t.threshold, t.flags, at["l"], at["j"], at["f"], len(t.joins), len(t.fulls))
            for p, span in t.joins:
                joins.append((p, 0, len(wire), len(span)))
                wire += span
            fulls += t.fulls
            at = {"w": at["w"] + (1 + 2 * t.P) * W, "p": at["p"] + t.P, "l": at["l"] + (t.P + 63) // 64,
                  "j": at["j"] + len(t.joins), "f": at["f"] + len(t.fulls)}
        rng = np.random.default_rng([SEED, k, at["w"]])
        a = self.arrays = {name: np.full(size + SPARE, 0xA5A5A5A5, dtype=np.uint32) for name, size in
                           (("remaining", k), ("tflags", k), ("held", at["p"]), ("wanted", at["p"]), ("status", at["p"]))}
        a["bits"] = rng.integers(1 << 63, size=at["w"] + SPARE, dtype=np.uint64)  # noise where the blocked rows are
        a["wire"] = np.frombuffer(bytes(wire + b"\xEE" * 9), dtype=np.uint8)
        self.live = np.full(at["l"] + SPARE, 0xFFFF0000FFFF0000, dtype=np.uint64)
        for t, o in zip(self.torrents, self.offs):
            rows = self.rows(a["bits"], t, o)
            for i, r in enumerate([t.have] + t.rows):
                rows[max(2 * i - 1, 0)] = words(r)
            self.live[o["l"]:o["l"] + (t.P + 63) // 64] = words(t.live + [False] * (-t.P % 64))
        self.joins, self.fulls = np.array(joins, dtype=PE_JOIN), np.asarray(fulls, dtype=np.uint32)

    @staticmethod
    def rows(bits, t, o):
        W = (t.n + 63) // 64
        return bits[o["w"]:o["w"] + (1 + 2 * t.P) * W].reshape(1 + 2 * t.P, W)

    @functools.lru_cache(None)
    def want(self):
        """Every buffer of OUTPUTS after the call."""
        w = {name: self.arrays[name].copy() for name in OUTPUTS}
        for j, (t, o) in enumerate(zip(self.torrents, self.offs)):
            rows, w["remaining"][j], w["tflags"][j], held, wanted, status = R.round_torrent(
                t.n, t.have, t.rows, t.live, t.joins, t.fulls, t.threshold, t.flags)
            for p, r in enumerate(rows):
                self.rows(w["bits"], t, o)[1 + 2 * p] = words(r)
            for name, v in (("held", held), ("wanted", wanted), ("status", status)):
                w[name][o["p"]:o["p"] + t.P] = v
        return w

    def args(self, ptr):
        """The argument list of a round call (without the stream); ptr: {array name: address}."""
        return [self.structs, self.peers, len(self.torrents), ptr["bits"], self.live.ctypes.data, self.joins.ctypes.data,
                self.fulls.ctypes.data, ptr["wire"], *(ptr[name] for name in OUTPUTS[1:])]


def run(b, dev=False, pinned=False, change=None):
    """(rc, every array after the call): the host form over copies, or the device form over uploads."""
    from kraken_amd import device as D
    if not dev:
        got = {k: v.copy() for k, v in b.arrays.items()}
        args = b.args({k: v.ctypes.data for k, v in got.items()})
        change and change(args)
        return lib.krk_peer_round(*args), got
    bufs = {k: D.PinnedArray((v.nbytes,), np.uint8) if pinned and k != "bits" else D.DeviceBuffer(v.nbytes)
            for k, v in b.arrays.items()}
    for k, v in b.arrays.items():
        raw = v.view(np.uint8).reshape(-1)
        bufs[k].a.__setitem__(slice(None), raw) if isinstance(bufs[k], D.PinnedArray) else bufs[k].from_host(raw)
    args = b.args({k: v.ptr for k, v in bufs.items()})
    change and change(args)
    rc = lib.krk_peer_round_dev(*args, None)
    check(lib.krk_stream_sync(None))
    return rc, {k: (bufs[k].a.copy() if isinstance(bufs[k], D.PinnedArray) else bufs[k].to_host(np.uint8, v.nbytes)).view(v.dtype)
                for k, v in b.arrays.items()}


def mismatches(b, rc, got, want=None):
    """What differs between one call's whole buffers and the reference's (or `want`), as text."""
    bad, want = [f"{b.label}: rc {rc}: {lib.krk_last_error()}"] * (rc != 0), want or b.want()
    for name in OUTPUTS:
        w, g = want[name], got[name]
        if g.tobytes() != w.tobytes():
            k = int(np.flatnonzero(g != w)[0])
            bad.append(f"{b.label}: {name}[{k}] is {g[k]:#x}, want {w[k]:#x} ({int((g != w).sum())} differ)")
    return bad


@functools.lru_cache(None)
def matrix():
    """N x P, one torrent a batch (built once), and one batch with more rows than the unit cap."""
    many = Batch([random_torrent(1 + j % 65, 300, salt=j) for j in range(UNIT_CAP // 301 + 1)], label="above the unit cap")
    return [Batch([random_torrent(n, P, salt=k)], wire_at=k % 8) for k, (n, P) in enumerate((n, P) for n in NS for P in PS)] + [many]


@functools.lru_cache(None)
def batch(k):
    """k torrents that mix the matrix's shapes, a zero-piece and a zero-peer torrent in the middle."""
    shape = lambda j: (0 if k >= 3 and j == k // 2 else NS[(3 * j + 1) % 9], 0 if k >= 3 and j == k // 2 + 1 else PS[1 + j % 4])  # noqa: E731
    return Batch([random_torrent(*shape(j), salt=100 + j) for j in range(k)], wire_at=3, label=f"batch of {k}")


def named():
    """[(Batch, {output: torrent 0's values worked out by hand})]: one property a case."""
    out = []
    J, B, F, PC, CL, NO = R.JOINED, R.BAD_BITFIELD, R.SET_FULL, R.PEER_COMPLETE, R.CLOSE, R.NOTIFY
    full, part, wire65 = bools(65, fill=True), bools(65, 3, 64), R.marshal(bools(65, 0, 64)[:65])

    def add(hand, label, *a, wire_at=1, **kw):
        out.append((Batch([Torrent(label, *a, **kw)], wire_at), hand))

    for at in range(8):  # two spans back to back from every byte offset; the hand-worked vector first
        add({"held": [2, 10], "wanted": [1, 9], "status": [J, J | PC]}, f"the hand-worked vector at byte {at}", 10, bools(10, 9),
            [bools(10, 5)] * 2, joins=[(0, HAND), (1, R.marshal([True] * 10))], wire_at=at)
    add({"held": [65], "status": [J | PC]}, "a last word with every tail bit set comes out cleared", 65, bools(65), [bools(65)],
        joins=[(0, R.marshal([True] * 128, 65))])
    bad = [b"", wire65[:7], wire65[:8], R.marshal(bools(65)[:65], 64), R.marshal(bools(65)[:65], 66),
           R.marshal(bools(65)[:65], 1 << 63), wire65 + b"\1", wire65[:-1]]
    add({"held": [3] * 8 + [2], "status": [B] * 8 + [J]}, "malformed spans leave their rows alone, the well-formed one after them lands",
        65, bools(65), [bools(65, 1, 2, 64, 100)] * 9, joins=list(enumerate(bad + [wire65])))
    add({"held": [65, 65, 2, 0], "status": [J | F | PC, F | PC, J, 0]}, "a join and a full for one peer, a full on a zero row, a join alone",
        65, bools(65), [part, bools(65), part, bools(65)], joins=[(0, wire65), (2, wire65)], fulls=[0, 1])
    add({"remaining": [63], "tflags": [0], "held": [2], "wanted": [1], "status": [0]}, "empty lists: derive only", 65, bools(65, 3, 7), [part])
    add({"remaining": [0], "tflags": [R.TORRENT_COMPLETE | R.ENDGAME], "status": [PC | CL, NO, 0, 0]},
        "a complete torrent: close the full, notify the partial, nothing for the slots that are not live", 65, full,
        [full, part, full, part], live=[True, True, False, False])
    for extra, flags, want in ((0, 0, R.ENDGAME), (1, 0, 0), (0, R.DISABLE_ENDGAME, 0)):
        add({"remaining": [4 + extra], "tflags": [want]}, f"remaining = threshold + {extra}, flags {flags}", 65,
            bools(65, *range(4 + extra), fill=True), [part], threshold=4, flags=flags)
    add({"remaining": [0], "held": [1], "wanted": [0], "status": [NO]}, "tail bits set in have and in a row no join wrote are not counted",
        65, bools(65, *range(65, 128), fill=True), [bools(65, 64, *range(65, 128))])
    add({"remaining": [0], "tflags": [R.TORRENT_COMPLETE | R.ENDGAME], "held": [0, 0], "status": [J | PC | CL, 0]},
        "a zero-piece torrent is complete and so is its live peer", 0, [], [[], []], live=[True, False], joins=[(0, R.marshal([]))])
    return out


def hand_mismatches(b, got, hand):
    o, t = b.offs[0], b.torrents[0]
    mine = {name: got[name][:1].tolist() if name in ("remaining", "tflags") else got[name][o["p"]:o["p"] + t.P].tolist()
            for name in hand}
    return [f"{b.label}: {k} is {mine[k]}, by hand {v}" for k, v in hand.items() if mine[k] != v]


def refusals(dev=False):
    """Mismatches: every invalid call is KRK_EINVAL and leaves the rows and the outputs as they were."""
    b = Batch([random_torrent(65, 3, salt=1), Torrent("lists", 65, bools(65), [bools(65, 1)] * 4, joins=[(1, HAND), (3, HAND)], fulls=[0, 2])],
              label="refusals")
    structs, peers, keep = type(b.structs)(), type(b.peers)(), []

    def field(k, j, name, v):
        return lambda a: setattr(a[k][j], name, v)

    def elem(k, arr, j, name, v):  # element j of torrent 1's list
        def change(a):
            keep.append(arr.copy())
            if name:
                keep[-1][j][name] = v
            else:
                keep[-1][j] = v
            a[k] = keep[-1].ctypes.data
        return change

    jo, fo = b.offs[1]["j"], b.offs[1]["f"]
    calls = [("n_pieces 2^32", field(0, 1, "n_pieces", 1 << 32)), ("unknown flag bit", field(1, 0, "flags", 2)),
             ("joins equal", elem(5, b.joins, jo + 1, "peer", 1)), ("joins descend", elem(5, b.joins, jo, "peer", 3)),
             ("join peer = n_peers", elem(5, b.joins, jo + 1, "peer", 4)), ("join reserved", elem(5, b.joins, jo, "reserved", 1)),
             ("wire span overflows", elem(5, b.joins, jo, "wire_off", (1 << 64) - 8)),
             ("fulls equal", elem(6, b.fulls, fo + 1, None, 0)), ("full peer = n_peers", elem(6, b.fulls, fo + 1, None, 4))]
    calls += [(f"NULL argument {k}", lambda a, k=k: a.__setitem__(k, None)) for k in (0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)]
    bad = []
    for label, change in calls:
        C.memmove(structs, b.structs, C.sizeof(structs))
        C.memmove(peers, b.peers, C.sizeof(peers))
        rc, got = run(b, dev, change=lambda a: (a.__setitem__(slice(0, 2), [structs, peers]), change(a)))
        bad += [f"{label}: rc {rc}"] * (rc != _capi.KRK_EINVAL) + [f"{label}: {m}" for m in mismatches(b, 0, got, want=b.arrays)]
    return bad
