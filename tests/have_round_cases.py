"""Have rounds (have_round.hip, have_round_math.hpp): the cases tests/test_have_round_cpu.py (the
host form) and tests/test_gpu_have_round.py (the device form) share.  A helper module, not a test
file.  Shapes come from krk_have_round_geometry; a torrent's expectation is tests/have_round_ref.py,
never the library.  Every output is prefilled with 0xA5 and has a margin, the rows beside `have`
hold noise, and every whole buffer is compared: the rows and the nine outputs."""

import numpy as np

from kraken_amd import _capi
from kraken_amd import device as D
from kraken_amd._capi import check, lib
from tests import have_round_ref as R

SEED, MARGIN = 20261127, 8
UNIT_CAP, PASS = D.have_round_geometry()
NS = (0, 1, 10, 63, 64, 65, 127, 128, 64 * PASS - 1, 64 * PASS, 64 * PASS + 1, 2 * 64 * PASS + 1)
EMITS = R.EMIT_STATUS | R.EMIT_WIRE | R.EMIT_MISSING
COMBOS = (R.RESTORE, R.IN_CACHE, R.RESTORE | R.MERGE_AND, R.MERGE_OR, 0)  # each also with the three emits
HAND = bytes.fromhex("000000000000000A 0000000000000201")  # bits {0, 9} of 10 pieces
OUTPUTS = ("bits",) + D.HaveOutputs.NAMES


def words(bools):
    return np.packbits(np.asarray(bools, dtype=bool), bitorder="little").view(np.uint64)


def bools(n, *on, fill=False, tail=False):
    b = [fill] * n + [tail] * (-n % 64)
    for i in on:
        b[i] = not b[i]
    return b


class T:
    """One torrent of a case: row and ok are 64 W bools (random, tail bits included, unless given),
    status the sidecar span (random bytes of 0, 1, 2 and 255, n of them, unless given)."""

    def __init__(self, n, flags, row=None, ok=None, status=None, caps=(None, None), piece_length=4, length=None, salt=0):
        rng = np.random.default_rng([SEED, n, flags, salt])
        L = 64 * ((n + 63) // 64)
        self.n, self.flags, self.piece_length = n, flags, piece_length
        self.length = max(4 * n - 1, 0) if length is None else length
        self.row = (rng.random(L) < 0.6).tolist() if row is None else row
        self.ok = (rng.random(L) < 0.7).tolist() if ok is None else ok
        self.status = bytes(rng.choice([0, 1, 1, 1, 2, 255], size=n).tolist()) if status is None else status
        self.caps = [n if c is None else c for c in caps]


def plan(ts, skew=(0, 0, 0)):
    batch = D.RequestBatch([t.n for t in ts], 1)
    have = D.HaveBatch(batch, [t.piece_length for t in ts], [t.length for t in ts])
    have.plan([t.flags for t in ts], {j: t.status for j, t in enumerate(ts) if t.flags & R.RESTORE},
              [t.caps[0] for t in ts], [t.caps[1] for t in ts], skew)
    bits = np.random.default_rng([SEED, len(ts)]).integers(1 << 63, size=batch.total_words + MARGIN, dtype=np.uint64)
    ok = np.zeros(int(have.ok_off[-1]) + 1, dtype=np.uint64)
    for j, t in enumerate(ts):
        if t.n:
            batch.rows(bits, j)[0] = words(t.row)
            ok[int(have.ok_off[j]):int(have.ok_off[j + 1])] = words(t.ok)
    return batch, have, bits, ok


def want(ts, skew=(0, 0, 0)):
    """Every buffer of OUTPUTS after the call."""
    batch, have, bits, _ = plan(ts, skew)
    w = {name: np.frombuffer(b"\xA5" * ((k + MARGIN) * np.dtype(dt).itemsize), dtype=dt).copy()
         for name, dt, k in zip(D.HaveOutputs.NAMES, D.HaveOutputs.DTYPES, have.sizes)}
    w["bits"] = bits
    for j, t in enumerate(ts):
        row, o = R.round_torrent(t.row, t.n, t.flags, t.piece_length, t.length, t.status, t.ok, *t.caps)
        if t.n:
            batch.rows(bits, j)[0] = words(row)
        for name in ("flags", "n_unexpected", "n_changed", "n_complete", "bytes"):
            w[name][j] = o[name]
        for name, at in (("changed", have.changed_off[j]), ("missing", have.missing_off[j]),
                         ("status_out", have.status_out_off[j]), ("wire_out", have.wire_out_off[j])):
            if o[name]:
                w[name][at:at + len(o[name])] = list(o[name])
    return w


def run(ts, dev=False, skew=(0, 0, 0), pinned=False, change=None):
    """(rc, every array after the call): the host form over numpy arrays, or the device form over uploads."""
    batch, have, bits, ok = plan(ts, skew)
    sizes = [k + MARGIN for k in have.sizes]
    if not dev:
        out = [np.frombuffer(b"\xA5" * (k * np.dtype(dt).itemsize), dtype=dt).copy() for dt, k in zip(D.HaveOutputs.DTYPES, sizes)]
        args = [batch.structs, have.structs, len(ts), bits.ctypes.data, have.sidecar.ctypes.data if have.sidecar.size else None,
                ok.ctypes.data, *(a.ctypes.data for a in out)]
        change and change(args)
        rc = lib.krk_have_round(*args)
        return rc, dict(zip(OUTPUTS, [bits] + out))
    bufs = [D.DeviceBuffer(max(a.nbytes, 1)) for a in (bits, have.sidecar, ok)]
    for b, a in zip(bufs, (bits, have.sidecar, ok)):
        if a.size:
            b.from_host(a)
    out = D.HaveOutputs(have, pinned=pinned, margin=MARGIN)
    out.fill(0xA5)
    args = [batch.structs, have.structs, len(ts), *(b.ptr for b in bufs), *(getattr(out, n).ptr for n in out.NAMES)]
    change and change(args)
    rc = lib.krk_have_round_dev(*args, None)
    check(lib.krk_stream_sync(None))
    return rc, dict(zip(OUTPUTS, (bufs[0].to_host(np.uint64, bits.size),) + out.to_host()))


def mismatches(label, rc, got, w):
    """What differs between one call's whole buffers and `w`, as text."""
    bad = [f"{label}: rc {rc}: {lib.krk_last_error()}"] * (rc != 0)
    for name in OUTPUTS:
        if got[name].tobytes() != w[name].tobytes():
            k = int(np.flatnonzero(got[name] != w[name])[0])
            bad.append(f"{label}: {name}[{k}] is {got[name][k]:#x}, want {w[name][k]:#x} ({int((got[name] != w[name]).sum())} differ)")
    return bad


def check_case(ts, dev, skew=(0, 0, 0), pinned=False):
    rc, got = run(ts, dev, skew, pinned)
    return mismatches(f"skew {skew}", rc, got, want(ts, skew))


def cases():
    """{label: (torrents, skew)}: one property a case."""
    out = {}
    for n in NS:  # every legal combination side by side, alone and with the emits: the spans abut
        out[f"n={n}"] = ([T(n, f | e, salt=k) for k, f in enumerate(COMBOS) for e in (0, EMITS)], (1, 3, 5))
    for at in range(8):  # every byte offset of the three byte spans
        out[f"offset {at}"] = ([T(n, R.RESTORE | EMITS, salt=at) for n in (65, 130, 10)], (at, (at + 3) % 8, (at + 5) % 8))
    for mid in (0, 5):  # three torrents packed back to back at odd offsets, two sharing a dword
        out[f"abutting, {mid} pieces in the middle"] = ([T(n, R.RESTORE | EMITS) for n in (13, mid, 67)], (1, 1, 3))
    for n_len in (64, 66, 0):  # BAD_STATUS: the row and every other output as without the restore
        out[f"status_len {n_len} of 65"] = ([T(65, f | EMITS, status=bytes([1] * n_len)) for f in (R.RESTORE, R.RESTORE | R.MERGE_AND)], (3, 0, 0))
    row, ok = bools(130, *range(0, 130, 3), tail=True), bools(130, *range(0, 130, 2), tail=True)  # 44 set, 86 clear; 43 changed by OR
    for d in (None, -1, 0, 1):
        caps = (0, 0) if d is None else (43 + d, 43 + d)
        out[f"caps {caps}"] = ([T(130, R.MERGE_OR | R.EMIT_MISSING, row, ok, caps=caps)], (0, 0, 0))
    for fill in (False, True):
        out[f"a row all {fill}, the tails set"] = ([T(130, f | EMITS, bools(130, fill=fill, tail=True), bools(130, fill=not fill, tail=True))
                                                    for f in (R.MERGE_OR, R.MERGE_AND, 0)], (0, 2, 2))
    full = bools(3, fill=True)
    out["bytes_out"] = ([T(3, 0, full, piece_length=0, length=77), T(3, 0, full, piece_length=5, length=13),
                         T(3, 0, full, piece_length=1 << 62, length=(1 << 63) - 1), T(3, 0, full, piece_length=5, length=0)], (0, 0, 0))
    out["above the unit cap"] = ([T(j % 10, (R.RESTORE | EMITS, R.MERGE_OR | EMITS)[j % 2], salt=j) for j in range(UNIT_CAP + 3)], (1, 2, 3))
    return out


def hand(dev):
    """Mismatches of the 10-piece vector, both directions, against values worked out by hand."""
    bad = []
    for at in (0, 3):
        _, got = run([T(10, R.EMIT_WIRE | R.EMIT_STATUS | R.EMIT_MISSING, bools(10, 0, 9), piece_length=4, length=37)], dev, (0, at, at))
        _, back = run([T(10, R.RESTORE, bools(10, 4), status=bytes([1, 0, 0, 0, 0, 0, 0, 0, 0, 2]))], dev, (at, 0, 0))
        mine = (got["wire_out"][at:at + 16].tobytes(), got["status_out"][at:at + 10].tolist(), got["missing"][:8].tolist(),
                int(got["n_complete"][0]), int(got["bytes"][0]), int(back["bits"][0]), int(back["n_unexpected"][0]))
        by_hand = (HAND, [1, 0, 0, 0, 0, 0, 0, 0, 0, 1], [1, 2, 3, 4, 5, 6, 7, 8], 2, 8, 1, 1)
        bad += [f"at {at}: {m!r}, by hand {h!r}" for m, h in zip(mine, by_hand) if m != h]
    return bad


def round_trips(dev):
    """Mismatches: wire_out joined by krk_peer_round, and status_out restored, both reproduce the row."""
    bad = []
    for n in (10, 65, 64 * PASS + 1):
        t = T(n, R.EMIT_WIRE | R.EMIT_STATUS, salt=7)
        _, got = run([t], dev, (0, 1, 3))
        row = words(t.row[:n] + [False] * (-n % 64))
        _, back = run([T(n, R.RESTORE, bools(n), status=got["status_out"][1:1 + n].tobytes())], dev)
        batch = D.RequestBatch([n], 1)
        peers = D.PeerBatch(batch).events(joins={0: [(0, got["wire_out"][3:3 + 8 + 8 * len(row)].tobytes())]})
        bits = np.zeros(batch.total_words, dtype=np.uint64)
        if dev:
            bits_dev, wire_dev = D.DeviceBuffer(bits.nbytes), D.DeviceBuffer(peers.wire.nbytes)
            bits_dev.from_host(bits)
            wire_dev.from_host(peers.wire)
            D.peer_round_dev(batch, peers, bits_dev, wire_dev, D.PeerOutputs(batch))
            check(lib.krk_stream_sync(None))
            bits = bits_dev.to_host(np.uint64, bits.size)
        else:
            D.peer_round(batch, peers, bits)
        bad += [f"n={n}: {name}" for name, r in (("restore", back["bits"][:len(row)]), ("join", batch.rows(bits, 0)[1])) if r.tolist() != row.tolist()]
    return bad


def refusals(dev=False):
    """Mismatches: every invalid call is KRK_EINVAL and leaves the rows and the outputs as they were."""
    ts = [T(65, R.RESTORE | R.MERGE_AND | EMITS), T(10, R.MERGE_OR | EMITS)]
    skew = (1, 1, 1)
    before = {**{n: np.frombuffer(b"\xA5" * a.nbytes, dtype=a.dtype) for n, a in want(ts, skew).items()}, "bits": plan(ts, skew)[2]}

    def field(k, j, name, v):  # argument k: a copy of the structs with one field changed
        def change(a):
            a[k] = type(a[k]).from_buffer_copy(a[k])
            setattr(a[k][j], name, v)
        return change

    calls = [("n_pieces 2^32", field(0, 1, "n_pieces", 1 << 32)), ("unknown flag bit", field(1, 0, "flags", 0x80)),
             ("both restores", field(1, 0, "flags", R.RESTORE | R.IN_CACHE)), ("both merges", field(1, 1, "flags", R.MERGE_OR | R.MERGE_AND)),
             ("reserved", field(1, 0, "reserved", 1)), ("negative piece_length", field(1, 1, "piece_length", -1)),
             ("negative length", field(1, 0, "length", -1)), ("status span overflows", field(1, 0, "status_len", (1 << 64) - 1)),
             ("changed cap overflows", field(1, 1, "changed_cap", (1 << 64) - 1)), ("missing cap overflows", field(1, 1, "missing_cap", (1 << 64) - 1)),
             ("bits_off 2^48", field(0, 0, "bits_off", 1 << 48))]
    calls += [(f"{name} 2^48", field(1, 0, name, 1 << 48)) for name in ("status_off", "ok_off", "changed_off", "missing_off", "status_out_off", "wire_out_off")]
    calls += [(f"NULL argument {k}", lambda a, k=k: a.__setitem__(k, None)) for k in (0, 1, *range(3, 15))]
    bad = []
    for label, change in calls:
        rc, got = run(ts, dev, skew, change=change)
        bad += [f"{label}: rc {rc}"] * (rc != _capi.KRK_EINVAL) + mismatches(label, 0, got, before)
    return bad
