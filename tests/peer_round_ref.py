"""One torrent's peer round (krk_peer_round, include/kraken_hip.h) restated in plain Python: lists
of bools and struct for the wire, nothing of the library.  A helper module, not a test file."""
import struct

DISABLE_ENDGAME, TORRENT_COMPLETE, ENDGAME = 1, 1, 2
JOINED, BAD_BITFIELD, SET_FULL, PEER_COMPLETE, CLOSE, NOTIFY = 1, 2, 4, 8, 16, 32


def marshal(bits, length=None):
    """willf/bitset MarshalBinary of a list of bools (a multiple of 64 of them spells the tail
    bits too): the bit length, then the words, all big-endian uint64; word k holds bits 64k ..."""
    words = [sum(1 << j for j, b in enumerate(bits[k:k + 64]) if b) for k in range(0, len(bits), 64)]
    return struct.pack(f">{1 + len(words)}Q", len(bits) if length is None else length, *words)


def unmarshal(wire, n):
    """The n bools of a well-formed wire, or None."""
    W = (n + 63) // 64
    if len(wire) < 8 or struct.unpack(">Q", wire[:8])[0] != n or len(wire) != 8 + 8 * W:
        return None
    words = struct.unpack(f">{W}Q", wire[8:])
    return [bool(words[i >> 6] >> (i & 63) & 1) for i in range(n)]


def round_torrent(n, have, rows, live, joins, fulls, threshold, flags):
    """have: 64 W bools, tail included; rows: one such list a slot; live: one bool a slot;
    joins: [(slot, wire bytes)]; fulls: [slot].  Returns (rows, remaining, tflags, held, wanted,
    status): the rows with only what the round wrote changed."""
    rows, status = [list(r) for r in rows], [0] * len(rows)
    tail = [False] * (len(have) - n)
    for p, wire in joins:
        got = unmarshal(wire, n)
        status[p] = BAD_BITFIELD if got is None else JOINED
        if got is not None:
            rows[p] = got + tail
    for p in fulls:
        rows[p] = [True] * n + tail
        status[p] |= SET_FULL
    remaining = n - sum(have[:n])
    tflags = (TORRENT_COMPLETE if remaining == 0 else 0) | (
        ENDGAME if not flags & DISABLE_ENDGAME and remaining <= threshold else 0)
    held = [sum(r[:n]) for r in rows]
    wanted = [sum(b and not h for b, h in zip(r[:n], have)) for r in rows]
    for p, alive in enumerate(live):
        if alive:
            full = held[p] == n
            status[p] |= (PEER_COMPLETE if full else 0) | (0 if remaining else CLOSE if full else NOTIFY)
    return rows, remaining, tflags, held, wanted, status
