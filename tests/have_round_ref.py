"""One have round (krk_have_round) restated in plain Python over lists and bytes, one loop a step:
what tests/have_round_cases.py holds both forms of the library against.  Nothing here is shared
with the C++."""
RESTORE, IN_CACHE, MERGE_OR, MERGE_AND, EMIT_STATUS, EMIT_WIRE, EMIT_MISSING = 1, 2, 4, 8, 16, 32, 64
BAD_STATUS = 1


def round_torrent(row, n, flags, piece_length=0, length=0, status=b"", ok=(), changed_cap=0, missing_cap=0):
    """row: 64 W bools (the tail included), ok the same; returns the row after the round and a dict
    of the outputs: flags, n_unexpected, n_changed, changed, n_complete, bytes, status_out, wire_out,
    missing (the emits None when not asked for)."""
    row, o = list(row), {"flags": 0, "n_unexpected": 0, "status_out": None, "wire_out": None, "missing": None}
    wrote = bool(flags & (IN_CACHE | MERGE_OR | MERGE_AND))
    if flags & RESTORE:
        if len(status) != n:
            o["flags"] = BAD_STATUS
        else:
            wrote = True
            for i in range(n):
                row[i] = status[i] == 1
                o["n_unexpected"] += status[i] > 1
    if flags & IN_CACHE:
        for i in range(n):
            row[i] = True
    changed = []
    for i in range(n):
        if flags & MERGE_OR and ok[i] and not row[i]:
            changed.append(i)
            row[i] = True
        if flags & MERGE_AND and row[i] and not ok[i]:
            changed.append(i)
            row[i] = False
    if wrote:
        for i in range(n, len(row)):
            row[i] = False
    o["n_changed"], o["changed"] = len(changed), changed[:changed_cap]
    done = o["n_complete"] = sum(row[:n])
    o["bytes"] = length if piece_length == 0 or done > length // piece_length else done * piece_length
    if flags & EMIT_STATUS:
        o["status_out"] = bytes(1 if row[i] else 0 for i in range(n))
    if flags & EMIT_WIRE:
        o["wire_out"] = marshal(row[:n])
    if flags & EMIT_MISSING:
        o["missing"] = [i for i in range(n) if not row[i]][:missing_cap]
    return row, o


def marshal(bits):
    """willf/bitset MarshalBinary: the bit length, then each word of 64 bits, all uint64 big-endian."""
    out = len(bits).to_bytes(8, "big")
    for w in range(0, len(bits), 64):
        out += sum(1 << k for k, b in enumerate(bits[w:w + 64]) if b).to_bytes(8, "big")
    return out
