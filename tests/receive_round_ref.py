"""Receive rounds restated in plain Python (Dispatcher.handlePiecePayload with Torrent.WritePiece
over a torrent's queued payloads): a loop over the payloads with Python ints, a list of bools for
the row and dicts for the counts.  A helper module, not a test file; nothing here calls the library."""

OK, CHUNK, INDEX, DUPLICATE, BAD_SUM = range(5)
COMPLETE, COMPLETED_NOW = 1, 2
NONE, INVALID = 0xFFFFFFFF, 3


def plen(i, n, length, piece_length):
    """MetaInfo.GetPieceLength."""
    if i < 0 or i >= n:
        return 0
    return length - piece_length * i if i == n - 1 else piece_length


def round_torrent(have, n, length, piece_length, pays, sums, expected, now, received):
    """have: bools, updated (only [:n] are pieces); received {slot: time} is updated; pays: (slot
    or NONE, index, offset, length) in arrival order, sums parallel to it, expected a piece.
    Returns ([(status, file_off) a payload], arrived [(piece, from)] ascending, marks [(piece,
    peer, INVALID)] in arrival order, n_good {slot: count}, n_duplicate {slot: count},
    (n_complete, bytes, flags))."""
    before = sum(have[:n])
    out, arrived, marks, good, dup = [], [], [], {}, {}
    for (p, i, off, ln), s in zip(pays, sums):
        if off != 0 or ln != plen(i, n, length, piece_length):
            st = CHUNK
        elif i < 0 or i >= n:
            st = INDEX
        elif have[i]:
            st = DUPLICATE
        elif s != expected[i]:
            st = BAD_SUM
        else:
            st = OK
        out.append((st, piece_length * i if st == OK else 0))
        if p != NONE and (st == BAD_SUM or (st == CHUNK and 0 <= i < n)):
            marks.append((i, p, INVALID))
        if st == DUPLICATE and p != NONE:
            dup[p] = dup.get(p, 0) + 1
        if st == OK:
            have[i] = True
            arrived.append((i, p))
            if p != NONE:
                good[p] = good.get(p, 0) + 1
                received[p] = now
    after = sum(have[:n])
    flags = (COMPLETE | (COMPLETED_NOW if before != n else 0)) if after == n else 0
    return out, sorted(arrived), marks, good, dup, (after, min(after * piece_length, length), flags)
