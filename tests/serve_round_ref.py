"""Serve rounds restated in plain Python (Dispatcher.handlePieceRequest over a torrent's queued
requests): a loop over the requests with Python ints, a list of bools a row and dicts for the
counts.  A helper module, not a test file; nothing here calls the library."""

OK, CHUNK, INDEX, INCOMPLETE, GONE = range(5)


def plen(i, n, length, piece_length):
    """MetaInfo.GetPieceLength."""
    if i < 0 or i >= n:
        return 0
    return length - piece_length * i if i == n - 1 else piece_length


def round_torrent(have, rows, live, n, length, piece_length, reqs, now, token_size, sent):
    """have: bools; rows {slot: bools} and sent {slot: time} are updated; live: bools a slot; reqs:
    (slot, index, offset, length) in arrival order.  Returns ([(status, file_off, len, send_off,
    token_off) a request], received {slot: count}, n_sent {slot: count}, (n_ok, bytes, tokens))."""
    out, received, n_sent, n_ok, total, tokens = [], {}, {}, 0, 0, 0
    for p, i, off, ln in reqs:
        received[p] = received.get(p, 0) + 1
        if off != 0 or ln != plen(i, n, length, piece_length):
            st = CHUNK
        elif i < 0 or i >= n:
            st = INDEX
        elif not have[i]:
            st = INCOMPLETE
        elif not live[p]:
            st = GONE
        else:
            st = OK
        if st != OK:
            out.append((st, 0, 0, 0, 0))
            continue
        out.append((OK, piece_length * i, ln, total, tokens))
        n_ok, total = n_ok + 1, total + ln
        tokens += max(ln * 8 // token_size, 1) if token_size else 0
        n_sent[p] = n_sent.get(p, 0) + 1
        sent[p] = now
        rows[p][i] = True
    return out, received, n_sent, (n_ok, total, tokens)
