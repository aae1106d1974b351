"""A plain-Python restatement of one request table round (include/kraken_hip.h, "request table
rounds"): lists of tuples, sets and `sorted`, no numpy and nothing of the library.  It is the
reference tests/request_table_matrix.py holds both forms of the round to.  A helper module, not a
test file."""

ALLOW_DUPLICATES = 0x100
PENDING, EXPIRED, UNSENT, INVALID = 0, 1, 2, 3


def round_torrent(n, n_peers, flags, have, held, table, cap, arrived=(), gone=(), marks=(), holds=(), records=(),
                  picks=None, now=0, timeout=0, limit=1):
    """One torrent's round.  have: a set of pieces; held: one set of pieces a peer; table:
    [(piece, peer, status, sent_at)] in recording order; picks: one list of pieces a peer, or None.
    Returns (have, held, table, blocked, quota, failed, n_dropped): blocked one set of pieces a
    peer, quota one int a peer, failed [(piece, peer, status)]."""
    have = set(have) | set(arrived)
    held = [set() if p in set(gone) else set(h) for p, h in enumerate(held)]
    table = [e for e in table
             if e[0] < n and e[1] < n_peers and e[2] <= INVALID and e[0] not in set(arrived) and e[1] not in set(gone)]
    for piece, peer, status in marks:
        table = [(e[0], e[1], status, e[3]) if (e[0], e[1]) == (piece, peer) else e for e in table]
    for piece, peer in holds:
        held[peer].add(piece)
    new = list(records)
    for p in range(n_peers if picks is not None else 0):
        new += [(i, p) for i in picks[p][:limit]]
    dropped = 0
    for piece, peer in new:
        if piece >= n or len(table) >= cap:
            dropped += 1
        else:
            table.append((piece, peer, PENDING, now))

    def live(e):
        return e[2] == PENDING and not now > e[3] + timeout

    quota = [max(limit - sum(1 for e in table if live(e) and e[1] == p), 0) for p in range(n_peers)]
    if flags & ALLOW_DUPLICATES:
        blocked = [{e[0] for e in table if live(e) and e[1] == p} for p in range(n_peers)]
    else:
        blocked = [{e[0] for e in table if live(e)} for p in range(n_peers)]
    failed = [(e[0], e[1], EXPIRED if e[2] == PENDING else e[2])
              for _, e in sorted(((e[0], k), e) for k, e in enumerate(table) if not live(e))]
    return have, held, table, blocked, quota, failed, dropped


def clear_peer_reference(requests, peer):
    """Manager.ClearPeer (manager.go:180-196) over {piece: [(peer, ...)]}: only the FIRST entry a piece leaves."""
    for rs in requests.values():
        for j, r in enumerate(rs):
            if r[0] == peer:
                rs[j] = rs[-1]
                rs.pop()
                break
    return requests
