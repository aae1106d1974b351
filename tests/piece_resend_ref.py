"""A restatement of the resend round's semantics (include/kraken_hip.h, "resend rounds"),
independent of the library's arithmetic: rows become one bool a piece, the rule is a plain double
loop over the failed entries and the peers, and "an earlier entry of this call with the same piece
was resent" is found by scanning the outputs so far -- where the library keeps the piece last
resent (to anybody, or to each peer).  A helper module, not a test file."""
import numpy as np

ALLOW_DUPLICATES, NONE = 0x100, 0xFFFFFFFF
EXPIRED, UNSENT, INVALID = 1, 2, 3


def bools(row: np.ndarray, n: int) -> np.ndarray:
    """The first n bits of a willf/bitset row (piece i = bit i & 63 of word i >> 6)."""
    return np.unpackbits(np.ascontiguousarray(row, dtype="<u8").view(np.uint8), bitorder="little")[:n].astype(bool)


def resend_torrent(rows: np.ndarray, n: int, n_peers: int, flags: int, quota, failed):
    """(target a failed entry, quota left a peer, entries resent) of one torrent: rows = have, then
    (bits_p, blocked_p) a peer; failed = [(piece, peer index or NONE, status)]."""
    have = bools(rows[0], n)
    holds = [bools(rows[1 + 2 * p], n) for p in range(n_peers)]
    blocked = [bools(rows[2 + 2 * p], n) for p in range(n_peers)]
    left = [max(int(q), 0) for q in quota]
    target = []
    for piece, peer, status in failed:
        got = NONE
        for p in range(n_peers):
            if status in (EXPIRED, INVALID) and p == peer:
                continue
            if not holds[p][piece] or have[piece]:
                continue
            if left[p] == 0:
                continue
            if blocked[p][piece]:
                continue
            earlier = [t for (i, _, _), t in zip(failed, target) if i == piece and t != NONE]
            if (p in earlier) if flags & ALLOW_DUPLICATES else bool(earlier):
                continue
            got = p
            left[p] -= 1
            break
        target.append(got)
    return (np.array(target, dtype=np.uint32), np.array(left, dtype=np.int32),
            sum(t != NONE for t in target))
