"""A restatement of the piece request round's semantics (include/kraken_hip.h, "piece request
rounds"), independent of the library's arithmetic: rows become one bool a piece, `taken` is a
bool array, and a peer's picks are the first q of its candidates sorted by (key, index) -- a full
sort where the library keeps a k-smallest list (host) or extracts one minimum a pass (device).
splitmix64 is written twice, on Python integers (the definition) and on numpy uint64 arrays (what
the rounds use); tests/test_piece_request_matrix_cpu.py pins the second to the first.  A helper
module, not a test file."""
import numpy as np

RAREST_FIRST, SAMPLE, ALLOW_DUPLICATES, NONE = 0, 1, 0x100, 0xFFFFFFFF
M64 = (1 << 64) - 1


def splitmix64(x: int) -> int:
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample_key(seed: int, peer: int, i: int) -> int:
    return splitmix64(seed ^ (peer << 32 | i)) >> 32


def splitmix64_np(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = x.astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def sample_keys_np(seed: int, peer: int, idx: np.ndarray) -> np.ndarray:
    x = np.uint64(seed) ^ (np.uint64(peer << 32) | idx.astype(np.uint64))
    return splitmix64_np(x) >> np.uint64(32)


def bools(row: np.ndarray, n: int) -> np.ndarray:
    """The first n bits of a willf/bitset row (piece i = bit i & 63 of word i >> 6): whatever the
    row holds past n is dropped here, which is all "tail bits are ignored" means."""
    return np.unpackbits(np.ascontiguousarray(row, dtype="<u8").view(np.uint8), bitorder="little")[:n].astype(bool)


def availability(peer_rows, n: int) -> np.ndarray:
    """counts[i] = the peers whose bitfield has bit i set."""
    c = np.zeros(n, dtype=np.uint32)
    for r in peer_rows:
        c += bools(r, n)
    return c


def select(cand: np.ndarray, counts, q: int, policy: int, seed: int, peer: int) -> list:
    """The min(q, |cand|) candidates (cand: one bool a piece) with the smallest (key(i), i)."""
    idx = np.flatnonzero(cand)
    if q <= 0 or not idx.size:
        return []
    keys = sample_keys_np(seed, peer, idx) if policy == SAMPLE else np.asarray(counts)[idx].astype(np.uint64)
    return idx[np.lexsort((idx, keys))[:q]].tolist()


def round_torrent(rows: np.ndarray, n: int, n_peers: int, flags: int, seed: int, quota, limit: int):
    """(counts, picks, n_picked) of one torrent: rows = have, then (bits_p, blocked_p) a peer."""
    have = bools(rows[0], n)
    counts = availability([rows[1 + 2 * p] for p in range(n_peers)], n)
    taken = np.zeros(n, dtype=bool)
    picks = np.full((n_peers, limit), NONE, dtype=np.uint32)
    n_picked = np.zeros(n_peers, dtype=np.uint32)
    for p in range(n_peers):
        q = max(int(quota[p]), 0)
        assert q <= limit
        cand = bools(rows[1 + 2 * p], n) & ~have & ~bools(rows[2 + 2 * p], n) & ~taken
        got = select(cand, counts, q, flags & 0xFF, seed, p)
        picks[p, :len(got)] = got
        n_picked[p] = len(got)
        if not flags & ALLOW_DUPLICATES:
            taken[got] = True
    return counts, picks, n_picked
