"""The HRW scoring kernel and the ring filter (hrw_place.hip) at their structural edges: the
case builders, two restated references and raw-byte callers shared by
tests/test_hrw_matrix_cpu.py (no device: the references and the inputs proved before they are
trusted) and tests/test_gpu_hrw_edges.py (bit for bit against the oracle).  A helper module,
not a test file; importing it loads neither library.

Keys and labels are raw `bytes` here (keys are passed to the ABI as their hex text): labels
carry 0x00 and bytes >= 0x80, which the `str` wrappers of kraken_amd.hrw and oracle.oracle
would re-encode as UTF-8.

murmur_preimage16: MurmurHash3_x64_128's block round and finaliser are bijections of the
128-bit state, so for any wanted Sum (h1 + h2 after the finaliser) and any free 64-bit `b`
there is exactly one 16-byte message -- one block, no tail -- that hashes to it.  A 32-digit
hex key scored against a node with the EMPTY label is that message, which puts a chosen Sum
(and so a chosen UInt64ToFloat64 value, rehash branch included) through the production
scoring kernel."""
import ctypes as C
import decimal
import math
import struct

import numpy as np

SEED = 20261019
M64 = (1 << 64) - 1
M53 = (1 << 53) - 1
C1, C2 = 0x87C37B91114253D5, 0x4CF5AD432745937F
F1, F2 = 0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
MAX_NODES = 4096  # kHrwMaxNodes: the doubles of one LDS tile
FOLD = 0x16A09E667F3BCD  # FOLD / 2^53 is the double sqrt(2)/2 that Go's log folds at

# ------------------------------------------------------------------ murmur3, loop-based


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def _rotr(x, r):
    return ((x >> r) | (x << (64 - r))) & M64


def _fmix(k):
    k ^= k >> 33
    k = (k * F1) & M64
    k ^= k >> 33
    k = (k * F2) & M64
    return k ^ (k >> 33)


def murmur3_h1(data: bytes) -> int:
    """murmur3.New64 (MurmurHash3_x64_128 h1 + h2, seed 0): blocks, then the tail gathered by
    two loops (no switch), as tests/golden/gen_golden.py states it."""
    h1 = h2 = 0
    n = len(data)
    nb = n // 16
    for i in range(nb):
        k1, k2 = struct.unpack_from("<QQ", data, 16 * i)
        h1 ^= (_rotl((k1 * C1) & M64, 31) * C2) & M64
        h1 = (_rotl(h1, 27) + h2) & M64
        h1 = (h1 * 5 + 0x52DCE729) & M64
        h2 ^= (_rotl((k2 * C2) & M64, 33) * C1) & M64
        h2 = (_rotl(h2, 31) + h1) & M64
        h2 = (h2 * 5 + 0x38495AB5) & M64
    tail = data[16 * nb:]
    k1 = k2 = 0
    for i in range(len(tail) - 1, 7, -1):
        k2 = (k2 << 8) | tail[i]
    for i in range(min(len(tail), 8) - 1, -1, -1):
        k1 = (k1 << 8) | tail[i]
    if len(tail) > 8:
        h2 ^= (_rotl((k2 * C2) & M64, 33) * C1) & M64
    if len(tail) > 0:
        h1 ^= (_rotl((k1 * C1) & M64, 31) * C2) & M64
    h1 ^= n
    h2 ^= n
    h1 = (h1 + h2) & M64
    h2 = (h2 + h1) & M64
    return (_fmix(h1) + _fmix(h2)) & M64


# ------------------------------------------------------------------ the inverse
_INV = {c: pow(c, -1, 1 << 64) for c in (C1, C2, 5, F1, F2)}


def _unxorshift(y, s):
    """x with x ^ (x >> s) == y: the top s bits of y are x's, each pass fixes s more."""
    x = y
    for _ in range(64 // s + 1):
        x = y ^ (x >> s)
    return x


def _unfmix(k):
    k = _unxorshift(k, 33)
    k = (k * _INV[F2]) & M64
    k = _unxorshift(k, 33)
    k = (k * _INV[F1]) & M64
    return _unxorshift(k, 33)


def murmur_preimage16(target: int, b: int) -> bytes:
    """The 16-byte message whose Sum is `target` and whose finalised h2 is `b`."""
    g1, g2 = _unfmix((target - b) & M64), _unfmix(b & M64)  # after h1 += h2; h2 += h1
    h2 = (g2 - g1) & M64
    h1 = (g1 - h2) & M64
    h1 ^= 16
    h2 ^= 16
    # the block round from h1 = h2 = 0, backwards (h2's half first: it added the new h1)
    x2 = _rotr(((((h2 - 0x38495AB5) & M64) * _INV[5] & M64) - h1) & M64, 31)
    k2 = (_rotr((x2 * _INV[C1]) & M64, 33) * _INV[C2]) & M64
    x1 = _rotr(((h1 - 0x52DCE729) & M64) * _INV[5] & M64, 27)
    k1 = (_rotr((x1 * _INV[C2]) & M64, 31) * _INV[C1]) & M64
    return struct.pack("<QQ", k1, k2)


# ------------------------------------------------------------------ references
def u64_value(h1: int) -> int:
    """The 53-bit integer hrw.UInt64ToFloat64 divides by 2^53: the Sum's low 53 bits, or those
    of murmur3 over its 8 big-endian bytes when they are all zero (rendezvous.go:99-118)."""
    val = h1 & M53
    if val == 0:
        val = murmur3_h1(h1.to_bytes(8, "big")) & M53
    return val


def score_decimal(val: int, weight: int) -> decimal.Decimal:
    """-w / ln(val / 2^53) at 50 digits (0 < val < 2^53)."""
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        return -decimal.Decimal(weight) / (decimal.Decimal(val) / decimal.Decimal(1 << 53)).ln()


def ulps_off(got: float, want: decimal.Decimal) -> float:
    """|got - want| in units of got's last place."""
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        return float(abs(decimal.Decimal(got) - want) / decimal.Decimal(math.ulp(got)))


# ------------------------------------------------------------------ builders
def _marked(rng, n):
    """n seeded bytes with one byte >= 0x80 (n >= 1) and one 0x00 (n >= 2)."""
    b = bytearray(rng.integers(1, 256, size=n, dtype=np.uint8).tobytes())
    if n >= 1:
        b[int(rng.integers(0, n))] |= 0x80
    if n >= 2:
        hi = [i for i in range(n) if b[i] >= 0x80]
        z = int(rng.integers(0, n))
        if [z] == hi:  # keep the only high byte
            z = (z + 1) % n
        b[z] = 0
    return bytes(b)


def seam_matrix():
    """(keys, labels): 34 keys of 0..33 bytes and 34 labels of 0..33 bytes.  The 1,156
    messages key || label have every length 0..66, every tail residue n & 15 with the key /
    label seam at every byte of the 16-byte block."""
    rng = np.random.default_rng(SEED + 1)
    return [_marked(rng, n) for n in range(34)], [_marked(rng, n) for n in range(34)]


def seam_pairs(keys, labels):
    return {((len(k) + len(l)) & 15, len(k) & 15) for k in keys for l in labels}


def mixed_weights(n):
    return [[100, 200, 400, 800, 1, 7, 1000003][i % 7] for i in range(n)]


B_NODES = (65, 100, 255, 256, 1000, 2048, 2049, 4095, 4096)


def keys_per_block(n_nodes):
    """launch_hrw_order's tile: the keys one workgroup scores against all nodes."""
    return min(64, MAX_NODES // n_nodes)


def tile_key_counts(n_nodes):
    """Batch sizes around one tile: below it, full, one over (a ragged second tile), and two
    tiles and one; from 2,049 nodes on a tile is one key."""
    if n_nodes >= 2049:
        return [1, 3]
    kpb = keys_per_block(n_nodes)
    return sorted({c for c in (1, kpb - 1, kpb, kpb + 1, 2 * kpb + 1) if c > 0})


def tile_case(n_nodes):
    """(keys, labels, weights) for group B: labels of varied length, cycling weights, and as
    many keys (1..40 bytes) as the largest batch needs."""
    rng = np.random.default_rng(SEED + 2 + n_nodes)
    labels = [f"n{i}".encode() for i in range(n_nodes)]
    weights = [[100, 200, 400, 800][i % 4] for i in range(n_nodes)]
    keys = [rng.bytes(int(rng.integers(1, 41))) for _ in range(max(tile_key_counts(n_nodes)))]
    return keys, labels, weights


def plain_case(n_nodes, n_keys, seed):
    """Ordinary labels (14..16 bytes), weights 100 and keys of 2, 1, 32 or 20 bytes."""
    rng = np.random.default_rng(SEED + seed)
    labels = [f"origin-{i:03d}:15002".encode() for i in range(n_nodes)]
    keys = [rng.bytes((2, 1, 32, 20)[i % 4]) for i in range(n_keys)]
    return keys, labels, [100] * n_nodes


TIE_PAIRS = ((0, 5), (63, 64), (1, 69))


def tie_case():
    """70 nodes of equal weight; each pair of TIE_PAIRS has byte-equal labels, so equal scores
    for every key: an exact tie inside a wave's worth of nodes, across node 63 | 64 and
    between the second and the last node."""
    keys, labels, weights = plain_case(70, 64, 40)
    for a, b in TIE_PAIRS:
        labels[b] = labels[a]
    return keys, labels, weights


EXTREME_WEIGHTS = (INT64_MIN, -1, 0, 1, (1 << 53) + 1, INT64_MAX)

BAD_KINDS = ("odd", "first", "last", "g0")


def bad_key(kind, rng):
    """Hex text hex.DecodeString refuses: an odd digit count, a non-hex first or last
    character, and "g0"."""
    body = rng.bytes(8).hex()
    return {"odd": body[:-1], "first": "x" + body[1:], "last": body[:-1] + "G", "g0": "g0"}[kind]


def mixed_keys(n=200):
    """n hex keys of which every seventh (1, 8, 15, ...) is bad, the kinds in turn.  Returns
    (hex texts, is_bad flags)."""
    rng = np.random.default_rng(SEED + 41)
    keys, bad = [], []
    for i in range(n):
        if i % 7 == 1:
            keys.append(bad_key(BAD_KINDS[(i // 7) % 4], rng))
            bad.append(True)
        else:
            keys.append(rng.bytes((2, 1, 32, 20)[i % 4]).hex())
            bad.append(False)
    return keys, np.array(bad)


def is_valid_hex(s: str) -> bool:
    return len(s) % 2 == 0 and all(c in "0123456789abcdefABCDEF" for c in s)


def sum_targets():
    """Group E: (name, Sum) -- the murmur3 Sums to put through the scoring kernel.  Only the
    low 53 bits of a Sum are scored; the high 11 are seeded but for the twelve zero-low-bit
    Sums of rendezvous_test.go:59-98, which are taken whole."""
    rng = np.random.default_rng(SEED + 5)
    hi = lambda: int(rng.integers(0, 1 << 11)) << 53
    out = [(f"rehash 2^{53 + i}", ((1 << 53) << i) & M64) for i in range(12)]
    out += [(name, hi() | v) for name, v in (("val 1", 1), ("val 2^53-1", M53), ("val 2^52", 1 << 52),
                                             ("val 2^52-1", (1 << 52) - 1), ("fold", FOLD),
                                             ("fold-1", FOLD - 1))]
    out += [(f"2^{k}", hi() | (1 << k)) for k in range(53)]
    out += [(f"3*2^{k}", hi() | (3 << k)) for k in range(52)]
    out += [(f"random {i}", int(rng.integers(0, 1 << 64, dtype=np.uint64))) for i in range(256)]
    return out


def sum_messages():
    """One 16-byte preimage a target of sum_targets(), each with its own seeded free half."""
    rng = np.random.default_rng(SEED + 6)
    return [murmur_preimage16(t, int(rng.integers(0, 1 << 64, dtype=np.uint64))) for _, t in sum_targets()]


ORDINARY_LABEL = b"origin-000.kraken.test:15002"


def healthy_sets(n_nodes):
    """Group F: all, none, exactly one node (first, middle, last) and all but one; duplicates
    of small rings dropped."""
    sets = [np.ones(n_nodes, np.uint8), np.zeros(n_nodes, np.uint8)]
    for j in (0, n_nodes // 2, n_nodes - 1):
        h = np.zeros(n_nodes, np.uint8)
        h[j] = 1
        sets.append(h)
    h = np.ones(n_nodes, np.uint8)
    h[n_nodes // 3] = 0
    sets.append(h)
    out = []
    for h in sets:
        if not any(np.array_equal(h, o) for o in out):
            out.append(h)
    return out


def replica_counts(n_nodes):
    return sorted({-2 ** 31, -1, 0, 1, n_nodes - 1, n_nodes, n_nodes + 1})


def ring_labels(n_nodes):
    return [f"origin-{i:03d}.kraken.test:15002".encode() for i in range(n_nodes)]


def ring_digests(n=512):
    return np.random.default_rng(SEED + 7).integers(0, 256, size=(n, 32), dtype=np.uint8)


# ------------------------------------------------------------------ raw-byte callers
def _offsets(parts):
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    if parts:
        off[1:] = np.cumsum([len(p) for p in parts])
    return off


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Nodes:
    """A krk_nodes over raw label bytes, kept alive with its arrays.  n_nodes may be forced
    (0 or past the arrays' end) for calls that must be refused before anything is read."""

    def __init__(self, labels, weights, n_nodes=None):
        from kraken_amd._capi import krk_nodes
        self.blob = b"".join(labels)
        self.off = _offsets(labels)
        self.w = np.ascontiguousarray(weights, dtype=np.int64)
        self.n = len(labels)
        self.s = krk_nodes(self.blob, _p(self.off, C.c_uint64), _p(self.w, C.c_int64),
                           self.n if n_nodes is None else n_nodes)


def as_hex(keys):
    return [k.hex() if isinstance(k, (bytes, bytearray)) else k for k in keys]


def krk_ordered(keys, labels, weights, n_out, want_scores=True, order=None, scores=None, n_nodes=None):
    """krk_hrw_ordered over hex texts (or raw keys, hexed here) and raw labels.  Returns
    (rc, order[len(keys), n_out], scores[len(keys), N] or None); `order` / `scores` may be
    given prefilled, to see what a call leaves of them."""
    from kraken_amd._capi import lib
    kb = [k.encode() for k in as_hex(keys)]
    nt = Nodes(labels, weights, n_nodes)
    if order is None:
        order = np.full((len(kb), n_out), -7, dtype=np.int32)
    if scores is None and want_scores:
        scores = np.full((len(kb), len(labels)), -7.0, dtype=np.float64)
    hold = order if order.size else np.zeros(1, np.int32)  # order_out must not be NULL
    rc = lib.krk_hrw_ordered(b"".join(kb), _p(_offsets(kb), C.c_uint64), len(kb), C.byref(nt.s), n_out,
                             _p(hold, C.c_int32), _p(scores, C.c_double) if want_scores else None)
    return rc, order, scores


_ORC = {}


def orc_ordered(orc, keys, labels, weights):
    """orc_hrw_ordered for every key: (full orders [len(keys), N], scores [len(keys), N]),
    computed once for a given input and returned read-only."""
    hx = as_hex(keys)
    memo = (tuple(hx), tuple(labels), tuple(int(w) for w in weights))
    hit = _ORC.get(memo)
    if hit is not None:
        return hit
    N = len(labels)
    blob, off = b"".join(labels), _offsets(labels)
    w = np.ascontiguousarray(weights, dtype=np.int64)
    order = np.zeros((len(hx), N), dtype=np.int32)
    scores = np.zeros((len(hx), N), dtype=np.float64)
    f = orc.lib().orc_hrw_ordered
    for i, k in enumerate(hx):
        kb = k.encode()
        m = f(kb, len(kb), blob, _p(off, C.c_uint64), _p(w, C.c_int64), N, N, _p(order[i], C.c_int32),
              _p(scores[i], C.c_double))
        assert m == N
    order.flags.writeable = scores.flags.writeable = False
    _ORC[memo] = (order, scores)
    return order, scores


def orc_owner_table(orc, labels, weights, healthy, max_replica):
    """orc_ring_owner_table over raw labels: (locs [65536, max(1, max_replica)], counts)."""
    blob, off = b"".join(labels), _offsets(labels)
    w = np.ascontiguousarray(weights, dtype=np.int64)
    h = np.ascontiguousarray(healthy, dtype=np.uint8)
    row = max(1, int(max_replica))
    locs = np.zeros((65536, row), dtype=np.int32)
    counts = np.zeros(65536, dtype=np.uint8)
    orc.lib().orc_ring_owner_table(blob, _p(off, C.c_uint64), _p(w, C.c_int64), len(labels), _p(h, C.c_uint8),
                                   int(max_replica), row, _p(locs, C.c_int32), _p(counts, C.c_uint8))
    return locs, counts
