"""Ring ownership as bitsets where no GPU is: the shard masks (krk_ring_mask_owns,
krk_ring_mask_moved) against the oracle's owner tables and plain set logic, bit by bit; the host
selection (krk_ring_select) over the ring-select matrix (tests/ring_select_matrix.py) against its
numpy transcription; castore.force_cleanup_plan against a per-name transcription of maybeDelete
(origin/blobserver/server.go:686-759); and krk_ring_select_dev refusing to run without a device."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from kraken_amd import _capi, castore, hashring
from kraken_amd._capi import lib
from tests import ring_select_matrix as M

i32p, u8p, u64p = C.POINTER(C.c_int32), M.u8p, M.u64p
CANARY = M.CANARY


def labels_of(n):
    return [f"origin-{i:03d}.kraken.test:15002" for i in range(n)]


def health_of(n, kind):
    h = np.ones(n, dtype=np.uint8)
    if kind == "one down":
        h[n // 2] = 0
    elif kind == "none":
        h[:] = 0
    return h


_tables = {}


def table(orc, labels, healthy, max_replica):
    """The oracle's 65,536-row owner table of a membership, computed once."""
    key = (tuple(labels), bytes(healthy), max_replica)
    if key not in _tables:
        _tables[key] = orc.ring_owner_table(labels, [100] * len(labels), healthy, max_replica)
    return _tables[key]


def owner_sets(locs, counts, names):
    """[frozenset of owner names] a shard: the stringset maybeDelete and applyToReplicas build."""
    return [frozenset(names[j] for j in locs[s, :counts[s]]) for s in range(65536)]


def mask_bools(mask):
    return np.unpackbits(mask.view(np.uint8), bitorder="little").astype(bool)


def owns(locs, counts, node):
    m = np.full(1024, CANARY, dtype=np.uint64)
    rc = lib.krk_ring_mask_owns(locs.ctypes.data_as(i32p), counts.ctypes.data_as(u8p), locs.shape[1], node,
                                m.ctypes.data_as(u64p))
    assert rc == _capi.KRK_OK, lib.krk_last_error()
    return m


def moved(ta, tb, b_to_a, n_nodes_b):
    (la, ca), (lb, cb) = ta, tb
    m = np.full(1024, CANARY, dtype=np.uint64)
    b2a = None if b_to_a is None else np.asarray(b_to_a, dtype=np.int32)
    rc = lib.krk_ring_mask_moved(la.ctypes.data_as(i32p), ca.ctypes.data_as(u8p), la.shape[1], lb.ctypes.data_as(i32p),
                                 cb.ctypes.data_as(u8p), lb.shape[1], None if b2a is None else b2a.ctypes.data_as(i32p),
                                 n_nodes_b, m.ctypes.data_as(u64p))
    assert rc == _capi.KRK_OK, lib.krk_last_error()
    return m


# ------------------------------------------------------------------ masks
@pytest.mark.parametrize("n_nodes", [1, 3, 5])
@pytest.mark.parametrize("health", ["all", "one down", "none"])
def test_owns_mask_equals_set_membership_of_the_oracle_table(orc, n_nodes, health):
    labels, healthy = labels_of(n_nodes), health_of(n_nodes, health)
    for max_replica in (1, 3, n_nodes + 2):
        locs, counts = table(orc, labels, healthy, max_replica)
        sets = owner_sets(locs, counts, labels)
        for node, name in enumerate(labels):
            want = np.fromiter((name in s for s in sets), dtype=bool, count=65536)
            assert np.array_equal(mask_bools(owns(locs, counts, node)), want), (n_nodes, health, max_replica, node)
        # a node index no row has, and the rows' padding value: nobody's shards
        assert not owns(locs, counts, n_nodes).any() and not owns(locs, counts, -1).any()
    # the owners of a shard are max(1, min(MaxReplica, healthy nodes)), so the masks' weights add up
    locs, counts = table(orc, labels, healthy, 3)
    total = sum(int(mask_bools(owns(locs, counts, j)).sum()) for j in range(n_nodes))
    assert total == int(counts.astype(np.int64).sum())


def test_moved_mask_cases(orc):
    l3, l4 = labels_of(3), labels_of(4)
    a = table(orc, l3, health_of(3, "all"), 2)
    zero = np.zeros(65536, dtype=bool)
    # identity b_to_a (NULL, and spelled out) and equal tables
    assert np.array_equal(mask_bools(moved(a, a, None, 3)), zero)
    assert np.array_equal(mask_bools(moved(a, a, [0, 1, 2], 3)), zero)

    def want(ta, names_a, tb, names_b):
        sa, sb = owner_sets(*ta, names_a), owner_sets(*tb, names_b)
        return np.fromiter((x != y for x, y in zip(sa, sb)), dtype=bool, count=65536)

    # a node added, a node removed
    b = table(orc, l4, health_of(4, "all"), 2)
    added = mask_bools(moved(a, b, [0, 1, 2, -1], 4))
    assert np.array_equal(added, want(a, l3, b, l4)) and 0 < added.sum() < 65536
    removed = mask_bools(moved(b, a, [0, 1, 2], 3))
    assert np.array_equal(removed, added)  # the same shards change hands either way
    # the new node's gain is exactly its owns mask, and a moved shard here is one it gained
    gained = mask_bools(owns(*b, 3))
    assert np.array_equal(added, gained)
    # a health flip only
    h = table(orc, l3, health_of(3, "one down"), 2)
    flip = mask_bools(moved(a, h, None, 3))
    assert np.array_equal(flip, want(a, l3, h, l3)) and flip.any()
    # MaxReplica changed: rows of another width
    wide = table(orc, l3, health_of(3, "all"), 3)
    assert np.array_equal(mask_bools(moved(a, wide, None, 3)), want(a, l3, wide, l3))
    # the same sets in another order: every row's owners reversed
    locs, counts = a
    rev = locs.copy()
    for q in range(locs.shape[1]):
        src = counts.astype(np.int64) - 1 - q
        ok = src >= 0
        rev[ok, q] = locs[ok, src[ok]]
    assert not np.array_equal(rev, locs)
    assert np.array_equal(mask_bools(moved(a, (rev, counts), None, 3)), zero)
    # the same ring under another node numbering
    perm = [l3[2], l3[0], l3[1]]
    p = table(orc, perm, health_of(3, "all"), 2)
    assert np.array_equal(mask_bools(moved(a, p, [2, 0, 1], 3)), zero)
    assert np.array_equal(mask_bools(moved(a, p, None, 3)), want(a, l3, p, l3))  # read as A's numbering: differs


def test_mask_refusals_leave_the_mask_untouched(orc):
    locs, counts = table(orc, labels_of(3), health_of(3, "all"), 2)
    lp, cp = locs.ctypes.data_as(i32p), counts.ctypes.data_as(u8p)
    m = np.full(1024, CANARY, dtype=np.uint64)
    mp = m.ctypes.data_as(u64p)
    b2a = np.array([0, 1, 2], dtype=np.int32).ctypes.data_as(i32p)
    E = _capi.KRK_EINVAL
    assert lib.krk_ring_mask_owns(None, cp, 2, 0, mp) == E
    assert lib.krk_ring_mask_owns(lp, None, 2, 0, mp) == E
    assert lib.krk_ring_mask_owns(lp, cp, 2, 0, None) == E
    assert lib.krk_ring_mask_owns(lp, cp, 0, 0, mp) == E
    assert lib.krk_ring_mask_moved(None, cp, 2, lp, cp, 2, b2a, 3, mp) == E
    assert lib.krk_ring_mask_moved(lp, None, 2, lp, cp, 2, b2a, 3, mp) == E
    assert lib.krk_ring_mask_moved(lp, cp, 2, None, cp, 2, b2a, 3, mp) == E
    assert lib.krk_ring_mask_moved(lp, cp, 2, lp, None, 2, b2a, 3, mp) == E
    assert lib.krk_ring_mask_moved(lp, cp, 2, lp, cp, 2, b2a, 3, None) == E
    assert lib.krk_ring_mask_moved(lp, cp, 0, lp, cp, 2, b2a, 3, mp) == E
    assert lib.krk_ring_mask_moved(lp, cp, 2, lp, cp, 0, b2a, 3, mp) == E
    # a B owner outside [0, n_nodes_b): node 2 owns shards, n_nodes_b says there are two nodes
    assert lib.krk_ring_mask_moved(lp, cp, 2, lp, cp, 2, b2a, 2, mp) == E
    bad = locs.copy()
    bad[65535, 0] = -1
    assert lib.krk_ring_mask_moved(lp, cp, 2, bad.ctypes.data_as(i32p), cp, 2, None, 3, mp) == E
    assert (m == CANARY).all()
    assert lib.krk_ring_mask_moved(lp, cp, 2, lp, cp, 2, b2a, 3, mp) == _capi.KRK_OK and not m.any()


# ------------------------------------------------------------------ the host selection
@pytest.fixture(scope="module")
def data():
    return M.Data()


def test_matrix_shapes_and_edges(data):
    W, T = M.W, M.T
    assert W % 256 == 0 and T >= 2 and M.N_TAIL > 2 * T * W and (M.N_TAIL - 2 * T * W) % W % 64
    assert {0, 63, 64, W - 1, W, T * W - 1, T * W, 2 * T * W, M.N_TAIL - 1} <= set(M.EDGES)
    for n in M.SHAPES:
        bits, idx = data.reference(M.Case(n, "edges", False, False))
        assert idx.tolist() == [e for e in M.EDGES if e < n]
        assert int(sum(bin(int(w)).count("1") for w in bits)) == idx.size
    assert len(M.cases()) == len(M.SHAPES) * 12


def test_host_select_small_shapes_every_cap(data):
    calls, bad = M.run_cases(M.HostBackend(data), M.cases(M.SMALL))
    assert calls > 0 and bad == [], bad[:5]


def test_host_select_scan_tile_shapes(data):
    host = M.HostBackend(data)
    calls, bad = M.run_cases(host, [c for c in M.cases(M.LARGE) if c.mask == "edges"])
    calls2, bad2 = M.run_cases(host, [c for c in M.cases(M.LARGE) if c.mask != "edges"], all_caps=False)
    assert calls and calls2 and bad + bad2 == [], (bad + bad2)[:5]


def test_host_select_refusals():
    mask = np.zeros(1024, dtype=np.uint64)
    d = np.zeros(64, dtype=np.uint8)
    out = np.full(4, CANARY, dtype=np.uint64)
    op = out.ctypes.data_as(u64p)
    E = _capi.KRK_EINVAL
    assert lib.krk_ring_select(d.ctypes.data_as(u8p), 2, None, 0, None, op, None, 0, op) == E
    assert lib.krk_ring_select(None, 2, mask.ctypes.data_as(u64p), 0, None, op, None, 0, op) == E
    assert lib.krk_ring_select(d.ctypes.data_as(u8p), 2, mask.ctypes.data_as(u64p), 0, None, None, None, 0, op) == E
    assert lib.krk_ring_select(d.ctypes.data_as(u8p), 2, mask.ctypes.data_as(u64p), 0, None, op, None, 0, None) == E
    assert lib.krk_ring_select(d.ctypes.data_as(u8p), 2, mask.ctypes.data_as(u64p), 0, None, op, None, 1, op) == E  # NULL idx, cap 1
    assert (out == CANARY).all()
    # n == 0 with NULL arrays: the count is written, 0
    assert lib.krk_ring_select(None, 0, mask.ctypes.data_as(u64p), 1, None, None, None, 0, op) == _capi.KRK_OK
    assert out.tolist() == [0] + [int(CANARY)] * 3


# ------------------------------------------------------------------ the Python surface
class _Digest:
    def __init__(self, hex_):
        self.hex = hex_

    def ShardID(self):
        return self.hex[:4]


def _ring(orc, labels, healthy, max_replica):
    """A Ring whose owner table comes from the device when there is one, else from the oracle."""
    from kraken_amd import device as D
    ring = hashring.Ring(labels, [l for l, h in zip(labels, healthy) if h], max_replica)
    if D.device_count() == 0:
        ring._table = table(orc, labels, healthy, max_replica)
    return ring


def test_ring_masks_and_owns_batch(orc):
    labels = labels_of(5)
    healthy = health_of(5, "one down")
    ring = _ring(orc, labels, healthy, 3)
    rng = np.random.default_rng(7)
    d = rng.integers(0, 256, size=(200, 32), dtype=np.uint8)
    bits = ring.OwnsBatch(labels[1], d)
    want = [labels[1] in ring.Locations(_Digest(bytes(x).hex())) for x in d]
    assert np.unpackbits(bits.view(np.uint8), bitorder="little")[:200].astype(bool).tolist() == want
    assert not ring.ShardMaskOwns("nobody.kraken.test:1").any()
    other = _ring(orc, labels[:4], healthy[:4], 3)
    sel, idx = ring.Select(d, ring.ShardMaskMoved(other))
    want = [i for i, x in enumerate(d) if set(ring.Locations(_Digest(bytes(x).hex()))) !=
            set(other.Locations(_Digest(bytes(x).hex())))]
    assert idx.tolist() == want and 0 < len(want) < 200
    assert np.flatnonzero(np.unpackbits(sel.view(np.uint8), bitorder="little")).tolist() == want


def test_force_cleanup_plan_equals_maybe_delete_name_by_name(orc):
    labels, healthy = labels_of(5), health_of(5, "all")
    ring = _ring(orc, labels, healthy, 3)
    addr = labels[2]
    rng = np.random.default_rng(11)
    names = [hashlib.sha256(bytes([i & 255, i >> 8])).hexdigest() for i in range(300)]
    names[17] = names[17][:-1] + "g"  # not hex
    names[203] = names[203][:40]      # not 64 characters
    names[250] = names[250].upper()   # hex.DecodeString takes upper case
    now, ttl = 1_700_000_000, 3600
    mtimes = now - rng.integers(0, 2 * ttl, size=300)
    mtimes[5] = now - ttl  # not expired: the comparison is strict
    owned = next(i for i, n in enumerate(names) if i not in (17, 203) and addr in ring.Locations(_Digest(n.lower())))
    mtimes[owned] = now - ttl - 1  # expired and owned: deleted all the same

    deleted, errs = [], []  # forceCleanupHandler's loop over maybeDelete, a name at a time
    for i, name in enumerate(names):
        if len(name) != 64 or any(c not in "0123456789abcdefABCDEF" for c in name):
            errs.append(name)
            continue
        expired = now - int(mtimes[i]) > ttl
        owns_ = addr in set(ring.Locations(_Digest(name.lower())))
        if expired or not owns_:
            deleted.append(i)
    idx, errors = castore.force_cleanup_plan(names, mtimes, now, ttl, ring, addr)
    assert idx.tolist() == deleted and owned in deleted
    assert (5 in deleted) == (addr not in ring.Locations(_Digest(names[5])))
    assert [e.split(":")[0] for e in errors] == errs == [names[17], names[203]]
    assert errors[0] == f"{names[17]}: parse digest: invalid sha256: hex: encoding/hex: invalid byte: U+0067 'g'"
    assert errors[1] == f'{names[203]}: parse digest: invalid sha256: expected 64 characters, got 40 from "{names[203]}"'
    assert 0 < len(deleted) < 298
    # every name bad: nothing to select, every name an error
    idx, errors = castore.force_cleanup_plan(["zz", ""], [0, 0], now, ttl, ring, addr)
    assert idx.size == 0 and len(errors) == 2


def test_ring_select_dev_without_a_device(data):
    """A refusal needs no device; a real call needs a gfx950 device (KRK_ENODEV here when there is
    none -- with one, tests/test_gpu_ring_select_matrix.py) and the host form still answers."""
    from kraken_amd import device as D
    mask = data.masks["random"]
    out = np.full(8, CANARY, dtype=np.uint64)
    o = out.ctypes.data
    d = data.digests[:65]
    assert lib.krk_ring_select_dev(d.ctypes.data, 65, None, 0, None, o, None, 0, o + 32, None) == _capi.KRK_EINVAL
    assert lib.krk_ring_select_dev(d.ctypes.data, 65, mask.ctypes.data_as(u64p), 0, None, o, None, 3, o + 32,
                                   None) == _capi.KRK_EINVAL
    if D.device_count() == 0:
        rc = lib.krk_ring_select_dev(d.ctypes.data, 65, mask.ctypes.data_as(u64p), 0, None, o, None, 0, o + 32, None)
        assert rc == _capi.KRK_ENODEV
        assert lib.krk_ring_select_dev(None, 0, mask.ctypes.data_as(u64p), 0, None, None, None, 0, o, None) == _capi.KRK_ENODEV
        assert (out == CANARY).all()
        bits, idx = hashring.Ring.Select(d, mask)
        want = data.reference(M.Case(65, "random", False, False))
        assert np.array_equal(bits, want[0]) and np.array_equal(idx, want[1])
