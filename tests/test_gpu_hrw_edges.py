"""The HRW scoring kernel and the ring filter (hrw_place.hip) at their structural edges,
through the C ABI with raw-byte labels (tests/hrw_matrix.py): every score bit for bit and
every order exactly against the oracle, no case sampled.

 A  the key | label seam at every byte of a 16-byte block with every tail residue;
 B  tile geometry: 65..4096 nodes (64..1 keys a workgroup), batches around one tile;
 C  n_out from 0 to 4096 (the -1 padding, scores alone);
 D  exact ties, NaN rows among good ones, weight extremes, hex case, the empty key;
 E  chosen murmur3 Sums (crafted preimages) through the scoring kernel: the rehash branch
    and go_log at its fold, at powers of two, at val = 1 and val = 2^53 - 1;
 F  the ring filter: whole owner tables over health sets and MaxReplica edges, rings of more
    than 255 nodes, and the refusal of owner counts past a byte."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from kraken_amd import device as D
from kraken_amd._capi import KRK_EHEX, KRK_EINVAL, KRK_ERANGE, KRK_OK, lib
from tests import hrw_matrix as M

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check(orc, keys, labels, weights, what):
    """One krk_hrw_ordered call: full orders and all scores equal the oracle's."""
    N = len(labels)
    rc, order, scores = M.krk_ordered(keys, labels, weights, N)
    assert rc == KRK_OK, (what, rc, lib.krk_last_error())
    want_o, want_s = M.orc_ordered(orc, keys, labels, weights)
    bad = np.argwhere(_bits(scores) != _bits(want_s))
    assert bad.size == 0, (what, "scores", bad[:5].tolist(), [(scores[i, j], want_s[i, j]) for i, j in bad[:5]])
    bad = np.nonzero((order != want_o).any(axis=1))[0]
    assert bad.size == 0, (what, "orders", bad[:5].tolist(), order[bad[0]].tolist(), want_o[bad[0]].tolist())
    return order, scores


# ------------------------------------------------------------------ A
@pytest.mark.parametrize("weights", ["all 100", "mixed"])
def test_a_seam_matrix(orc, weights):
    """34 keys of 0..33 bytes x 34 labels of 0..33 bytes in ONE call: 1,156 messages of
    0..66 bytes, every n & 15 with the seam between key and label at every block byte."""
    keys, labels = M.seam_matrix()
    w = [100] * 34 if weights == "all 100" else M.mixed_weights(34)
    _check(orc, keys, labels, w, "A " + weights)


# ------------------------------------------------------------------ B
@pytest.mark.parametrize("n_nodes", M.B_NODES)
def test_b_tile_geometry(orc, n_nodes):
    """kpb = min(64, 4096 // N) keys a workgroup: batches of less than a tile, a tile, a tile
    and a ragged one, two tiles and one."""
    keys, labels, weights = M.tile_case(n_nodes)
    for c in M.tile_key_counts(n_nodes):
        _check(orc, keys[:c], labels, weights, f"B N={n_nodes} keys={c}")


@pytest.mark.parametrize("n_nodes", [0, 4097])
def test_b_node_count_out_of_range_is_refused(n_nodes):
    """No node, or more than an LDS tile holds: KRK_EINVAL, outputs untouched (upload_nodes
    refuses before any upload or launch)."""
    keys, labels, weights = M.plain_case(3, 5, 20)
    order = np.full((5, 3), -7, dtype=np.int32)
    scores = np.full((5, 3), -7.0, dtype=np.float64)
    rc, order, scores = M.krk_ordered(keys, labels, weights, 3, order=order, scores=scores, n_nodes=n_nodes)
    assert rc == KRK_EINVAL
    assert (order == -7).all() and (scores == -7.0).all()


# ------------------------------------------------------------------ C
@pytest.mark.parametrize("n_nodes", [5, 70])
def test_c_n_out(orc, n_nodes):
    """Rows are n_out wide: the first min(n_out, N) oracle entries, then -1; the scores do not
    depend on n_out."""
    keys, labels, weights = M.plain_case(n_nodes, 150, 30 + n_nodes)
    want_o, want_s = M.orc_ordered(orc, keys, labels, weights)
    for n_out in (1, n_nodes - 1, n_nodes, n_nodes + 1, 4096):
        rc, order, scores = M.krk_ordered(keys, labels, weights, n_out)
        assert rc == KRK_OK, (n_out, lib.krk_last_error())
        m = min(n_out, n_nodes)
        assert order.shape == (150, n_out)
        assert np.array_equal(order[:, :m], want_o[:, :m]), n_out
        assert (order[:, m:] == -1).all(), n_out
        assert np.array_equal(_bits(scores), _bits(want_s)), n_out
    order = np.full((150, 2), -7, dtype=np.int32)
    scores = np.full((150, n_nodes), -7.0, dtype=np.float64)
    rc, order, scores = M.krk_ordered(keys, labels, weights, 4097, order=order, scores=scores)
    assert rc == KRK_EINVAL and (order == -7).all() and (scores == -7.0).all()


@pytest.mark.parametrize("n_nodes", [5, 70])
def test_c_n_out_zero(orc, n_nodes):
    """n_out == 0 asks for no order: with scores_out the scores are the oracle's, without it
    the call does nothing and succeeds."""
    keys, labels, weights = M.plain_case(n_nodes, 150, 30 + n_nodes)
    _, want_s = M.orc_ordered(orc, keys, labels, weights)
    rc, order, scores = M.krk_ordered(keys, labels, weights, 0)
    assert rc == KRK_OK and order.shape == (150, 0)
    assert np.array_equal(_bits(scores), _bits(want_s))
    rc, _, _ = M.krk_ordered(keys, labels, weights, 0, want_scores=False)
    assert rc == KRK_OK


# ------------------------------------------------------------------ D
def test_d_exact_ties_go_to_the_lower_index(orc):
    keys, labels, weights = M.tie_case()
    order, scores = _check(orc, keys, labels, weights, "D ties")
    pos = np.argsort(order, axis=1)  # pos[i, j]: the rank of node j for key i
    for a, b in M.TIE_PAIRS:
        assert np.array_equal(_bits(scores[:, a]), _bits(scores[:, b]))
        assert (pos[:, a] + 1 == pos[:, b]).all(), (a, b)


def test_d_all_weights_zero(orc):
    keys, labels, _ = M.plain_case(70, 64, 42)
    order, scores = _check(orc, keys, labels, [0] * 70, "D zero weights")
    assert (_bits(scores) == 0).all()  # +0.0, sign bit included
    assert (order == np.arange(70)).all()


def test_d_weight_extremes(orc):
    keys, labels, _ = M.plain_case(len(M.EXTREME_WEIGHTS), 100, 43)
    _, scores = _check(orc, keys, labels, list(M.EXTREME_WEIGHTS), "D weight extremes")
    assert (scores[:, 0] < 0).all() and (scores[:, 1] < 0).all() and (_bits(scores[:, 2]) == 0).all()
    assert (scores[:, 3:] > 0).all() and np.isfinite(scores).all()


@pytest.mark.parametrize("n_nodes", [3, 100])
def test_d_bad_keys_among_good_ones(orc, n_nodes):
    """Every seventh key is not valid hex: its row is NaN scores and the identity order, the
    good keys of the same tile are untouched by it, and the call says KRK_EHEX."""
    keys, bad = M.mixed_keys()
    _, labels, weights = M.plain_case(n_nodes, 1, 44)
    rc, order, scores = M.krk_ordered(keys, labels, weights, n_nodes)
    assert rc == KRK_EHEX
    assert np.isnan(scores[bad]).all() and (order[bad] == np.arange(n_nodes)).all()
    good = [k for k, b in zip(keys, bad) if not b]
    want_o, want_s = M.orc_ordered(orc, good, labels, weights)
    assert np.array_equal(_bits(scores[~bad]), _bits(want_s))
    assert np.array_equal(order[~bad], want_o)
    # the oracle treats the bad keys alike
    bo, bs = M.orc_ordered(orc, [k for k, b in zip(keys, bad) if b], labels, weights)
    assert np.isnan(bs).all() and (bo == np.arange(n_nodes)).all()


def test_d_hex_case_and_empty_key(orc):
    keys, labels, weights = M.plain_case(7, 40, 45)
    lower = [k.hex() for k in keys]
    assert any(c in "abcdef" for k in lower for c in k)
    _, want = _check(orc, lower, labels, weights, "D lower case")
    mixed = [k.upper() if i % 2 else "".join(c.upper() if j % 3 else c for j, c in enumerate(k))
             for i, k in enumerate(lower)]
    rc, order, scores = M.krk_ordered(mixed, labels, weights, 7)
    assert rc == KRK_OK and np.array_equal(_bits(scores), _bits(want))
    # "" decodes to no bytes: the label alone is hashed; alone in a call and among others
    order, scores = _check(orc, [""], labels, weights, "D empty key alone")
    _, s2 = _check(orc, [lower[0], "", lower[1]], labels, weights, "D empty key among others")
    assert np.array_equal(_bits(s2[1]), _bits(scores[0]))
    for j, l in enumerate(labels):
        val = M.u64_value(M.murmur3_h1(l))
        assert M.ulps_off(float(scores[0, j]), M.score_decimal(val, weights[j])) <= 2.0


# ------------------------------------------------------------------ E
@pytest.fixture(scope="module")
def sums():
    return M.sum_targets(), M.sum_messages()


@pytest.mark.parametrize("weights", [(100, 800), (800, 100)])
def test_e_chosen_sums_whole_key(orc, sums, weights):
    """Each crafted 16-byte message as a 32-digit key against node 0 with the EMPTY label (and
    one ordinary node): hrw_score sees exactly the chosen Sum."""
    tg, msgs = sums
    labels = [b"", M.ORDINARY_LABEL]
    _, scores = _check(orc, msgs, labels, list(weights), "E whole")
    for (name, t), s in zip(tg, scores[:, 0]):
        assert np.isfinite(s) and s > 0, name
        assert M.ulps_off(float(s), M.score_decimal(M.u64_value(t), weights[0])) <= 2.0, name
    fold = {n: s for (n, _), s in zip(tg, scores[:, 0])}
    assert fold["fold"] != fold["fold-1"]


def test_e_chosen_sums_split_key_and_label(orc, sums):
    """The same messages split 5 / 11 between the key and a raw-byte label: key i against node
    i is message i, the same score bits as whole; the other pairs are ordinary messages."""
    tg, msgs = sums
    n = len(msgs)
    keys, labels = [m[:5] for m in msgs], [m[5:] for m in msgs]
    weights = [100 if i % 2 == 0 else 800 for i in range(n)]
    _, scores = _check(orc, keys, labels, weights, "E split")
    for w in (100, 800):
        _, whole = M.orc_ordered(orc, msgs, [b"", M.ORDINARY_LABEL], [w, 900 - w])
        pick = np.arange(n)[np.array(weights) == w]
        assert np.array_equal(_bits(scores[pick, pick]), _bits(whole[pick, 0])), w


# ------------------------------------------------------------------ F
def _owner_table(labels, weights, healthy, max_replica, locs=None, counts=None):
    nt = M.Nodes(labels, weights)
    row = max(1, max_replica)
    if locs is None:
        locs = np.full((65536, row), -7, dtype=np.int32)
        counts = np.full(65536, 0xEE, dtype=np.uint8)
    h = np.ascontiguousarray(healthy, dtype=np.uint8)
    rc = lib.krk_ring_owner_table(C.byref(nt.s), M._p(h, C.c_uint8), max_replica, M._p(locs, C.c_int32),
                                  M._p(counts, C.c_uint8))
    return rc, locs, counts


@pytest.mark.parametrize("n_nodes", [1, 2, 65])
def test_f_owner_tables_exhaustive(orc, n_nodes):
    """All 65,536 rows of krk_ring_owner_table -- owners, -1 padding, counts -- against the
    oracle's table, for every health set x MaxReplica edge (negative included)."""
    labels, weights = M.ring_labels(n_nodes), [100] * n_nodes
    full, _ = M.orc_owner_table(orc, labels, weights, np.ones(n_nodes, np.uint8), n_nodes)  # the HRW orders
    rank = np.argsort(full, axis=1)
    combos = [(h, r) for h in M.healthy_sets(n_nodes) for r in M.replica_counts(n_nodes)]
    with ThreadPoolExecutor(8) as pool:  # the oracle's tables: plain C loops that hold no lock
        wants = list(pool.map(lambda c: M.orc_owner_table(orc, labels, weights, *c), combos))
    for (healthy, max_replica), (want_l, want_c) in zip(combos, wants):
        what = (healthy.tolist(), max_replica)
        rc, locs, counts = _owner_table(labels, weights, healthy, max_replica)
        assert rc == KRK_OK, what
        bad = np.nonzero((locs != want_l).any(axis=1) | (counts != want_c))[0]
        assert bad.size == 0, (what, bad[:5], locs[bad[:3]], want_l[bad[:3]])
        if healthy.sum() == 1:  # one healthy node is the one owner whichever rank it has
            j = int(healthy.argmax())
            assert (counts == 1).all() and (locs[:, 0] == j).all() and (locs[:, 1:] == -1).all(), what
            assert n_nodes < 65 or len(set(rank[:, j].tolist())) == n_nodes, "every rank occurs"
        if not healthy.any():
            assert (counts == 1).all() and (locs[:, 0] == full[:, 0]).all(), what


def _locations(labels, healthy, max_replica, digests, locs=None, counts=None):
    nt = M.Nodes(labels, [100] * len(labels))
    n, row = len(digests), max(1, max_replica)
    if locs is None:
        locs = np.full((n, row), -7, dtype=np.int32)
        counts = np.full(n, 0xEE, dtype=np.uint8)
    h = np.ascontiguousarray(healthy, dtype=np.uint8)
    d = np.ascontiguousarray(digests)
    rc = lib.krk_ring_locations(M._p(d, C.c_uint8), n, C.byref(nt.s), M._p(h, C.c_uint8), max_replica,
                                M._p(locs, C.c_int32), M._p(counts, C.c_uint8))
    return rc, locs, counts


@pytest.mark.parametrize("n_nodes,max_replica", [(300, 255), (255, 300)])
def test_f_255_owners_a_shard(orc, n_nodes, max_replica):
    """The most owners a count can say: 300 nodes with MaxReplica 255, and 255 nodes with
    MaxReplica 300, every node healthy.  Every count is 255 and the rows are the first 255
    of the oracle's order (then -1)."""
    labels = M.ring_labels(n_nodes)
    digests = M.ring_digests()
    rc, locs, counts = _locations(labels, np.ones(n_nodes, np.uint8), max_replica, digests)
    assert rc == KRK_OK, lib.krk_last_error()
    assert (counts == 255).all()
    want_o, _ = M.orc_ordered(orc, [bytes(d[:2]) for d in digests], labels, [100] * n_nodes)
    assert np.array_equal(locs[:, :255], want_o[:, :255])
    assert (locs[:, 255:] == -1).all() and locs.shape[1] == max_replica


@pytest.mark.parametrize("n_nodes,max_replica", [(300, 256), (4096, 2 ** 31 - 1)])
def test_f_more_than_255_owners_is_refused(n_nodes, max_replica):
    """min(MaxReplica, N) > 255 owners do not fit a count byte (a wrapped count would go out,
    and the oracle wraps alike): all four ring entry points return KRK_ERANGE before anything
    is launched or written -- every output keeps its fill.  The outputs are sized for the call
    where that is possible at all (MaxReplica 256)."""
    labels = M.ring_labels(n_nodes)
    healthy = np.ones(n_nodes, np.uint8)
    digests = M.ring_digests()
    n = len(digests)
    row = max_replica if max_replica <= 256 else 4
    locs = np.full((n, row), -7, dtype=np.int32)
    counts = np.full(n, 0xEE, dtype=np.uint8)
    rc, locs, counts = _locations(labels, healthy, max_replica, digests, locs, counts)
    assert rc == KRK_ERANGE, ("krk_ring_locations", rc, lib.krk_last_error())
    assert (locs == -7).all() and (counts == 0xEE).all()

    tl = np.full((65536, row), -7, dtype=np.int32)
    tc = np.full(65536, 0xEE, dtype=np.uint8)
    rc, tl, tc = _owner_table(labels, [100] * n_nodes, healthy, max_replica, tl, tc)
    assert rc == KRK_ERANGE, ("krk_ring_owner_table", rc, lib.krk_last_error())
    assert (tl == -7).all() and (tc == 0xEE).all()

    nt = M.Nodes(labels, [100] * n_nodes)
    dbuf = D.DeviceBuffer(n * 32)
    dbuf.from_host(digests.reshape(-1))
    hp = M._p(healthy, C.c_uint8)
    for name, item in (("krk_ring_locations_dev", 4), ("krk_ring_locations_u8_dev", 1)):
        lb, cb = D.DeviceBuffer(n * row * item), D.DeviceBuffer(n)
        lb.from_host(np.full(n * row * item, 0xAA, dtype=np.uint8))
        cb.from_host(np.full(n, 0xEE, dtype=np.uint8))
        rc = getattr(lib, name)(dbuf.ptr, n, C.byref(nt.s), hp, max_replica, lb.ptr, cb.ptr, None)
        D.synchronize()
        assert rc == KRK_ERANGE, (name, rc, lib.krk_last_error())
        assert (lb.to_host(np.uint8) == 0xAA).all() and (cb.to_host(np.uint8) == 0xEE).all(), name
