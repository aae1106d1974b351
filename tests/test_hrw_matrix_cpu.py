"""The HRW matrix helper (tests/hrw_matrix.py) checked where no GPU is: the two murmur3
references agree on every message the GPU tests hash, the crafted preimages hit their Sums,
the oracle's score stands against a 50-digit reference, and the case builders are what they
say they are -- before tests/test_gpu_hrw_edges.py trusts any of it."""
import json
import math
import os

import numpy as np
import pytest

from tests import hrw_matrix as M

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))


@pytest.fixture(scope="module")
def targets():
    return M.sum_targets(), M.sum_messages()


def test_two_murmur_references_agree(orc):
    """The oracle's switch-based tail and the loop-based restatement: every message of the
    seam matrix (every length 0..66), and the golden vectors."""
    keys, labels = M.seam_matrix()
    lengths = set()
    for k in keys:
        for l in labels:
            msg = k + l
            lengths.add(len(msg))
            assert orc.murmur3_h1(msg) == M.murmur3_h1(msg), (len(k), len(l))
    assert lengths == set(range(67))
    for s, h in GOLD["kat"]["murmur3_h1"]:
        assert orc.murmur3_h1(s.encode()) == M.murmur3_h1(s.encode()) == int(h, 16), s


def test_preimages_hit_their_targets(orc, targets):
    """Every 16-byte preimage hashes to its target under both references -- as one message,
    which is what a key against the empty label and a 5 / 11 split between key and label
    both hash."""
    tg, msgs = targets
    assert len(tg) == len(msgs) == 12 + 6 + 53 + 52 + 256
    assert len(set(msgs)) == len(msgs)
    for (name, t), m in zip(tg, msgs):
        assert len(m) == 16
        assert M.murmur3_h1(m) == t, name
        assert orc.murmur3_h1(m) == t, name
        assert orc.murmur3_h1(m[:5] + m[5:]) == t, name
    # the free half is free: other choices of it reach the same Sum with other messages
    for b in (0, 1, M.M64):
        m = M.murmur_preimage16(0x0123456789ABCDEF, b)
        assert M.murmur3_h1(m) == orc.murmur3_h1(m) == 0x0123456789ABCDEF


def test_targets_are_the_edges_they_name(targets):
    tg, _ = targets
    by = dict(tg)
    assert len(by) == len(tg)
    rehash = [t for n, t in tg if n.startswith("rehash")]
    assert len(rehash) == 12 and all(t & M.M53 == 0 for t in rehash) and rehash[-1] == 0
    assert all(M.u64_value(t) != 0 for t in rehash)
    assert all(t & M.M53 != 0 for n, t in tg if not n.startswith("rehash") and not n.startswith("random"))
    assert by["val 1"] & M.M53 == 1 and by["val 2^53-1"] & M.M53 == M.M53
    # both sides of go_log's fold: FOLD / 2^53 is exactly the double sqrt(2)/2 the kernel compares with
    assert M.FOLD / 2.0 ** 53 == 0.70710678118654752440084436210484904 == 0.7071067811865476
    assert (M.FOLD - 1) / 2.0 ** 53 == 0.7071067811865475 < 0.7071067811865476
    assert by["fold"] & M.M53 == M.FOLD and by["fold-1"] & M.M53 == M.FOLD - 1
    for k in range(53):  # f == 0 in the folded branch: the fraction is exactly 0.5
        assert math.frexp((by[f"2^{k}"] & M.M53) / 2.0 ** 53) == (0.5, k - 52)
    for k in range(52):
        assert math.frexp((by[f"3*2^{k}"] & M.M53) / 2.0 ** 53)[0] == 0.75


def test_oracle_score_against_decimal(orc, targets):
    """-w / ln(val / 2^53) at 50 digits against the oracle's score for every crafted Sum, whole
    as the key and split 5 / 11: within 2 ulp (1 ulp is the error bound documented for Go's
    log, FreeBSD e_log.c; the rest the roundings of the division and of the conversion)."""
    tg, msgs = targets
    worst = (0.0, None)
    for (name, t), m in zip(tg, msgs):
        val = M.u64_value(t)
        assert 0 < val <= M.M53
        for w in (100, 800):
            want = M.score_decimal(val, w)
            whole = orc.lib().orc_hrw_score(m.hex().encode(), 32, b"", 0, w)
            split = orc.lib().orc_hrw_score(m[:5].hex().encode(), 10, m[5:], 11, w)
            assert split.hex() == whole.hex(), name
            assert math.isfinite(whole) and whole > 0, name
            off = M.ulps_off(whole, want)
            worst = max(worst, (off, name))
            assert off <= 2.0, (name, w, whole, str(want), off)
    print("worst distance from the 50-digit score: %.3f ulp (%s)" % worst)


def test_seam_matrix_is_complete():
    keys, labels = M.seam_matrix()
    assert [len(k) for k in keys] == list(range(34)) == [len(l) for l in labels]
    assert M.seam_pairs(keys, labels) == {(r, s) for r in range(16) for s in range(16)}
    assert {len(k) + len(l) for k in keys for l in labels} == set(range(67))
    for b in keys + labels:
        assert len(b) < 1 or any(x >= 0x80 for x in b)
        assert len(b) < 2 or 0 in b


def test_tile_counts_and_builders():
    assert [M.keys_per_block(n) for n in M.B_NODES] == [63, 40, 16, 16, 4, 2, 1, 1, 1]
    assert M.tile_key_counts(65) == [1, 62, 63, 64, 127]
    assert M.tile_key_counts(2048) == [1, 2, 3, 5]
    assert M.tile_key_counts(2049) == M.tile_key_counts(4096) == [1, 3]
    keys, labels, weights = M.tile_case(100)
    assert len(keys) == 81 and len(set(labels)) == 100 and len({len(l) for l in labels}) > 1
    assert set(weights) == {100, 200, 400, 800}


def test_tied_labels_are_byte_equal():
    _, labels, weights = M.tie_case()
    assert len(labels) == 70 and set(weights) == {100}
    for a, b in M.TIE_PAIRS:
        assert a < b and labels[a] == labels[b]
    assert len(set(labels)) == 70 - len(M.TIE_PAIRS)


def test_bad_keys_are_invalid_hex(orc):
    keys, bad = M.mixed_keys()
    assert len(keys) == 200 and bad.sum() == 29
    assert bad.nonzero()[0].tolist() == list(range(1, 200, 7))
    kinds = set()
    for k, b in zip(keys, bad):
        assert M.is_valid_hex(k) != b, k
        if b:
            with pytest.raises(ValueError):
                bytes.fromhex(k)
            assert math.isnan(orc.lib().orc_hrw_score(k.encode(), len(k), b"x", 1, 100)), k
            kinds.add("g0" if k == "g0" else "odd" if len(k) % 2 else
                      "first" if not M.is_valid_hex(k[0] + "0") else "last")
    assert kinds == set(M.BAD_KINDS)
    assert "" == b"".hex() and M.is_valid_hex("")


def test_healthy_sets_and_replica_counts():
    assert [h.tolist() for h in M.healthy_sets(1)] == [[1], [0]]
    assert [h.tolist() for h in M.healthy_sets(2)] == [[1, 1], [0, 0], [1, 0], [0, 1]]
    sets = M.healthy_sets(65)
    assert [int(h.sum()) for h in sets] == [65, 0, 1, 1, 1, 64]
    assert [int(h.argmax()) for h in sets[2:5]] == [0, 32, 64]
    assert M.replica_counts(65) == [-2 ** 31, -1, 0, 1, 64, 65, 66]
    assert M.replica_counts(1) == [-2 ** 31, -1, 0, 1, 2]


def test_oracle_orders_and_ties(orc):
    """The raw-byte oracle caller equals the str one, and resolves an exact tie by index."""
    keys, labels, weights = M.tie_case()
    order, scores = M.orc_ordered(orc, keys, labels, weights)
    for i in (0, 7, 63):
        o, s = orc.hrw_ordered(keys[i].hex(), [l.decode() for l in labels], weights, with_scores=True)
        assert order[i].tolist() == o and scores[i].tobytes() == np.asarray(s).tobytes()
    pos = np.argsort(order, axis=1)
    for a, b in M.TIE_PAIRS:
        assert (scores[:, a].view(np.uint64) == scores[:, b].view(np.uint64)).all()
        assert (pos[:, b] == pos[:, a] + 1).all()
