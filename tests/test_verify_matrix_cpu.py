"""The verify matrix harness (tests/verify_matrix.py) checked where no GPU is: its builders give
the counts the module states, and groups A - D, blob by blob through krk_piece_bitfield -- the
host packer piece_bitfield.hip is documented to equal -- pass the same comparison against
numpy.packbits: the expected values, the layouts and the mismatch reporting are right before a
kernel is involved."""
import numpy as np
import pytest

from tests import verify_matrix as M
from tests.verify_cache import ref_words


@pytest.fixture(scope="module")
def host():
    return M.HostBackend()


def test_group_a_and_b_builders():
    b = M.batch_a()
    assert b.np.tolist() == list(M.A_PIECES) and b.pieces == 49_153 and (b.L % M.P == 7).all()
    assert np.diff(b.word_off).tolist() == [64, 64, 65, 128, 128, 129, 193] and b.words == 771
    bad = M.chosen_a(b)
    for i, n in enumerate(M.A_PIECES):
        mine = np.nonzero(bad[b.first[i]:b.first[i + 1]])[0]
        assert {p for p in (0, 63, 64, 4095, 4096, n - 1) if p < n} <= set(mine.tolist())
        groups = np.bincount(mine // 4096, minlength=(n + 4095) // 4096)  # a bad piece in every 64-word group
        assert (groups >= 1).all() and mine.size <= 6 + groups.size
    mixed, empty, one = M.batches_b()
    assert mixed.np.tolist() == [0, 0, 0, 5, 0, 0, 64, 0, 65, 0, 0] and mixed.words == 1 + 1 + 2
    assert mixed.word_off.tolist() == [0, 0, 0, 0, 1, 1, 1, 2, 2, 4, 4, 4]
    assert empty.n == 5 and empty.pieces == empty.words == empty.exp_size == 0
    assert one.np.tolist() == [1] and one.words == 1
    assert np.nonzero(M.chosen_b(mixed))[0].tolist() == [0, 4, 5, 9, 68, 69, 73, 132, 133]


def test_group_c_builder():
    e = M.empty_c()
    assert int(e.sum()) == 276 and e[[0, 1, 2, 999, 131072, 131075, 262143, 262146, 262997, 262999]].all()
    assert not e[[3, 131071, 131076, 262142, 262147, 262996]].any()
    b = M.batch_c()
    assert b.n == 263_000 and b.words == 262_724 and b.pieces == 525_448
    assert b.words > M.STRIDE_UNITS == 262_144 and b.n > M.STRIDE_UNITS
    assert np.array_equal(b.np[~e], (1 + np.arange(b.n) % 3)[~e]) and (b.np[e] == 0).all()
    assert (b.L % M.P != 0).mean() > 0.9  # a short last piece on most
    assert (b.off + b.L <= M.BUF_BYTES).all() and np.unique(b.off).size > 200_000
    share = M.bad_c(b).mean()
    assert 0.068 < share < 0.072
    # the count kernel's second pass starts inside a run of empty blobs, and the word kernel's
    # second pass at a word whose owner is found past more than 260 empty blobs
    w = M.STRIDE_UNITS
    assert e[w - 1:w + 3].all() and not e[w - 2] and not e[w + 3]
    owner = int(np.searchsorted(b.word_off, w, side="right")) - 1
    assert b.np[owner] > 0 and b.word_off[owner] == w and owner - w == int(e[:owner].sum()) > 260


def test_group_d_and_e_builders():
    cases = M.cases_d()
    assert len(cases) == 8
    a, bm = M.batch_a(), M.batches_b()[0]
    for k, (b, bad) in enumerate(cases):
        base = a if k < 4 else bm
        assert np.array_equal(b.L, base.L) and np.array_equal(b.off, base.off) and bad.size == base.pieces
        live = b.np > 0
        if "permuted" in b.label:
            assert (np.diff(b.sums_off[live]) < 0).any()
        else:
            assert (np.diff(b.sums_off[live]) > 0).all()
        gaps = b.exp_size - b.pieces - (1000 if "1000" in b.label else 0)
        assert (gaps >= int(live.sum()) - 1) if "gapped" in b.label else gaps == 0
        assert (int(b.sums_off[live].min()) == 1000) == ("1000" in b.label)
        # the gap value reaches exactly the entries no piece owns
        e0, e1 = b.expected(np.zeros(M.BUF_BYTES, np.uint8), bad, 0), b.expected(np.zeros(M.BUF_BYTES, np.uint8), bad, 7)
        assert int((e0 != e1).sum()) == b.exp_size - b.pieces
    e = M.batch_e()
    assert e.n == 1031 > 4 * M.DIGEST_BLOCK and e.L.min() == 0 and e.L.max() == 200 and int((e.L == 0).sum()) == 6
    true, exp, ok = M.digests_e(M.make_buffer(), e)
    diff = true ^ exp
    assert int((~ok).sum()) == 32 + 5 and np.count_nonzero(diff) == 37
    for k in range(32):  # one bit of one byte each: every dword of both halves decides a blob alone
        assert np.nonzero(diff[32 + k])[0].tolist() == [k] and diff[32 + k, k] == 1 << (k % 8)
    assert sorted({k // 4 for k in range(32)}) == list(range(8))
    assert all(np.nonzero(diff[i])[0].tolist() == [13] for i in M.E_BYTE13)
    assert ok[e.L == 0][1:].all() and not ok[0]  # the empty blobs verify, but blob 0 (byte 13)


def test_want_is_packbits_blob_by_blob():
    """Batch.want's one ref_words call over the whole batch equals one call a blob."""
    b = M.batches_b()[0]
    bad = M.chosen_b(b)
    words, n_bad = b.want(bad)
    per_blob = [ref_words(~bad[b.first[i]:b.first[i + 1]]) for i in range(b.n)]
    assert np.array_equal(words, np.concatenate(per_blob))
    assert n_bad.tolist() == [0, 0, 0, 2, 0, 0, 3, 0, 4, 0, 0]


@pytest.mark.parametrize("group,count", [("A", 21), ("B", 3 * 11 + 4 * 5 + 3), ("C", 263_000), ("D", 2 * 4 * (7 + 11))])
def test_groups_pass_on_the_host_packer(host, group, count):
    n, bad = M.run_group_counted(group, host)
    assert n == count
    assert bad == []


def test_reporting_names_the_blob_the_word_and_the_count(host):
    b = M.batches_b()[0]
    bad = M.chosen_b(b)
    want_bits, want_bad = b.want(bad)
    bits, n_bad, _, spare = host.verify(b, b.expected(host.host, bad))
    assert M.compare("X", b, (bits, n_bad, None, spare), want_bits, want_bad) == []
    bits, n_bad = bits.copy(), n_bad.copy()
    bits[3] ^= 1 << 5   # blob 8 (65 pieces), its second word
    n_bad[10] = 1       # a trailing empty blob
    out = M.compare("X", b, (bits, n_bad, None, spare), want_bits, want_bad)
    assert len(out) == 2
    assert out[0][0].startswith("X blob 8 (65 pieces") and "word 1 (batch word 3)" in out[0][0] and out[0][1] ^ out[0][2] == 32
    assert out[1] == ("X blob 10 (0 pieces) n_bad", 1, 0)
    # a piece the expectation calls good although its expected sum is flipped
    wrong = bad.copy()
    wrong[0] = False
    out = M.compare("X", b, host.verify(b, b.expected(host.host, bad)), *b.want(wrong))
    assert [d.split(" word ")[0] for d, _, _ in out] == ["X blob 3 (5 pieces, sums at 0)", "X blob 3 (5 pieces) n_bad"]
