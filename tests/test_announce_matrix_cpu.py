"""The announce round's host forms (krk_announce_round, krk_announce_handout: announce_math.hpp,
what announce_round.hip is documented to equal) over tests/announce_matrix.py's cases: against
tests/announce_ref.py's restatement and tests/golden/announce_rounds.json, the properties the
reference guarantees whatever its randomness, every refusal with its outputs and bits untouched,
and the reference's own unit cases (peerhandoutpolicy_test.go, completeness_policy_test.go)."""
import ctypes as C

import numpy as np

from kraken_amd import _capi, device as D
from kraken_amd._capi import lib
from tests import announce_matrix as M
from tests import announce_ref as R


def test_header_symbols_and_constants():
    assert {"krk_announce_handout", "krk_announce_round", "krk_announce_round_dev"} <= set(_capi.public_symbols())
    hdr = open(_capi.HEADER_PATH).read()
    for name in ("KRK_AN_MAX_WINDOWS 8u", "KRK_AN_MAX_ORIGINS 8u", "KRK_AN_MAX_LIMIT 64u", "KRK_AN_NONE 0xFFFFFFFFu",
                 "KRK_AN_ORIGIN 0x80000000u", "KRK_AN_COMPLETE_BIT 0x40000000u"):
        assert f"#define {name}" in hdr, name
    assert C.sizeof(_capi.krk_announce_torrent) == 32 and C.sizeof(_capi.krk_announce) == 24


def test_the_restatement_is_what_the_golden_file_records():
    gold = M.golden()
    assert sorted(gold) == sorted(c.label for c in M.cases())
    for c in M.cases():
        assert M.golden_entry(c) == gold[c.label], c.label


def test_round_equals_the_restatement():
    calls, bad = M.run_cases(M.HostBackend(), M.cases())
    assert calls == len(M.cases()) >= 45 and bad == [], bad[:5]


def test_handout_equals_the_restatement():
    """krk_announce_handout announce by announce over the updated rows: the round's handout phase."""
    calls, bad = M.run_cases(M.HandoutBackend(), M.cases())
    assert calls > 0 and bad == [], bad[:5]


def test_matrix_covers_the_shapes():
    seen = {(c.torrents[0][0], c.limit, c.torrents[0][1]) for c in M.cases() if c.label.startswith("matrix")}
    assert seen == {(p, l, w) for p in M.PS for l in M.LIMITS for w in M.WS}
    matrix = [c for c in M.cases() if c.label.startswith("matrix")]
    assert {c.torrents[0][3] for c in matrix} == set(M.OS) and {c.policy for c in matrix} == {0, 1}
    assert all(c.torrents[0][2] != 0 for c in matrix if c.torrents[0][1] > 1)
    assert any(a[3] == M.NONE for c in matrix for a in c.announces)
    # "sampled": the source the announce would have got is gone from what it gets
    c = M.case("all ones P=64")
    assert c.announces[1][3] != M.NONE and c.announces[1][3] not in {h & ~M.CBIT for h in c.ref()[1][1]}


def members(c, t, updated=True):
    """[(member set, complete set) a window] of torrent t, from the restatement's rows."""
    T = R.Torrent(*c.torrents[t])
    T.load(c.ref()[0] if updated else c.bits.tolist())
    return list(zip(T.member, T.complete))


def test_properties_of_every_handout():
    """What the reference guarantees whatever its randomness, on the host form's own outputs."""
    host, n_small = M.HostBackend(), 0
    for c in M.cases():
        _, handout, n_out, labels = host.run(c)
        for k, (t, peer, flags, source, _) in enumerate(c.announces):
            got = handout[k * c.cap:k * c.cap + int(n_out[k])].tolist()
            P, O = c.torrents[t][0], c.torrents[t][3]
            if flags & M.COMPLETE:  # a complete announcer gets nothing
                assert got == [] and labels[3 * k:3 * k + 3].tolist() == [0, 0, 0], c.label
                continue
            ids = [g & ~M.CBIT for g in got]
            assert len(set(ids)) == len(ids), (c.label, "a duplicate")
            store = [i for i in ids if not i & M.ORIGIN]
            assert len(store) <= c.limit and all(i < P for i in store), c.label
            assert sorted(i for i in ids if i & M.ORIGIN) == [M.ORIGIN | o for o in range(O)], (c.label, "the origins")
            assert source not in ids, (c.label, "the source")
            wins = members(c, t)
            union = set().union(*(m for m, _ in wins))
            assert set(store) <= union, c.label
            prio = [0 if c.policy == M.DEFAULT else 1 if g & M.ORIGIN else 0 if g & M.CBIT else 2 for g in got]
            assert prio == sorted(prio), (c.label, "priorities")
            assert labels[3 * k:3 * k + 3].tolist() == [prio.count(p) for p in range(3)], c.label
            for g in got:  # a complete bit only where some window says so
                if g & M.CBIT:
                    assert any(g & ~M.CBIT in m and g & ~M.CBIT in cm for m, cm in wins), c.label
            # SRANDMEMBER with a count >= the set size returns the whole set: while the windows' sizes
            # ADD UP to no more than the limit, every window is taken whole, so the whole union is
            # handed out and a complete bit is the OR over every window.  A union of U <= limit
            # peers alone does not give that: a sample of `need` from a window larger than `need`
            # may repeat peers already selected and leave others of the union out for good
            # (redis.go:172-188; "matrix P=63 limit=64 W=5 cur=2 O=3 policy=0" is such a round).
            if sum(len(m) for m, _ in wins) <= c.limit:
                n_small += 1
                assert set(store) == union - {source}, (c.label, "every peer of a small union")
                for g in got:
                    if not g & M.ORIGIN:
                        i = g & ~M.CBIT
                        assert bool(g & M.CBIT) == any(i in m and i in cm for m, cm in wins), (c.label, "OR over the windows")
    assert n_small > 20


def test_tail_bits_are_never_sampled_and_never_set():
    for p in (63, 65, 4097):
        c = M.case(f"all ones P={p}" if p < 100 else "all ones, more than one stride of words")
        bits, handout, n_out, _ = M.HostBackend().run(c)
        assert np.array_equal(bits, c.bits)  # every bit was set already: nothing changes
        for k in range(len(c.announces)):
            got = [g & ~M.CBIT for g in handout[k * c.cap:k * c.cap + int(n_out[k])].tolist() if not g & M.ORIGIN]
            assert got and all(i < p for i in got), c.label


def test_reference_unit_cases():
    """TestCompletenessPriorityPolicy: seeders, then origins, then incomplete peers;
    TestPriorityPolicyRemoveSource: everybody but the source."""
    c = M.case("completeness_policy_test.go")
    _, handout, n_out, labels = M.HostBackend().run(c)
    got = handout[:int(n_out[0])].tolist()
    assert len(got) == 33 and labels[:3].tolist() == [10, 3, 20]
    assert all(g & M.CBIT and (g & ~M.CBIT) < 10 for g in got[:10])
    assert sorted(got[10:13]) == [M.ORIGIN | o for o in range(3)]
    assert sorted(got[13:]) == list(range(10, 30))
    c = M.case("peerhandoutpolicy_test.go remove source")
    _, handout, n_out, _ = M.HostBackend().run(c)
    assert sorted(handout[:int(n_out[0])].tolist()) == list(range(10))


def test_updates_land_before_any_handout():
    """The last announce of a round is seen by the first one's handout."""
    b = D.AnnounceBatch([(70, 2, 1, 0)], [(0, 3, 0, 3, 1), (0, 69, D.AN_COMPLETE, D.AN_NONE, 2)])
    bits = np.zeros(b.total_words, dtype=np.uint64)
    handout, n_out, labels = D.announce_round(b, bits, 50, D.AN_COMPLETENESS)
    assert handout[0, :int(n_out[0])].tolist() == [69 | D.AN_COMPLETE_BIT] and n_out[1] == 0
    assert labels.tolist() == [[1, 0, 0], [0, 0, 0]]
    assert bits.tolist() == [0, 0, 0, 0, 1 << 3, 1 << 5, 0, 1 << 5]  # ring row 1 is the current window


def test_a_round_of_no_announces():
    assert lib.krk_announce_round(None, 0, None, None, 0, 50, 0, None, None, None) == _capi.KRK_OK
    assert lib.krk_announce_round_dev(None, 0, None, None, 0, 50, 0, None, None, None, None) == _capi.KRK_OK


def test_refusals_leave_outputs_and_bits_untouched():
    c = M.refusal_case()
    bits = c.bits.copy()
    outs = [M.prefilled(k) for k in c.sizes()]
    ptrs = [o.ctypes.data_as(M.u32p) for o in outs]

    def call(change=None):
        a = M.call_args(c, bits.ctypes.data_as(M.u64p), ptrs)
        if change:
            change(a)
        return a

    for label, change in M.invalid_calls():
        assert lib.krk_announce_round(*call(change)) == _capi.KRK_EINVAL, label
        assert b"announce_round" in lib.krk_last_error(), label
        a = call(change)
        # the same through the one-announce form, for each announce the change may concern
        rcs = []
        for k in range(len(c.announces)):
            one = [M.prefilled(n) for n in (c.cap, 1, 3)]
            given = [None if a[7 + j] is None else o.ctypes.data_as(M.u32p) for j, o in enumerate(one)]
            rcs.append(lib.krk_announce_handout(a[0], a[1], a[2], C.byref(a[3][k]) if a[3] is not None else None, a[5],
                                                a[6], *given))
            assert rcs[-1] == _capi.KRK_OK or all((o == M.CANARY32).all() for o in one), label
        assert _capi.KRK_EINVAL in rcs, label
        assert np.array_equal(bits, c.bits) and all((o == M.CANARY32).all() for o in outs), label
    assert lib.krk_announce_round(*call()) == _capi.KRK_OK
    assert M.compare(c, (bits, *outs)) == []
