"""The _torrentmeta JSON matrix (tests/metainfo_json_matrix.py) where no GPU is: the matrix's own
conditions -- the six unit totals hit exactly, the last-step shapes and break positions complete,
every mutant refused and every twin accepted by the plain-Python reference, the stride cases larger
than a launch -- the host forms (krk_metainfo_serialize, krk_metainfo_parse) through the same cases
and comparison the device runs, and the krk_metainfo_json_scan_geometry hook."""
import ctypes as C

import numpy as np
import pytest

from kraken_amd import _capi
from kraken_amd._capi import lib
from tests import metainfo_json_matrix as M
from tests import metainfo_json_ref as R


@pytest.fixture(scope="module")
def host():
    return M.HostBackend()


# ------------------------------------------------------------------ the hook
def test_scan_geometry_hook():
    assert M.PASS > 0 and M.G > 0 and M.PASS % 64 == 0
    v = C.c_uint64(77)
    assert lib.krk_metainfo_json_scan_geometry(None, C.byref(v)) == _capi.KRK_EINVAL
    assert lib.krk_metainfo_json_scan_geometry(C.byref(v), None) == _capi.KRK_EINVAL
    assert v.value == 77 and b"metainfo_json_scan_geometry" in lib.krk_last_error()
    assert "krk_metainfo_json_scan_geometry" in _capi.internal_symbols()
    assert "krk_metainfo_json_scan_geometry" not in _capi.public_symbols()
    assert R.geometry() == (M.Us, M.Up)  # the older hook is as it was


# ------------------------------------------------------------------ the matrix's own conditions
def test_the_six_unit_totals_are_hit_exactly():
    P = M.PASS
    assert M.TOTALS == (P - 1, P, P + 1, 2 * P, 2 * P + 1, 3 * P + 517)
    assert [c.n_units for c in M.s1_cases()] == list(M.TOTALS)
    assert [c.n_units for c in M.p1_cases()] == list(M.TOTALS)
    blobs, _ = M.s1_blobs()
    assert 5000 < len(blobs) < 7000
    big = M.s1_case(M.TOTALS[-1])
    # prefixes of one list: the documents are shared, all but the trimmed last
    assert all(a is b for a, b in zip(M.s1_case(M.TOTALS[0]).blobs[:-1], big.blobs))
    # every sum count of the cycle, null and [] among them, and unit byte counts that differ
    assert {b.k if b.sums is not None else None for b in big.blobs[:10]} == set(M.S1_COUNTS)
    assert len({len(b.doc) for b in big.blobs if b.k == M.Us}) > 50
    spans, _ = M.p1_spans()
    assert {len(s) for s in spans[:8]} == set(M.P1_LENGTHS)
    # span i starts at text_off % 16 == i % 16, as the device tests lay their spans
    d = M.p1_case(M.TOTALS[2]).desc
    assert ((d["text_off"] % 16) == (np.arange(len(d)) % 16)).all()
    assert not M.p1_case(M.TOTALS[2]).want_status.any()


def test_every_last_step_shape_is_present():
    call = M.s2_case()
    got = M.s2_coverage(call)
    assert got == M.S2_SHAPES and len(M.S2_SHAPES) == 48 * 3 and call.n == 48 * 3
    # the three narrow store branches: inside one dword, ending a dword exactly, a head alone
    for pos in M.S2_POSITIONS:
        assert {(pos, 1, 1), (pos, 1, 2), (pos, 2, 1), (pos, 1, 3), (pos, 2, 2), (pos, 3, 1), (pos, 3, 4)} <= got
    # both ways to a phase are used
    assert len({len(str(b.pl)) for b in call.blobs}) == 4 and len(set((call.desc["out_off"] % 4).tolist())) == 4


def test_every_break_position_is_present_and_refused():
    base = M.p2_base()
    assert len(base) >= 130 * M.Up and M.parse_units(len(base)) - 1 == M.P2_LAST and M.span_reference(base) is not None
    muts = M.p2_mutants()
    assert {(u, at) for u, at, _, _ in muts} == {(u, at) for u in M.P2_UNITS for at in M.P2_AT}
    assert set(M.P2_UNITS) == {0, 63, 64, 65, 127, 128, M.P2_LAST} and set(M.P2_AT) == {0, 63, 64, M.Up - 1}
    assert 28 < len(muts) <= 64
    for at in M.P2_AT:  # every kind at every in-unit position, in some unit
        assert {k for _, a, k, _ in muts if a == at} == set(M.P2_KINDS), at
    for u, at, kind, m in muts:
        p = u * M.Up + at
        assert len(m) == len(base) and m[:p] == base[:p] and m[p + 1:] == base[p + 1:] and m[p] != base[p]
        assert M.span_reference(m) is None, (u, at, kind)
        if kind == "double comma":
            assert m[p - 1:p + 1] == b",,"
        if kind == "leading zero":
            assert (p == 0 or m[p - 1:p] == b",") and m[p:p + 1] == b"0" and m[p + 1:p + 2].isdigit()
    # a break on the 64-byte step edge, in a unit's last byte, in the span's last byte
    assert any(at == 64 and k != "non-digit" for _, at, k, _ in muts)
    assert any(u == M.P2_LAST and at == M.Up - 1 for u, at, _, _ in muts)
    call = M.p2_case()
    refused = call.status_mask == 1
    assert refused.sum() == len(muts) and not call.want_status[~refused].any()
    assert call.text.nbytes <= 64 * 131 * M.Up + 65 * 2 * M.Up


def test_every_edge_mutant_is_refused_and_every_twin_accepted():
    bad, good = M.p3_spans()
    assert len(bad) == 2 * (1 + 10 + 9 + 5) and len(good) == 2 * (11 + 2)
    for name, s in bad.items():
        assert M.span_reference(s) is None, name
    for name, s in good.items():
        assert M.span_reference(s) is not None, name
    for j in M.P3_EDGE_UNITS:
        E = j * M.Up
        s = bad[f"j={j} leading zero ends the unit"]
        assert s[E - 2:E + 1] == b",05"
        for k in range(1, 11):
            s = bad[f"j={j} 11 digits, {k} before the edge"]
            assert s[E - k - 1:E - k + 12] == b",12345678901,"
        for k in range(1, 10):
            assert bad[f"j={j} 2^32, {k} digits before the edge"][E - k - 1:E - k + 11] == b",4294967296,"
        assert bad[f"j={j} comma ends the unit, comma begins the next"][E - 2:E + 1] == b"7,,"
        s = bad[f"j={j} trailing comma ends the span on the edge"]
        assert len(s) == E and s.endswith(b"7,")
        s = bad[f"j={j} the span's last byte a comma, a unit's first"]
        assert len(s) == E + 1 and s.endswith(b",7,")
        assert bad[f"j={j} non-digit begins the unit"][E:E + 1] == b"x"
        assert bad[f"j={j} non-digit ends the unit"][E - 1:E] == b"x"
        for k in range(0, 11):
            s = good[f"j={j} 2^32-1, {k} digits before the edge"]
            assert s[E - k:E - k + 10] == b"4294967295" and (k == 0 or s[E - k - 1:E - k] == b",")
        assert good[f"j={j} zero ends the unit, comma next"][E - 2:E + 1] == b",0,"
        s = good[f"j={j} zero ends the span on the edge"]
        assert len(s) == E and s.endswith(b",0")
    call = M.p3_case()
    assert (call.status_mask == 1).sum() == len(bad) and not call.want_status[call.status_mask != 1].any()


def test_the_span_reference_itself():
    for s in (b"0", b"4294967295", b"1,2,3", b"10,0,9", b""):
        assert M.span_reference(s) == [int(x) for x in s.split(b",") if x]
    for s in (b"00", b"01", b"4294967296", b"12345678901", b"1,,2", b",1", b"1,", b" 1", b"1 ", b"-1", b"1.0", b"1e3",
              b"1,2\n", b"x", b","):
        assert M.span_reference(s) is None, s


def test_the_stride_cases_exceed_a_launch():
    assert M.S4_BLOBS > M.G and M.P5_SPANS > M.G
    s4 = M.s4_case()
    assert s4.n == M.S4_BLOBS and s4.n_units == s4.n > M.G
    img, lens = s4.expect()
    for i in (0, 7, M.G - 1, M.G, M.G + 2):  # the template rows against json.dumps
        doc = R.serialize(4096, [i % 10], R.NAME_MIXED, 4096)
        o = int(s4.desc["out_off"][i])
        assert img[o:o + len(doc)].tobytes() == doc and lens[i] == len(doc)
        assert (img[o - M.GAP:o] == M.FILL).all() and (img[o + len(doc):o + M.bound(1) + M.GAP] == M.FILL).all()
    assert len(set((s4.desc["out_off"] % 4).tolist())) == 4
    p5 = M.p5_stride_case()
    assert p5.n == M.P5_SPANS and p5.n_units == p5.n > M.G
    for i in (0, 7, M.G - 1, M.G, M.G + 2):
        d = p5.desc[i]
        span = p5.text[int(d["text_off"]):int(d["text_off"]) + int(d["text_len"])].tobytes()
        assert span == str(i % 10).encode() and int(d["text_off"]) % 16 == i % 16
        assert p5.want[int(d["sums_off"])] == M.span_reference(span)[0]
        assert p5.want[int(d["sums_off"]) - 1] == M.CANARY and p5.want[int(d["sums_off"]) + 1] == M.CANARY


def test_the_owner_search_cases():
    s3 = M.s3_cases()
    assert len(s3) == len(M.S3_RUNS) + len(M.S3_ONLY_UNITLESS) + len(M.S3_WITH_UNITS)
    for r, call in zip(M.S3_RUNS, s3):
        k = call.desc["n_sums"]
        assert not k[:r].any() and not k[-r:].any() and k[r] and k[-r - 1]      # head and tail
        assert not k[r + 4:2 * r + 4].any() and k[r + 3] and k[2 * r + 4]        # middle
        assert set(call.desc["sums_null"][:max(r, 2)].tolist()) <= {0, 1}
    assert {int(c.desc["sums_null"][:2].sum()) for c in s3[2:5]} == {1}          # null and [] mixed
    assert [c.n_units for c in s3[5:7]] == [0, 0] and [c.n for c in s3[5:7]] == list(M.S3_ONLY_UNITLESS)
    assert [c.n for c in s3[7:]] == list(M.S3_WITH_UNITS) and all(c.desc["n_sums"].all() for c in s3[7:])
    p5 = M.p5_cases()
    for r, call in zip(M.S3_RUNS, p5):
        n = call.desc["text_len"]
        assert not n[:r].any() and not n[-r:].any() and not n[r + 4:2 * r + 4].any() and n[r:r + 4].all()
        assert set(call.want_status[:r].tolist()) == ({0, 2} if r > 1 else {0})
    assert [c.n_units for c in p5[5:]] == [0, 0]
    p4 = M.p4_case()
    assert set(p4.desc["text_len"].tolist()) <= set(range(2 * M.Up + 1, 3 * M.Up + 1))
    assert int((p4.desc["expect_n"].astype(np.int64)).max()) > 2 * M.Up  # thousands of words that must stay canaries


# ------------------------------------------------------------------ the host forms over the matrix
def test_host_serialize_scan_pass_prefix(host):
    calls, bad = M.run_cases(host, [M.s1_case(M.PASS + 1)])
    assert calls == 1 and bad == [], bad[:5]


def test_host_serialize_last_step_shapes_and_owner_search(host):
    calls, bad = M.run_cases(host, [M.s2_case()] + M.s3_cases())
    assert calls == 1 + len(M.s3_cases()) and bad == [], bad[:5]


def test_host_parse_scan_pass_prefix(host):
    calls, bad = M.run_cases(host, [M.p1_case(M.PASS + 1)])
    assert calls == 1 and bad == [], bad[:5]


def test_host_parse_breaks_edges_and_count_guard(host):
    calls, bad = M.run_cases(host, [M.p2_case(), M.p3_case(), M.p4_case()])
    assert calls == 3 and bad == [], bad[:5]


def test_the_comparison_notices_a_wrong_byte_word_and_status(host):
    """The comparison is what every backend's result goes through: one flipped byte, one canary
    overwritten, one wrong status bit must each be reported."""
    ser = M.s3_cases()[0]
    out, lens = host.serialize(ser)
    assert M.compare_ser(ser, (out, lens)) == []
    out2 = out.copy()
    out2[-1] ^= 1  # the last canary byte
    lens2 = lens.copy()
    lens2[3] += 1
    assert len(M.compare_ser(ser, (out2, lens))) == 1 and len(M.compare_ser(ser, (out, lens2))) == 1
    par = M.p4_case()
    sums, status = host.parse(par)
    assert M.compare_parse(par, (sums, status)) == []
    sums2 = sums.copy()
    sums2[0] = 0  # a canary in front of the first range
    status2 = status.copy()
    status2[0] |= 1
    assert len(M.compare_parse(par, (sums2, status))) == 1 and len(M.compare_parse(par, (sums, status2))) == 1
    # an unspecified word (inside expect_n, past the count) is not compared
    i = int(np.flatnonzero(~par.care)[0])
    sums3 = sums.copy()
    sums3[i] ^= 0xFFFF
    assert M.compare_parse(par, (sums3, status)) == []
