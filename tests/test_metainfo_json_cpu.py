"""The _torrentmeta JSON codec's host ABI (krk_metainfo_serialize, krk_metainfo_parse,
krk_metainfo_json_envelope, krk_metainfo_json_bound: metainfo_json.cpp) and its use by
core.MetaInfo.Serialize / core.DeserializeMetaInfo, against the plain-Python restatement of
tests/metainfo_json_ref.py.  No device."""
import ctypes as C

import numpy as np
import pytest

from kraken_amd import _capi, core, metainfogen
from kraken_amd._capi import KRK_EFORMAT, KRK_EINVAL, KRK_ERANGE, lib
from tests import metainfo_json_ref as R


def native_serialize(pl, sums, name, length, cap=None, slack=8):
    """(rc, exact size, the buffer with `slack` canary bytes of 0xA5 after cap)."""
    s = np.zeros(0, np.uint32) if sums is None else np.ascontiguousarray(sums, dtype=np.uint32)
    bound = int(lib.krk_metainfo_json_bound(s.size))
    cap = bound if cap is None else cap
    out = np.full(cap + slack, 0xA5, dtype=np.uint8)
    n = C.c_uint64(0)
    nb = name.encode()
    rc = lib.krk_metainfo_serialize(pl, s.ctypes.data if s.size else None, s.size, sums is None, nb, len(nb), length,
                                    out.ctypes.data, cap, C.byref(n))
    return rc, n.value, out


def native_parse(doc: bytes, sums_cap=None):
    """(rc, (piece length, sums list or None, name, length))."""
    cap = (len(doc) + 1) // 2 if sums_cap is None else sums_cap
    sums = np.full(max(cap, 1), 0xDEADBEEF, dtype=np.uint32)
    pl, ln, n, null = C.c_int64(), C.c_int64(), C.c_uint64(), C.c_int()
    name = C.create_string_buffer(64)
    rc = lib.krk_metainfo_parse(doc, len(doc), C.byref(pl), sums.ctypes.data, cap, C.byref(n), C.byref(null), name,
                                C.byref(ln))
    if rc:
        return rc, None
    return rc, (pl.value, None if null.value else [int(x) for x in sums[:n.value]], name.raw.decode(), ln.value)


@pytest.fixture(scope="module")
def documents():
    """[(arguments, the restatement's bytes)] over the whole matrix, computed once."""
    return [(m, R.serialize(*m)) for m in R.matrix()]


def test_status_code_and_geometry():
    assert KRK_EFORMAT == -8
    unit, span = R.geometry()
    assert unit >= 64 and unit % 64 == 0 and span >= 64 and span % 64 == 0


def test_serialize_bytes_equal_the_restatement_over_the_matrix(documents):
    assert len(documents) > 80
    for (pl, sums, name, length), want in documents:
        rc, n, out = native_serialize(pl, sums, name, length)
        assert rc == 0 and n == len(want) and out[:n].tobytes() == want
        assert (out[n:] == 0xA5).all()  # nothing past the document
        n_sums = 0 if sums is None else len(sums)
        assert int(lib.krk_metainfo_json_bound(n_sums)) >= len(want)


def test_bound_is_never_below_the_largest_document():
    for n in (0, 1, 2, 63, 257):
        worst = R.serialize(R.I64_MIN, [0xFFFFFFFF] * n, R.NAME_LOWER, R.I64_MIN)
        assert int(lib.krk_metainfo_json_bound(n)) >= len(worst)
    assert int(lib.krk_metainfo_json_bound(0)) >= len(R.serialize(R.I64_MIN, None, R.NAME_LOWER, R.I64_MIN))


def test_serialize_cap_exact_and_one_short(documents):
    for (pl, sums, name, length), want in documents[::5]:
        rc, n, out = native_serialize(pl, sums, name, length, cap=len(want))
        assert rc == 0 and out[:n].tobytes() == want and (out[n:] == 0xA5).all()
        rc, n, out = native_serialize(pl, sums, name, length, cap=len(want) - 1)
        assert rc == KRK_ERANGE and n == len(want)
        assert (out[len(want) - 1:] == 0xA5).all()  # the canary after cap


@pytest.mark.parametrize("name", ["", "ab" * 31 + "a", "ab" * 32 + "a", "g" + "0" * 63, "0" * 63 + '"', "é" * 32])
def test_serialize_refuses_a_name_that_is_not_64_hex_digits(name):
    rc, _, out = native_serialize(4, [1], name, 3)
    assert rc == KRK_EINVAL and (out == 0xA5).all()
    # the mirror falls back to json.dumps, as before
    mi = core.MetaInfo(4, np.array([1], np.uint32), name, 3, None, None)
    assert mi.Serialize() == R.serialize(4, [1], name, 3)


def test_serialize_refuses_null_with_sums():
    s = np.array([1], np.uint32)
    n = C.c_uint64()
    out = np.zeros(256, np.uint8)
    assert lib.krk_metainfo_serialize(4, s.ctypes.data, 1, 1, R.NAME_LOWER.encode(), 64, 3, out.ctypes.data, 256,
                                      C.byref(n)) == KRK_EINVAL


def test_mirror_serialize_is_the_restatement(documents):
    for (pl, sums, name, length), want in documents:
        assert core.MetaInfo(pl, sums, name, length, None, None).Serialize() == want
    # beyond int64 the native call cannot take the value: json.dumps, as before
    big = core.MetaInfo(1 << 63, None, R.NAME_LOWER, -(1 << 63) - 1, None, None)
    assert big.Serialize() == R.serialize(1 << 63, None, R.NAME_LOWER, -(1 << 63) - 1)


def test_every_serialised_document_round_trips(documents):
    for (pl, sums, name, length), doc in documents:
        rc, got = native_parse(doc)
        want_sums = None if sums is None else [int(x) for x in sums]
        assert rc == 0 and got == (pl, want_sums, name, length)
        assert got == R.general_fields(doc)
        mi = core.DeserializeMetaInfo(doc)
        assert R.observed(mi) == R.parent_deserialize(doc)
        assert (mi._sums is None) == (sums is None)  # null and [] stay distinct
        assert mi.Serialize() == doc


def test_parse_sums_cap():
    doc = R.serialize(4, [1, 2, 3], R.NAME_LOWER, 10)
    assert native_parse(doc, sums_cap=3)[0] == 0
    assert native_parse(doc, sums_cap=2)[0] == KRK_ERANGE
    # (len + 1) / 2 suffices for the densest array a document can hold
    dense = R.serialize(0, [0] * 500, R.NAME_LOWER, 0)
    assert native_parse(dense)[0] == 0


def test_mutation_property_accept_means_the_general_decoders_result():
    """Every single-byte substitution, insertion and deletion, at every position of the nine
    documents: a mutant the native parser accepts decodes to the general decoder's four fields."""
    total = accepted = 0
    for doc in R.mutation_documents():
        assert native_parse(doc) == (0, R.general_fields(doc))
        for m in R.mutants(doc):
            total += 1
            rc, got = native_parse(m)
            assert rc in (0, KRK_EFORMAT), (rc, m)
            if rc == 0:
                accepted += 1
                assert got == R.general_fields(m), m
    # a position brings 36 insertions, at least 35 substitutions and a deletion
    assert total >= 72 * sum(len(d) for d in R.mutation_documents()) and accepted > 1_000, (total, accepted)


@pytest.mark.parametrize("case", sorted(R.must_refuse()))
def test_must_refuse_then_the_mirror_gives_the_parents_result(case):
    doc = R.must_refuse()[case]
    rc, _ = native_parse(doc)
    assert rc == KRK_EFORMAT
    assert b"not the canonical form at byte" in lib.krk_last_error()
    want = R.parent_deserialize(doc)
    try:
        got = R.observed(core.DeserializeMetaInfo(doc))
    except ValueError as e:
        got = str(e)
    assert got == want


def test_envelope_span_is_the_bracket_positions(documents):
    pl, ln, a0, a1, null = C.c_int64(), C.c_int64(), C.c_uint64(), C.c_uint64(), C.c_int()
    name = C.create_string_buffer(64)
    for (p, sums, nm, length), doc in documents:
        assert lib.krk_metainfo_json_envelope(doc, len(doc), C.byref(pl), C.byref(a0), C.byref(a1), C.byref(null),
                                              name, C.byref(ln)) == 0
        assert (a0.value, a1.value) == R.bracket_span(doc)
        assert (pl.value, name.raw.decode(), ln.value, bool(null.value)) == (p, nm, length, sums is None)
    # the span is not looked at: garbage between the brackets is still an envelope
    doc = R.serialize(4, [1, 2, 3], R.NAME_LOWER, 10).replace(b"[1,2,3]", b"[ x,,]]")
    assert lib.krk_metainfo_json_envelope(doc, len(doc), C.byref(pl), C.byref(a0), C.byref(a1), C.byref(null), name,
                                          C.byref(ln)) == 0
    assert doc[a0.value:a1.value] == b" x,,]"
    for case, bad in R.must_refuse().items():
        span_only = case in ("leading zero", "2^32", "11 digits", "[,]", "[1,]", "[,1]", "1.0", "1e3", "negative sum")
        rc = lib.krk_metainfo_json_envelope(bad, len(bad), C.byref(pl), C.byref(a0), C.byref(a1), C.byref(null), name,
                                            C.byref(ln))
        assert rc == (0 if span_only else KRK_EFORMAT), case


def test_device_entry_points_refuse_bad_descriptors_before_a_device_is_needed():
    assert lib.krk_metainfo_serialize_batch_dev(None, 0, None, None, None, None) == 0
    assert lib.krk_metainfo_parse_sums_batch_dev(None, 0, None, None, None, None) == 0
    blob = _capi.krk_metainfo_json_blob(0, 0, 4, 3, 0, 0, 0, b"g" * 64)
    buf = np.zeros(1024, np.uint8)
    assert lib.krk_metainfo_serialize_batch_dev(C.byref(blob), 1, None, buf.ctypes.data, buf.ctypes.data,
                                                None) == KRK_EINVAL
    assert b"64 hex digits" in lib.krk_last_error()


def test_dircas_stores_serialised_bytes_with_the_same_changed_answer(tmp_path):
    cas = metainfogen.DirCAS(str(tmp_path))
    d = cas.WriteCacheFile(b"abc")
    mi = core.NewMetaInfo(d, b"abc", 4)
    assert cas.SetCacheFileMetadataBytes(d.Hex(), mi.Serialize()) is True
    assert cas.SetCacheFileMetadata(d.Hex(), mi) is False
    assert cas.SetCacheFileMetadataBytes(d.Hex(), mi.Serialize()) is False
    assert cas.SetCacheFileMetadataBytes(d.Hex(), b"x") is True
    assert cas.GetCacheFileMetadata(d.Hex()) == b"x"
