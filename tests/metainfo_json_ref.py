"""The reference of the _torrentmeta JSON codec tests, in plain Python: json.dumps with Go's
separators in core.info's declared field order, and the four fields the general decoder
(encoding/json's rules, kraken_amd.core._decode_general) reads from any document.  Shared by
tests/test_metainfo_json_cpu.py and tests/test_gpu_metainfo_json.py, which also take their
sum-count / value / header matrix from here."""
import ctypes as C
import json

import numpy as np

from kraken_amd import core
from kraken_amd._capi import lib

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
NAME_LOWER = "0123456789abcdef" * 4
NAME_UPPER = "0123456789ABCDEF" * 4
NAME_MIXED = "aBcDeF0123456789" * 4


def serialize(piece_length, sums, name, length) -> bytes:
    """MetaInfo.Serialize restated: sums is None (nil slice -> null) or a sequence."""
    obj = {"Info": {"PieceLength": int(piece_length), "PieceSums": None if sums is None else [int(x) for x in sums],
                    "Name": name, "Length": int(length)}}
    return json.dumps(obj, separators=(",", ":")).encode()


def general_fields(data):
    """(piece length, sums list or None, name, length) by the general decoder, or the ValueError's
    text."""
    try:
        pl, arr, name, length = core._decode_general(data)
    except ValueError as e:
        return str(e)
    return pl, None if arr is None else [int(x) for x in arr], name, length


def parent_deserialize(data):
    """What DeserializeMetaInfo gave before the native parser: the general decoder, then the
    InfoHash and the digest.  The six observable values, or the ValueError's text."""
    try:
        pl, arr, name, length = core._decode_general(data)
        ih = core._info_hash(pl, arr if arr is not None else np.zeros(0, np.uint32), name, length)
        try:
            d = core.NewSHA256DigestFromHex(name)
        except ValueError as e:
            raise ValueError(f"parse name: {e}") from None
    except ValueError as e:
        return str(e)
    return pl, None if arr is None else [int(x) for x in arr], name, length, bytes(ih), d


def observed(mi):
    s = None if mi._sums is None else [int(x) for x in mi._sums]
    return mi.PieceLength(), s, mi._name, mi.Length(), bytes(mi.InfoHash()), mi.Digest()


def bracket_span(doc: bytes):
    """(begin, end) of the bytes strictly between '[' and ']' of a canonical document, or the
    position after `null` twice."""
    k = doc.index(b'"PieceSums":') + len(b'"PieceSums":')
    if doc[k:k + 4] == b"null":
        return k + 4, k + 4
    assert doc[k:k + 1] == b"["
    return k + 1, doc.index(b"]", k)


def geometry():
    s, p = C.c_uint64(), C.c_uint64()
    assert lib.krk_metainfo_json_geometry(C.byref(s), C.byref(p)) == 0
    return s.value, p.value


def i64_edges():
    """0, +-1, every digit count up to 19, the int64 extremes."""
    out = [0, 1, -1, I64_MAX, I64_MIN]
    for k in range(1, 19):
        out += [10 ** k - 1, 10 ** k, -(10 ** k)]
    return out


def sum_counts():
    """None stands for the nil slice."""
    unit, _ = geometry()
    return [None, 0, 1, 63, 64, 65, unit - 1, unit, unit + 1, 2 * unit + 1]


def sum_values(kind: str, n: int, seed: int = 1) -> np.ndarray:
    if kind == "one_digit":
        return (np.arange(n, dtype=np.uint32) % 10).astype(np.uint32)
    if kind == "max":
        return np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    if kind == "ladder":
        steps = [v for k in range(1, 10) for v in (10 ** k - 1, 10 ** k)]
        return np.array([steps[i % len(steps)] for i in range(n)], dtype=np.uint32)
    rng = np.random.default_rng(seed + n)
    # every digit count is likely: a random width, then a random value of that width
    width = rng.integers(1, 33, size=n)
    return (rng.integers(0, 1 << 32, size=n, dtype=np.uint64) >> (32 - width).astype(np.uint64)).astype(np.uint32)


VALUE_KINDS = ("one_digit", "max", "ladder", "random")


def matrix():
    """[(piece_length, sums or None, name, length)]: every sum count crossed with every value
    kind, the headers walking through the int64 edges and the three name cases."""
    edges, names = i64_edges(), (NAME_LOWER, NAME_UPPER, NAME_MIXED)
    out, k = [], 0
    for n in sum_counts():
        for kind in VALUE_KINDS if n else VALUE_KINDS[:1]:
            sums = None if n is None else sum_values(kind, n)
            out.append((edges[k % len(edges)], sums, names[k % 3], edges[(k * 7 + 3) % len(edges)]))
            k += 1
    for k, e in enumerate(edges):  # every header edge at least once in both fields
        out.append((e, sum_values("random", 5, k), names[k % 3], edges[-1 - k]))
    return out


# The nine documents of the mutation property: null / [] / five sums at the digit edges, crossed
# with small, negative and int64-extreme headers.
def mutation_documents():
    five = [0, 9, 10, 4294967295, 1000000000]
    return [serialize(pl, s, NAME_MIXED, ln)
            for s in (None, [], five)
            for pl, ln in ((4, 17), (-3, -25), (I64_MAX, I64_MIN))]


MUTATION_ALPHABET = b'0123456789-,:"{}[] nulaeIPN.\\+EfxL\x00\xff'
assert len(MUTATION_ALPHABET) == 36


def mutants(doc: bytes):
    """Every single-byte substitution, insertion and deletion over the alphabet."""
    for i in range(len(doc) + 1):
        for c in MUTATION_ALPHABET:
            yield doc[:i] + bytes([c]) + doc[i:]
            if i < len(doc) and doc[i] != c:
                yield doc[:i] + bytes([c]) + doc[i + 1:]
        if i < len(doc):
            yield doc[:i] + doc[i + 1:]


def must_refuse():
    """Documents outside the canonical form, by name."""
    ok = serialize(4, [1, 2, 3], NAME_LOWER, 10)
    body = lambda arr: ok.replace(b"[1,2,3]", arr)
    name = lambda s: ok.replace(NAME_LOWER.encode(), s)
    return {
        "whitespace": ok.replace(b",", b", ", 1),
        "leading space": b" " + ok,
        "trailing newline": ok + b"\n",
        "leading zero": body(b"[1,02,3]"),
        "leading zero header": ok.replace(b'"PieceLength":4', b'"PieceLength":04'),
        "2^32": body(b"[1,4294967296,3]"),
        "11 digits": body(b"[1,10000000000,3]"),
        "-0": ok.replace(b'"Length":10', b'"Length":-0'),
        "int64 overflow": ok.replace(b'"Length":10', b'"Length":9223372036854775808'),
        "int64 underflow": ok.replace(b'"PieceLength":4', b'"PieceLength":-9223372036854775809'),
        "[,]": body(b"[,]"),
        "[1,]": body(b"[1,]"),
        "[,1]": body(b"[,1]"),
        "1.0": body(b"[1.0]"),
        "1e3": body(b"[1e3]"),
        "negative sum": body(b"[-1]"),
        "lower-case key": ok.replace(b'"Name"', b'"name"'),
        "reordered keys": b'{"Info":{"PieceSums":[1,2,3],"PieceLength":4,"Name":"' + NAME_LOWER.encode() +
                          b'","Length":10}}',
        "duplicated key": ok.replace(b'"Length":10', b'"Length":10,"Length":10'),
        "missing field": ok.replace(b'"PieceLength":4,', b""),
        "name 63": name(NAME_LOWER[:63].encode()),
        "name 65": name(NAME_LOWER.encode() + b"0"),
        "name non-hex": name(b"g" + NAME_LOWER[1:].encode()),
        "trailing bytes": ok + b"}",
        "empty": b"",
        "truncated": ok[:40],
        "null document": b"null",
    }
