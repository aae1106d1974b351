"""The device _torrentmeta JSON codec (metainfo_json.hip behind krk_metainfo_serialize_batch_dev and
krk_metainfo_parse_sums_batch_dev) at its scan-pass, grid-stride, store-step and unit edges: the
cases, their expectations and the comparison, shared by tests/test_gpu_metainfo_json_matrix.py (the
device entry points) and tests/test_metainfo_json_matrix_cpu.py (krk_metainfo_serialize and
krk_metainfo_parse, the host forms the kernels are documented to equal).  A helper module, not a
test file.

Expectations are plain Python, never the library: tests/metainfo_json_ref.serialize (json.dumps)
for a document, and for a span the grammar as a regular expression, a <= 0xFFFFFFFF check and
int() (span_reference).  The geometry is read from the built library: Us sums a serialise unit, Up
span bytes a parse unit, PASS unit counts a pass of the one-workgroup scan, G workgroups a launch
at the most.

A call is ONE batch call (SerCall / ParseCall) that carries its descriptors, its inputs and the
WHOLE expected output: every document byte, every out_len, every status word, every sums word and
the canaries between and behind the ranges.  Groups:
 S1 prefixes of one seeded blob list with exactly PASS-1 .. 3 PASS + 517 serialise units;
 S2 blobs whose final 64-sum step stores 1..12 bytes at every phase of a dword, at three positions;
 S3 runs of unit-less blobs (null, []) at the head, in the middle and at the tail, and none but;
 S4 G + 3 one-sum blobs: unit u and unit u + G share a workgroup;
 P1 the same six unit totals in parse units, valid spans of mixed lengths;
 P2 single-byte breaks of one long span in unit 0, 63, 64, 65, 127, 128 and the last;
 P3 malformed numbers across a unit edge, and their valid twins;
 P4 expect_n far from the number count: nothing outside the expect_n words is written;
 P5 runs of empty spans, G + 3 one-byte spans, outputs in page-locked host memory."""
import ctypes as C
import functools
import re

import numpy as np

from kraken_amd import _capi
from kraken_amd._capi import KRK_EFORMAT, KRK_OK, check, lib
from tests import metainfo_json_ref as R

SEED = 20261021
FILL = 0xA5            # every output byte before a call
CANARY = 0x5AFEC0DE    # every sums_out word before a call
GAP = 24               # canary bytes between two documents' slots
PAD = 5                # canary words between two spans' sums
LANES = 64             # sums a format step takes: one wave
FILLER = 0x0BADBAD0    # unused sums between two blobs' ranges

BLOB_DT = np.dtype([("sums_off", "<u8"), ("n_sums", "<u8"), ("piece_length", "<i8"), ("length", "<i8"),
                    ("out_off", "<u8"), ("sums_null", "<u4"), ("reserved", "<u4"), ("name", "S64")])
SPAN_DT = np.dtype([("text_off", "<u8"), ("text_len", "<u8"), ("sums_off", "<u8"), ("expect_n", "<u8")])
assert BLOB_DT.itemsize == C.sizeof(_capi.krk_metainfo_json_blob)
assert SPAN_DT.itemsize == C.sizeof(_capi.krk_metainfo_json_span)
BLOBP, SPANP = C.POINTER(_capi.krk_metainfo_json_blob), C.POINTER(_capi.krk_metainfo_json_span)


def scan_geometry():
    p, g = C.c_uint64(), C.c_uint64()
    check(lib.krk_metainfo_json_scan_geometry(C.byref(p), C.byref(g)))
    return int(p.value), int(g.value)


Us, Up = R.geometry()
PASS, G = scan_geometry()
TOTALS = (PASS - 1, PASS, PASS + 1, 2 * PASS, 2 * PASS + 1, 3 * PASS + 517)
NAMES = (R.NAME_LOWER, R.NAME_UPPER, R.NAME_MIXED)


@functools.lru_cache(maxsize=None)
def bound(n_sums):
    """The slot a caller gives a document of n_sums sums."""
    return int(lib.krk_metainfo_json_bound(n_sums))


def ser_units(n_sums):
    return (n_sums + Us - 1) // Us


def parse_units(n_bytes):
    return (n_bytes + Up - 1) // Up


# ------------------------------------------------------------------ the span reference
U32 = rb"(0|[1-9][0-9]{0,9})"
SPAN_RX = re.compile(U32 + rb"(," + U32 + rb")*")
_span_cache = {}


def span_reference(span: bytes):
    """The values of a canonical span (U32(,U32)*, or empty), or None: the reference refuses it."""
    if span not in _span_cache:
        vals = None
        if not span:
            vals = []
        elif SPAN_RX.fullmatch(span):
            vals = [int(x) for x in span.split(b",")]
            if max(vals) > 0xFFFFFFFF:
                vals = None
        _span_cache[span] = vals
    return _span_cache[span]


# ------------------------------------------------------------------ calls
class Blob:
    """One document's fields and its reference bytes, built once."""

    def __init__(self, pl, sums, name, length):
        self.pl, self.name, self.length = int(pl), name, int(length)
        self.sums = None if sums is None else np.ascontiguousarray(sums, dtype=np.uint32)
        self.doc = R.serialize(pl, None if sums is None else self.sums.tolist(), name, length)

    @property
    def k(self):
        return 0 if self.sums is None else int(self.sums.size)


class SerCall:
    def __init__(self, label, desc, sums, out_size, expect, blobs=None):
        self.label, self.desc, self.sums, self.out_size, self.blobs = label, desc, sums, int(out_size), blobs
        self.expect = expect  # () -> (the whole out buffer, out_len)
        self.n = len(desc)
        self.n_units = int(ser_units(desc["n_sums"].astype(np.int64)).sum())


def ser_call(label, blobs, residues=(0, 1, 2, 3)):
    """Blob i's slot lies GAP bytes behind the one before at out_off % 4 == residues[i % len]; up
    to two unused sums lie between two blobs' ranges."""
    n = len(blobs)
    desc = np.zeros(n, BLOB_DT)
    off = s_off = 0
    parts = []
    for i, b in enumerate(blobs):
        k = b.k
        off += GAP
        off += (residues[i % len(residues)] - off) % 4
        desc[i] = (s_off, k, b.pl, b.length, off, b.sums is None, 0, b.name.encode())
        if k:
            parts.append(b.sums)
        if i % 3:
            parts.append(np.full(i % 3, FILLER, np.uint32))
        s_off += k + i % 3
        off += bound(k)
    sums = np.concatenate(parts + [np.zeros(1, np.uint32)])
    out_size = off + GAP

    def expect():
        img = np.full(out_size, FILL, np.uint8)
        lens = np.zeros(n, np.uint64)
        for i, b in enumerate(blobs):
            o = int(desc["out_off"][i])
            img[o:o + len(b.doc)] = np.frombuffer(b.doc, np.uint8)
            lens[i] = len(b.doc)
        return img, lens

    return SerCall(label, desc, sums, out_size, expect, blobs)


class ParseCall:
    """want / care: the whole sums buffer and the words the contract specifies; status i must be
    want_status[i] under status_mask[i] (all bits for a canonical span, bit 0 for a refused one)."""

    def __init__(self, label, desc, text, want, care, want_status, status_mask, spans=None):
        self.label, self.desc, self.text, self.want, self.care = label, desc, text, want, care
        self.want_status, self.status_mask, self.spans = want_status, status_mask, spans
        self.n = len(desc)
        self.n_units = int(parse_units(desc["text_len"].astype(np.int64)).sum())


def parse_call(label, items):
    """items: [(span bytes, expect_n)].  Span i starts at text_off % 16 == i % 16 with '#' between
    the spans; the spans' sums ranges lie PAD canary words apart."""
    n = len(items)
    desc = np.zeros(n, SPAN_DT)
    text = bytearray()
    s_off = PAD
    for i, (span, expect_n) in enumerate(items):
        text += b"#" * ((i - len(text)) % 16)
        desc[i] = (len(text), len(span), s_off, expect_n)
        text += span
        s_off += expect_n + PAD
    text += b"#"
    want = np.full(s_off, CANARY, np.uint32)
    care = np.ones(s_off, bool)
    want_status = np.zeros(n, np.uint32)
    status_mask = np.full(n, 0xFFFFFFFF, np.uint32)
    for i, (span, expect_n) in enumerate(items):
        vals, o = span_reference(span), int(desc["sums_off"][i])
        if vals is None:  # bit 0, and the expect_n sums unspecified
            want_status[i], status_mask[i] = 1, 1
            care[o:o + expect_n] = False
            continue
        m = min(len(vals), expect_n)
        want[o:o + m] = np.asarray(vals[:m], dtype=np.uint32)
        if len(vals) != expect_n:
            want_status[i] = 2
            care[o + m:o + expect_n] = False
    return ParseCall(label, desc, np.frombuffer(bytes(text), np.uint8), want, care, want_status, status_mask,
                     [s for s, _ in items])


# ------------------------------------------------------------------ valid span text
class Numbers:
    """Canonical span text of exact lengths: the bulk cut from one seeded pool of random numbers of
    every digit count, the last few bytes made to measure."""

    def __init__(self, seed, n=1 << 16):
        toks = [str(v) for v in R.sum_values("random", n, seed).tolist()]
        self.text = (",".join(toks) + ",").encode()
        self.start = np.concatenate([[0], np.cumsum([len(t) + 1 for t in toks])])
        self.at = 0
        self.rng = np.random.default_rng(seed)

    def digits(self, d):
        """A canonical number of exactly d digits."""
        lo = 0 if d == 1 else 10 ** (d - 1)
        return str(int(self.rng.integers(lo, min(10 ** d, 1 << 32)))).encode()

    def commas(self, rem):
        """Numbers with a comma behind each, `rem` bytes in all (0, or at least 2)."""
        assert rem == 0 or rem >= 2
        out = []
        while rem > 24:
            i = self.at
            j = int(np.searchsorted(self.start, self.start[i] + rem - 12, "right")) - 1
            piece = self.text[self.start[i]:self.start[j]]
            out.append(piece)
            rem -= len(piece)
            self.at = j if j < len(self.start) - 1 else 0
        while rem:
            d = rem - 1 if rem <= 11 else min(int(self.rng.integers(1, 11)), rem - 3)
            out.append(self.digits(d) + b",")
            rem -= d + 1
        return b"".join(out)

    def span(self, n_bytes, starts=None):
        """A canonical span of exactly n_bytes; starts {position: digits}: a number of exactly that
        many digits begins there."""
        out, cur = [], 0
        for p in sorted(starts or ()):
            out += [self.commas(p - cur), self.digits(starts[p])]
            cur = p + starts[p]
            if cur < n_bytes:
                out.append(b",")
                cur += 1
        rem = n_bytes - cur
        if rem:
            k = rem if rem <= 10 else min(int(self.rng.integers(1, 11)), rem - 2)
            out += [self.commas(rem - k), self.digits(k)]
        s = b"".join(out)
        assert len(s) == n_bytes and not s.endswith(b",")
        return s


# ------------------------------------------------------------------ S1: scan passes
S1_COUNTS = (1, Us, Us + 1, None, 2 * Us + 1, 3, Us - 1, 0, 64, 65)  # None: null; 0: []


def _s1_blob(i, k):
    sums = None if k is None else R.sum_values("random", k, SEED + i)
    return Blob(1 << (i % 40), sums, NAMES[i % 3], (i * 2654435761) % (1 << 40))


@functools.lru_cache(maxsize=None)
def s1_blobs():
    """The one list (about 6,000 blobs) every S1 case is a prefix of, and its cumulative units."""
    blobs, cum, units = [], [], 0
    while units < max(TOTALS):
        i = len(blobs)
        blobs.append(_s1_blob(i, S1_COUNTS[i % len(S1_COUNTS)]))
        units += ser_units(blobs[-1].k)
        cum.append(units)
    return blobs, cum


def _prefix(cum, total):
    """(k, units the blob at k must keep): the blobs before k and that many units make `total`."""
    k = next(i for i, c in enumerate(cum) if c >= total)
    return k, total - (cum[k - 1] if k else 0)


@functools.lru_cache(maxsize=None)
def s1_case(total):
    blobs, cum = s1_blobs()
    k, keep = _prefix(cum, total)
    last = blobs[k]
    if ser_units(last.k) > keep:  # trimmed to a ragged last unit
        last = Blob(last.pl, last.sums[:keep * Us - 3], last.name, last.length)
    call = ser_call(f"S1 {total} units", blobs[:k] + [last])
    assert call.n_units == total
    return call


def s1_cases(totals=TOTALS):
    return [s1_case(t) for t in totals]


# ------------------------------------------------------------------ S2: last-step shapes
S2_POSITIONS = ("unit 0 step 0", "unit 0 later step", "later unit step 0")
S2_SHAPES = {(pos, phase, total) for pos in S2_POSITIONS for phase in range(4) for total in range(1, 13)}


def _last_step(doc):
    """(first sum of the final 64-sum step, its first byte's offset in the document, its bytes)."""
    a, b = R.bracket_span(doc)
    toks = doc[a:b].split(b",")
    s = (len(toks) - 1) // LANES * LANES
    off = a + sum(len(t) + 1 for t in toks[:s])
    return s, off, b - off


def s2_shape(doc, out_off):
    """(position, phase, total) of a document's final step, from the reference bytes alone; out is
    at least 4-byte aligned."""
    s, off, total = _last_step(doc)
    pos = "unit 0 step 0" if s == 0 else "unit 0 later step" if s < Us else \
        "later unit step 0" if s % Us == 0 else "later unit later step"
    return pos, (out_off + off) % 4, total


@functools.lru_cache(maxsize=None)
def s2_case():
    """One call: for every position, phase and total a blob whose final step is `total` bytes (one
    number of `total` digits, or two for 11 and 12) at that phase, reached through the header
    length (one to four PieceLength digits) and out_off % 4."""
    blobs, residues = [], []
    before = {"unit 0 step 0": 0, "unit 0 later step": LANES, "later unit step 0": Us}
    for pos in S2_POSITIONS:
        head = R.sum_values("random", before[pos], SEED + before[pos])
        for phase in range(4):
            for total in range(1, 13):
                ds = [total] if total <= 10 else [5, total - 6]
                tail = [int("1234567890"[:d]) for d in ds]
                b = Blob(10 ** ((phase + total) % 4 + 1) - 1, np.concatenate([head, np.array(tail, np.uint32)]),
                         NAMES[total % 3], phase * 100 + total)
                blobs.append(b)
                residues.append((phase - _last_step(b.doc)[1]) % 4)
    return ser_call("S2 last-step shapes", blobs, residues)


def s2_coverage(call):
    return {s2_shape(b.doc, int(o)) for b, o in zip(call.blobs, call.desc["out_off"])}


# ------------------------------------------------------------------ S3: owner search
@functools.lru_cache(maxsize=None)
def unitless(i):
    """null and [] by turns."""
    return Blob(4 + i, None if i % 2 else np.zeros(0, np.uint32), NAMES[i % 3], i)


@functools.lru_cache(maxsize=None)
def with_units(i):
    k = (3, Us + 1, 1, 64, 2 * Us, Us)[i % 6]
    return Blob(1 << (i % 33), R.sum_values("random", k, SEED + 7 * i), NAMES[i % 3], 1000 + i)


S3_RUNS = (1, 2, 3, 64, 65)
S3_ONLY_UNITLESS = (1, 300)
S3_WITH_UNITS = (1, 2, 3, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def s3_cases():
    out = []
    for r in S3_RUNS:  # head, middle, tail
        blobs = ([unitless(i) for i in range(r)] + [with_units(i) for i in range(4)] +
                 [unitless(r + 1 + i) for i in range(r)] + [with_units(4 + i) for i in range(3)] +
                 [unitless(i) for i in range(r)])
        out.append(ser_call(f"S3 runs of {r} unit-less blobs", blobs))
    for n in S3_ONLY_UNITLESS:
        out.append(ser_call(f"S3 {n} unit-less blobs only", [unitless(i) for i in range(n)]))
    for n in S3_WITH_UNITS:
        out.append(ser_call(f"S3 {n} blobs with units", [with_units(i) for i in range(n)]))
    return out


# ------------------------------------------------------------------ S4: grid stride
S4_BLOBS = G + 3


@functools.lru_cache(maxsize=None)
def s4_case():
    """G + 3 blobs of one one-digit sum (index % 10) under one header: the expected image is a
    template row with one varying byte."""
    n, stride = S4_BLOBS, bound(1) + GAP
    doc = R.serialize(4096, [0], R.NAME_MIXED, 4096)
    digit = R.bracket_span(doc)[0]
    idx = np.arange(n, dtype=np.uint64)
    desc = np.zeros(n, BLOB_DT)
    desc["sums_off"], desc["n_sums"], desc["piece_length"], desc["length"] = 2 * idx, 1, 4096, 4096
    desc["out_off"], desc["name"] = GAP + idx * stride, R.NAME_MIXED.encode()
    sums = np.full(2 * n + 1, FILLER, np.uint32)
    sums[0:2 * n:2] = idx % 10
    out_size = GAP + n * stride

    def expect():
        img = np.full(out_size, FILL, np.uint8)
        rows = img[GAP:].reshape(n, stride)
        rows[:, :len(doc)] = np.frombuffer(doc, np.uint8)
        rows[:, digit] = ord("0") + (idx % 10).astype(np.uint8)
        return img, np.full(n, len(doc), np.uint64)

    return SerCall(f"S4 {n} one-sum blobs", desc, sums, out_size, expect)


# ------------------------------------------------------------------ P1: scan passes
P1_LENGTHS = (1, 2, Up - 1, Up, Up + 1, 2 * Up + 1, 0, 3 * Up)


@functools.lru_cache(maxsize=None)
def p1_spans():
    gen = Numbers(SEED + 1)
    spans, cum, units = [], [], 0
    while units < max(TOTALS):
        spans.append(gen.span(P1_LENGTHS[len(spans) % len(P1_LENGTHS)]))
        units += parse_units(len(spans[-1]))
        cum.append(units)
    return spans, cum


@functools.lru_cache(maxsize=None)
def p1_case(total):
    spans, cum = p1_spans()
    k, keep = _prefix(cum, total)
    last = spans[k]
    if parse_units(len(last)) > keep:
        last = Numbers(SEED + total).span(keep * Up - 5)
    items = [(s, len(span_reference(s))) for s in spans[:k] + [last]]
    call = parse_call(f"P1 {total} units", items)
    assert call.n_units == total
    return call


def p1_cases(totals=TOTALS):
    return [p1_case(t) for t in totals]


# ------------------------------------------------------------------ P2: break positions
P2_LAST = 130
P2_UNITS = (0, 63, 64, 65, 127, 128, P2_LAST)
P2_AT = (0, 63, 64, Up - 1)
P2_KINDS = ("non-digit", "double comma", "leading zero")


@functools.lru_cache(maxsize=None)
def p2_base():
    """(P2_LAST + 1) whole units.  A kind needs its context (a comma in front, a digit behind), and
    two neighbouring bytes cannot both begin a number, so a two-digit number begins at in-unit
    byte 63 of every other unit of P2_UNITS and at byte 64 of the rest, at a unit's last byte
    (straddling the edge) in every other unit, and at a unit's first byte wherever the unit before
    does not straddle into it.  The span's last byte is a one-digit number."""
    starts, n_bytes = {}, (P2_LAST + 1) * Up
    for ju, u in enumerate(P2_UNITS):
        if not (ju % 2 and u - 1 in P2_UNITS):
            starts[u * Up] = 2
        starts[u * Up + (64 if ju % 2 else 63)] = 2
        if ju % 2 == 0:
            starts[u * Up + Up - 1] = 2 if u < P2_LAST else 1
    return Numbers(SEED + 2).span(n_bytes, starts)


def _p2_mutant(base, p, kind):
    """The substitution of `kind` at byte p, or None where the base lacks its context."""
    starts = p == 0 or base[p - 1:p] == b","
    if kind == "non-digit":
        c = b"x"
    elif kind == "double comma":  # right behind a comma
        c = b"," if p > 0 and starts else None
    else:  # right behind a comma (or first) and in front of a digit
        c = b"0" if starts and base[p + 1:p + 2].isdigit() and base[p:p + 1] != b"0" else None
    return None if c is None else base[:p] + c + base[p + 1:]


@functools.lru_cache(maxsize=None)
def p2_mutants():
    """[(unit, in-unit position, kind, span)]: at every position the first two kinds, counted
    round the cycle from the position's own, whose context the base has there."""
    base, out = p2_base(), []
    for idx, (u, at) in enumerate((u, at) for u in P2_UNITS for at in P2_AT):
        made = 0
        for t in range(3):
            kind = P2_KINDS[(idx + t) % 3]
            m = _p2_mutant(base, u * Up + at, kind)
            if m is not None and made < 2:
                out.append((u, at, kind, m))
                made += 1
    assert len(out) <= 64
    return out


@functools.lru_cache(maxsize=None)
def p2_case():
    """The base between two valid neighbours, then every mutant with a valid neighbour behind."""
    base = p2_base()
    nb = len(span_reference(base))
    near = Numbers(SEED + 3).span(Up + 17)
    near_item = (near, len(span_reference(near)))
    items = [near_item, (base, nb), near_item]
    for _, _, _, m in p2_mutants():
        items += [(m, nb), near_item]
    return parse_call("P2 break positions", items)


# ------------------------------------------------------------------ P3: numbers across a unit edge
P3_EDGE_UNITS = (1, 64)


def _head(n_bytes):
    """`7,7,..7,` (`17,7,..` for an odd length): a number begins right behind it."""
    return (b"1" if n_bytes % 2 else b"") + b"7," * (n_bytes // 2)


@functools.lru_cache(maxsize=None)
def p3_spans():
    """({name: malformed span}, {name: valid span}); E = j Up is the first byte of unit j."""
    bad, good = {}, {}
    for j in P3_EDGE_UNITS:
        E = j * Up
        bad[f"j={j} leading zero ends the unit"] = _head(E - 1) + b"05,7"
        for k in range(1, 11):
            bad[f"j={j} 11 digits, {k} before the edge"] = _head(E - k) + b"12345678901,7"
        for k in range(1, 10):
            bad[f"j={j} 2^32, {k} digits before the edge"] = _head(E - k) + b"4294967296,7"
        bad[f"j={j} comma ends the unit, comma begins the next"] = _head(E) + b",7"
        bad[f"j={j} trailing comma ends the span on the edge"] = _head(E)
        bad[f"j={j} the span's last byte a comma, a unit's first"] = _head(E - 1) + b"7,"
        bad[f"j={j} non-digit begins the unit"] = _head(E) + b"x,7"
        bad[f"j={j} non-digit ends the unit"] = _head(E - 1) + b"x,7,7"
        for k in range(0, 11):
            good[f"j={j} 2^32-1, {k} digits before the edge"] = _head(E - k) + b"4294967295,12,0"
        good[f"j={j} zero ends the unit, comma next"] = _head(E - 1) + b"0,7"
        good[f"j={j} zero ends the span on the edge"] = _head(E - 1) + b"0"
    return bad, good


@functools.lru_cache(maxsize=None)
def p3_case():
    """Malformed and valid by turns; a malformed span expects as many numbers as its commas say."""
    bad, good = p3_spans()
    items, g = [], list(good.values())
    for i, s in enumerate(bad.values()):
        items += [(s, s.count(b",") + 1), (g[i % len(g)], len(span_reference(g[i % len(g)])))]
    return parse_call("P3 unit edges", items)


# ------------------------------------------------------------------ P4: the count guard
@functools.lru_cache(maxsize=None)
def p4_case():
    """Two spans of three units (random numbers; one-digit numbers, 1.5 Up of them) at every
    expect_n that is not the number count -- status 2 exactly -- and once at the count."""
    gen = Numbers(SEED + 4)
    dense = ",".join(str(i % 10) for i in range(3 * Up // 2)).encode()
    items = []
    for span in (gen.span(3 * Up - 7), dense):
        assert parse_units(len(span)) == 3
        n = len(span_reference(span))
        early = len(span_reference(span[:3 * Up // 2].rsplit(b",", 1)[0]))  # the numbers of the first 1.5 units
        for expect_n in (0, 1, early, n - 1, n + 1, n + Up, n):
            items.append((span, expect_n))
    call = parse_call("P4 count guard", items)
    assert sorted(set(call.want_status.tolist())) == [0, 2] and (call.want_status == 0).sum() == 2
    return call


# ------------------------------------------------------------------ P5: owner search and stride
P5_SPANS = G + 3


@functools.lru_cache(maxsize=None)
def p5_cases():
    """Runs of empty spans (expect_n 0: status 0; expect_n 3: status 2) at the head, in the middle
    and at the tail, and calls of nothing but empty spans."""
    gen = Numbers(SEED + 5)
    full = [gen.span(n) for n in (5, Up + 1, 1, 2 * Up, Up, 64, 3)]
    full = [(s, len(span_reference(s))) for s in full]
    empty = lambda r, k: [(b"", 3 * ((i + k) % 2)) for i in range(r)]
    out = []
    for r in S3_RUNS:
        out.append(parse_call(f"P5 runs of {r} empty spans", empty(r, 0) + full[:4] + empty(r, 1) + full[4:] + empty(r, 0)))
    for n in S3_ONLY_UNITLESS:
        out.append(parse_call(f"P5 {n} empty spans only", empty(n, 0)))
    return out


@functools.lru_cache(maxsize=None)
def p5_stride_case():
    """G + 3 one-byte spans `d`, d = index % 10, one sum each: more units than workgroups in the
    count and check launches, more blobs than workgroups in the status launch."""
    n = P5_SPANS
    idx = np.arange(n, dtype=np.uint64)
    desc = np.zeros(n, SPAN_DT)
    desc["text_off"], desc["text_len"], desc["sums_off"], desc["expect_n"] = 17 * idx, 1, 1 + 2 * idx, 1
    text = np.full(17 * n + 1, ord("#"), np.uint8)
    text[17 * idx.astype(np.int64)] = ord("0") + (idx % 10).astype(np.uint8)
    want = np.full(2 * n + 1, CANARY, np.uint32)
    want[1 + 2 * idx.astype(np.int64)] = idx % 10
    return ParseCall(f"P5 {n} one-byte spans", desc, text, want, np.ones(2 * n + 1, bool), np.zeros(n, np.uint32),
                     np.full(n, 0xFFFFFFFF, np.uint32))


@functools.lru_cache(maxsize=None)
def p5_pinned_case():
    """A small mixed call for outputs in page-locked host memory."""
    bad, good = p3_spans()
    items = [(b"", 0), (good["j=1 2^32-1, 3 digits before the edge"], Up // 2), (b"", 3),
             (bad["j=1 leading zero ends the unit"], Up // 2 + 1), (b"1,2,3,4", 3), (b"0", 1)]
    return parse_call("P5 page-locked outputs", items)


# ------------------------------------------------------------------ backends
class HostBackend:
    """krk_metainfo_serialize a blob; krk_metainfo_parse of a span inside a canonical envelope
    (KRK_OK and the values, or KRK_EFORMAT).  No device."""

    def __init__(self):
        h, t = R.serialize(4, [], R.NAME_LOWER, 9).split(b"[]")
        self.head, self.tail = h + b"[", b"]" + t

    def reserve(self, calls):
        pass

    def serialize(self, call):
        out = np.full(call.out_size, FILL, np.uint8)
        lens = np.zeros(call.n, np.uint64)
        ln = C.c_uint64()
        for i, d in enumerate(call.desc):
            k = int(d["n_sums"])
            s = call.sums[int(d["sums_off"]):int(d["sums_off"]) + k]
            check(lib.krk_metainfo_serialize(int(d["piece_length"]), s.ctypes.data if k else None, k, int(d["sums_null"]),
                                             bytes(d["name"]), 64, int(d["length"]),
                                             out.ctypes.data + int(d["out_off"]), bound(k), C.byref(ln)))
            lens[i] = ln.value
        return out, lens

    def parse(self, call):
        """The status a host caller derives: bit 0 on KRK_EFORMAT (nothing stored, the count
        unknown), else bit 1 by the count, and the first min(count, expect_n) values."""
        sums = np.full(call.want.size, CANARY, np.uint32)
        status = np.zeros(call.n, np.uint32)
        n, pl, ln, null = C.c_uint64(), C.c_int64(), C.c_int64(), C.c_int()
        name = C.create_string_buffer(64)
        text = call.text.tobytes()
        for i, d in enumerate(call.desc):
            doc = self.head + text[int(d["text_off"]):int(d["text_off"]) + int(d["text_len"])] + self.tail
            cap = (len(doc) + 1) // 2
            tmp = np.zeros(cap, np.uint32)
            rc = lib.krk_metainfo_parse(doc, len(doc), C.byref(pl), tmp.ctypes.data, cap, C.byref(n), C.byref(null), name,
                                        C.byref(ln))
            if rc == KRK_EFORMAT:
                status[i] = 1
                continue
            assert rc == KRK_OK and not null.value, (call.label, i, rc)
            m = min(int(n.value), int(d["expect_n"]))
            sums[int(d["sums_off"]):int(d["sums_off"]) + m] = tmp[:m]
            status[i] = 0 if n.value == d["expect_n"] else 2
        return sums, status


class DeviceBackend:
    """The two _batch_dev entry points: one set of buffers, sized by reserve() for the largest call
    and prefilled before every call, freed by close()."""

    def __init__(self):
        from kraken_amd import device as D
        self.D, self.bufs = D, {}

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def close(self):
        for b in self.bufs.values():
            b.free()
        self.bufs = {}

    def _buf(self, name, nbytes):
        b = self.bufs.get(name)
        if b is None or b.nbytes < nbytes:
            if b is not None:
                b.free()
            b = self.bufs[name] = self.D.DeviceBuffer(max(nbytes, 16))
        return b

    def reserve(self, calls):
        need = {}
        for c in calls:
            if isinstance(c, SerCall):
                sizes = {"sums": c.sums.nbytes, "out": c.out_size, "lens": 8 * c.n}
            else:
                sizes = {"text": c.text.nbytes, "sums_out": c.want.nbytes, "status": 4 * c.n}
            for name, nbytes in sizes.items():
                need[name] = max(need.get(name, 0), nbytes)
        for name, nbytes in need.items():
            self._buf(name, nbytes)

    def serialize(self, call):
        n = call.n
        sums, out, lens = self._buf("sums", call.sums.nbytes), self._buf("out", call.out_size), self._buf("lens", 8 * n)
        assert out.ptr % 4 == 0  # S2 takes its phases from out_off alone
        sums.from_host(call.sums)
        out.from_host(np.full(call.out_size, FILL, np.uint8))
        lens.from_host(np.full(8 * n, FILL, np.uint8))
        check(lib.krk_metainfo_serialize_batch_dev(C.cast(call.desc.ctypes.data, BLOBP), n, sums.ptr, out.ptr, lens.ptr,
                                                   None))
        check(lib.krk_stream_sync(None))
        return out.to_host(np.uint8, call.out_size), lens.to_host(np.uint64, n)

    def parse(self, call, pinned=False):
        n, D = call.n, self.D
        text = self._buf("text", call.text.nbytes)
        text.from_host(call.text)
        if pinned:
            sums, status = D.PinnedArray((call.want.size,), np.uint32), D.PinnedArray((n,), np.uint32)
            sums.a[:] = CANARY
            status.a.view(np.uint8)[:] = FILL
        else:
            sums, status = self._buf("sums_out", call.want.nbytes), self._buf("status", 4 * n)
            sums.from_host(np.full(call.want.size, CANARY, np.uint32))
            status.from_host(np.full(4 * n, FILL, np.uint8))
        check(lib.krk_metainfo_parse_sums_batch_dev(C.cast(call.desc.ctypes.data, SPANP), n, text.ptr, sums.ptr,
                                                    status.ptr, None))
        check(lib.krk_stream_sync(None))
        if pinned:
            return sums.a.copy(), status.a.copy()
        return sums.to_host(np.uint32, call.want.size), status.to_host(np.uint32, n)


# ------------------------------------------------------------------ comparison
def compare_ser(call, got):
    """Mismatches of one call's (out, out_len) against the whole expected buffers, as text."""
    out, lens = got
    img, want_len = call.expect()
    bad = []
    if not np.array_equal(lens, want_len):
        i = int(np.flatnonzero(lens != want_len)[0])
        bad.append(f"{call.label}: out_len[{i}] is {int(lens[i])}, want {int(want_len[i])}")
    diff = np.flatnonzero(out != img)
    if diff.size:
        at = int(diff[0])
        i = max(int(np.searchsorted(call.desc["out_off"], at, "right")) - 1, 0)
        bad.append(f"{call.label}: {diff.size} bytes differ, the first at {at} ({at - int(call.desc['out_off'][i])} "
                   f"into blob {i}'s slot): {int(out[at]):#x}, want {int(img[at]):#x}")
    return bad


def compare_parse(call, got):
    """Mismatches of one call's (sums_out, status): every specified word, every canary, and the
    status under its mask."""
    sums, status = got
    bad = []
    diff = np.flatnonzero((sums != call.want) & call.care)
    if diff.size:
        at = int(diff[0])
        i = max(int(np.searchsorted(call.desc["sums_off"], at, "right")) - 1, 0)
        bad.append(f"{call.label}: {diff.size} sums words differ, the first at {at} (span {i}, sums_off "
                   f"{int(call.desc['sums_off'][i])}, expect_n {int(call.desc['expect_n'][i])}): {int(sums[at]):#x}, "
                   f"want {int(call.want[at]):#x}")
    diff = np.flatnonzero((status & call.status_mask) != call.want_status)
    if diff.size:
        i = int(diff[0])
        bad.append(f"{call.label}: {diff.size} status words differ, the first span {i}: {int(status[i]):#x}, want "
                   f"{int(call.want_status[i]):#x} under {int(call.status_mask[i]):#x}")
    return bad


def run_cases(backend, calls, **kw):
    """(calls made, mismatches): every call once through the backend."""
    backend.reserve(calls)
    bad = []
    for c in calls:
        if isinstance(c, SerCall):
            bad += compare_ser(c, backend.serialize(c))
        else:
            bad += compare_parse(c, backend.parse(c, **kw))
    return len(calls), bad
