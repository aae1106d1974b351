"""The SHA-256 hex codec (digest_hex.hip, digest_hex_math.hpp) at its lane, wave and workgroup
edges and at every text alignment: the cases, their expectations and the comparison, shared by
tests/test_gpu_digest_hex_matrix.py (krk_digest_parse_hex_dev / krk_digest_format_hex_dev on the
production library) and tests/test_digest_hex_matrix_cpu.py (the host forms the kernels are
documented to equal).  A helper module, not a test file.

Every parse case is a prefix of ONE listing of N_MAX names: random-case valid names with the
INJECTED names at every ninth position from 2 on -- the first of them has 63 characters, so every
later name starts at an odd offset -- and ALIGNED, valid names only, for the wholly aligned text.
INJECTED holds: all 256 byte values (name b has byte b at position b & 63, valid exactly when b is
a hex digit); 'g' at each of the 64 positions; two bad bytes in one name (the lower position is
reported); the lengths 0, 1, 63, 65, 66 and 128; a 40-character name that also holds a bad byte
(the length error wins); and 64 x 'g'.  A case packs its names behind `lead` junk bytes (off[0] =
lead), and a backend may place the text and the digest output at a byte shift of its own.  The
expectation is a plain-Python transcription of the contract (bytes.fromhex and a character set),
never the library.  G (the names a workgroup takes) is read from the built library
(krk_digest_hex_geometry); shapes: 0, 1, 63, 64, 65, G - 1, G, G + 1, 3 G + 37.  Outputs are
prefilled with 0xFF bytes and carry SPARE entries past their end: every documented byte is stored
and nothing past it."""
import ctypes as C

import numpy as np

from kraken_amd._capi import check, lib

SEED = 20261021
SPARE = 4
KRK_DHEX_LEN, KRK_DHEX_BYTE = 0x40000000, 0x80000000
HEX = b"0123456789abcdefABCDEF"
LEADS = (0, 1, 3, 7, 13)
u64p = C.POINTER(C.c_uint64)


def geometry():
    g = C.c_uint64()
    check(lib.krk_digest_hex_geometry(C.byref(g)))
    return int(g.value)


G = geometry()
N_MAX = 3 * G + 37
SHAPES = (0, 1, 63, 64, 65, G - 1, G, G + 1, N_MAX)


def words(n):
    return (n + 63) // 64


def ref_parse(name: bytes):
    """(status, 32 digest bytes) of the contract, a byte at a time."""
    if len(name) != 64:
        return KRK_DHEX_LEN | min(len(name), 0x3FFFFFFF), bytes(32)
    for p, c in enumerate(name):
        if c not in HEX:
            return KRK_DHEX_BYTE | p << 8 | c, bytes(32)
    return 0, bytes.fromhex(name.decode("ascii"))


def _valid_names(rng, n):
    """n random digests as hex with a random case a letter."""
    out = []
    for row, up in zip(rng.integers(0, 256, size=(n, 32), dtype=np.uint8), rng.random((n, 64)) < 0.5):
        h = bytes(row).hex().encode()
        out.append(bytes(c - 32 if u and c >= 0x61 else c for c, u in zip(h, up)))
    return out


def injected(rng):
    v = iter(_valid_names(rng, 400))

    def put(name, *at):
        b = bytearray(name)
        for p, c in at:
            b[p] = c
        return bytes(b)

    out = [next(v)[:63]]  # first: odd length, every later name starts at an odd offset
    out += [put(next(v), (b & 63, b)) for b in range(256)]
    out += [put(next(v), (p, 0x67)) for p in range(64)]
    out.append(put(next(v), (40, 0x78), (9, 0x2F)))  # 'x' at 40 and '/' at 9: position 9 is reported
    out += [b"", b"a", b"a" * 65, b"a" * 66, b"a" * 128]
    out.append(put(next(v)[:40], (3, 0x7A)))
    out.append(b"g" * 64)
    return out


class Data:
    """The shared listings and their expectations, built once and left unchanged."""

    def __init__(self):
        rng = np.random.default_rng(SEED)
        self.injected = injected(rng)
        names = _valid_names(rng, N_MAX)
        for k, name in enumerate(self.injected):
            names[2 + 9 * k] = name
        assert 2 + 9 * (len(self.injected) - 1) < N_MAX
        self.listings = {"mixed": names, "aligned": _valid_names(rng, 130), "injected": self.injected}
        self.ref = {k: [ref_parse(x) for x in v] for k, v in self.listings.items()}
        self.format_digests = np.concatenate([np.arange(256, dtype=np.uint8),
                                              rng.integers(0, 256, size=32 * N_MAX - 256, dtype=np.uint8)])
        self.format_digests.setflags(write=False)

    def pack(self, listing, n, lead):
        """(text bytes: `lead` junk bytes then the first n names back to back, off uint64 [n + 1])."""
        names = self.listings[listing][:n]
        off = np.zeros(n + 1, dtype=np.uint64)
        off[0] = lead
        if n:
            off[1:] = lead + np.cumsum([len(x) for x in names], dtype=np.uint64)
        return b"g" * lead + b"".join(names), off

    def reference(self, listing, n):
        """(digests uint8 [32 n], status uint32 [n], valid uint64 [words(n)])."""
        r = self.ref[listing][:n]
        status = np.array([s for s, _ in r], dtype=np.uint32)
        ok = np.zeros(words(n) * 64, dtype=np.uint8)
        ok[:n] = status == 0
        return (np.frombuffer(b"".join(d for _, d in r), dtype=np.uint8), status,
                np.packbits(ok, bitorder="little").view(np.uint64))


class Case:
    def __init__(self, listing, n, lead=0, nullable=False):
        self.listing, self.n, self.lead, self.nullable = listing, n, lead, nullable
        self.label = f"{listing} n={n} off[0]={lead}" + (" status=valid=NULL" if nullable else "")


def cases(shapes=SHAPES):
    """Every shape of the mixed listing at off[0] = 0, the other leads at 65 and G + 1 names, the
    aligned and the injected listings whole at every lead, and the nullable outputs left out."""
    out = [Case("mixed", n) for n in shapes]
    out += [Case("mixed", n, lead) for n in (65, G + 1) for lead in LEADS[1:]]
    out += [Case(k, None, lead) for k in ("aligned", "injected") for lead in LEADS]
    out += [Case("mixed", G + 1, 3, nullable=True), Case("injected", None, 1, nullable=True)]
    return out


# ------------------------------------------------------------------ backends
class HostBackend:
    """krk_digest_parse_hex / krk_digest_format_hex: no device.  text_shift and out_shift place the
    text and the digest (or hex) output that many bytes past an aligned base."""

    def __init__(self, data, text_shift=0, out_shift=0):
        self.data, self.text_shift, self.out_shift = data, text_shift, out_shift

    def parse(self, case):
        n = len(self.data.listings[case.listing]) if case.n is None else case.n
        return self.parse_text(*self.data.pack(case.listing, n, case.lead), n, case.nullable)

    def parse_text(self, text, off, n, nullable=False):
        buf = np.zeros(len(text) + self.text_shift + 1, dtype=np.uint8)
        buf[self.text_shift:self.text_shift + len(text)] = np.frombuffer(text, dtype=np.uint8)
        dig = np.full(32 * n + SPARE + self.out_shift, 0xFF, dtype=np.uint8)
        status = np.full(n + SPARE, 0xFFFFFFFF, dtype=np.uint32)
        valid = np.full(words(n) + SPARE, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        check(lib.krk_digest_parse_hex(buf.ctypes.data + self.text_shift, off.ctypes.data_as(u64p), n,
                                       dig.ctypes.data + self.out_shift,
                                       None if nullable else status.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       None if nullable else valid.ctypes.data_as(u64p)))
        return n, dig[self.out_shift:], status, valid

    def format(self, digests, n):
        d = np.zeros(32 * n + self.text_shift + 1, dtype=np.uint8)
        d[self.text_shift:self.text_shift + 32 * n] = digests[:32 * n]
        hex_ = np.full(64 * n + SPARE + self.out_shift, 0xFF, dtype=np.uint8)
        check(lib.krk_digest_format_hex(d.ctypes.data + self.text_shift, n, hex_.ctypes.data + self.out_shift))
        return hex_[self.out_shift:]


class DeviceBackend:
    """krk_digest_parse_hex_dev / krk_digest_format_hex_dev: inputs uploaded a call, outputs in
    device memory or, with pinned, in krk_host_alloc memory."""

    def __init__(self, data, text_shift=0, out_shift=0, pinned=False):
        from kraken_amd import device as D
        self.D, self.data, self.text_shift, self.out_shift, self.pinned = D, data, text_shift, out_shift, pinned

    def _out(self, nbytes):
        D = self.D
        if self.pinned:
            o = D.PinnedArray((nbytes,), np.uint8)
            o.a[:] = 0xFF
        else:
            o = D.DeviceBuffer(nbytes)
            o.from_host(np.full(nbytes, 0xFF, dtype=np.uint8))
        return o

    def _get(self, o, dtype):
        return (o.a.copy() if self.pinned else o.to_host(np.uint8)).view(dtype)

    def parse(self, case):
        n = len(self.data.listings[case.listing]) if case.n is None else case.n
        return self.parse_text(*self.data.pack(case.listing, n, case.lead), n, case.nullable)

    def parse_text(self, text, off, n, nullable=False):
        D = self.D
        tbuf = D.DeviceBuffer(len(text) + self.text_shift + 1)
        tbuf.from_host(np.frombuffer(text, dtype=np.uint8), offset=self.text_shift)
        obuf = D.DeviceBuffer(off.nbytes)
        obuf.from_host(off)
        pad = -(32 * n + SPARE + self.out_shift) % 8
        dig = self._out(32 * n + SPARE + self.out_shift + pad)
        status, valid = self._out(4 * (n + SPARE)), self._out(8 * (words(n) + SPARE))
        check(lib.krk_digest_parse_hex_dev(tbuf.ptr + self.text_shift, obuf.ptr, n, dig.ptr + self.out_shift,
                                           None if nullable else status.ptr,
                                           None if nullable else valid.ptr, None))
        check(lib.krk_stream_sync(None))
        return (n, self._get(dig, np.uint8)[self.out_shift:32 * n + SPARE + self.out_shift], self._get(status, np.uint32),
                self._get(valid, np.uint64))

    def format(self, digests, n):
        D = self.D
        dbuf = D.DeviceBuffer(32 * n + self.text_shift + 1)
        dbuf.from_host(np.ascontiguousarray(digests[:32 * n]), offset=self.text_shift)
        pad = -(64 * n + SPARE + self.out_shift) % 8
        hex_ = self._out(64 * n + SPARE + self.out_shift + pad)
        check(lib.krk_digest_format_hex_dev(dbuf.ptr + self.text_shift, n, hex_.ptr + self.out_shift, None))
        check(lib.krk_stream_sync(None))
        return self._get(hex_, np.uint8)[self.out_shift:64 * n + SPARE + self.out_shift]


# ------------------------------------------------------------------ comparison
def compare_parse(data, case, got):
    """Mismatches of one parse call against reference() as text."""
    n, dig, status, valid = got
    wd, ws, wv = data.reference(case.listing, n)
    bad, tag = [], case.label
    if not np.array_equal(dig[:32 * n], wd):
        i = int(np.flatnonzero(dig[:32 * n] != wd)[0])
        bad.append(f"{tag}: digest byte {i % 32} of name {i // 32} is {int(dig[i]):#x}, want {int(wd[i]):#x}")
    if not (dig[32 * n:32 * n + SPARE] == 0xFF).all():
        bad.append(f"{tag}: a byte past the {n} digests was written")
    if case.nullable:
        if not ((status == 0xFFFFFFFF).all() and (valid == 0xFFFFFFFFFFFFFFFF).all()):
            bad.append(f"{tag}: an output passed as NULL was written")
        return bad
    if not np.array_equal(status[:n], ws):
        i = int(np.flatnonzero(status[:n] != ws)[0])
        bad.append(f"{tag}: status[{i}] is {int(status[i]):#x}, want {int(ws[i]):#x}")
    if not (status[n:] == 0xFFFFFFFF).all():
        bad.append(f"{tag}: a status word past {n} was written")
    if not np.array_equal(valid[:words(n)], wv):
        w = int(np.flatnonzero(valid[:words(n)] != wv)[0])
        bad.append(f"{tag}: valid word {w} is {int(valid[w]):#x}, want {int(wv[w]):#x}")
    if not (valid[words(n):] == 0xFFFFFFFFFFFFFFFF).all():
        bad.append(f"{tag}: a valid word past {words(n)} was written")
    return bad


def run_parse(backend, case_list):
    calls, bad = 0, []
    for case in case_list:
        bad += compare_parse(backend.data, case, backend.parse(case))
        calls += 1
    return calls, bad


def run_format(backend, shapes=SHAPES):
    """Format over every shape of format_digests (whose first 256 bytes are the 256 byte values)
    against bytes.hex(), and nothing stored past the 64 n characters."""
    calls, bad = 0, []
    src = backend.data.format_digests
    for n in shapes:
        got = backend.format(src, n)
        want = np.frombuffer(bytes(src[:32 * n]).hex().encode(), dtype=np.uint8)
        if not np.array_equal(got[:64 * n], want):
            i = int(np.flatnonzero(got[:64 * n] != want)[0])
            bad.append(f"format n={n}: character {i % 64} of digest {i // 64} is {int(got[i]):#x}, want {int(want[i]):#x}")
        if not (got[64 * n:64 * n + SPARE] == 0xFF).all():
            bad.append(f"format n={n}: a byte past the {n} names was written")
        calls += 1
    return calls, bad


def run_round_trip(backend, n=G + 1):
    """Format then parse gives the digests back, every name valid."""
    src = backend.data.format_digests
    hex_ = backend.format(src, n)[:64 * n]
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(64)
    _, dig, status, valid = backend.parse_text(hex_.tobytes(), off, n)
    ok = np.zeros(words(n) * 64, dtype=np.uint8)
    ok[:n] = 1
    bad = []
    if not np.array_equal(dig[:32 * n], src[:32 * n]):
        bad.append(f"round trip n={n}: the digests differ")
    if status[:n].any() or not np.array_equal(valid[:words(n)], np.packbits(ok, bitorder="little").view(np.uint64)):
        bad.append(f"round trip n={n}: a formatted name is not valid")
    return bad
