"""Cleanup plans from a listing's text where no GPU is: the host form krk_cleanup_plan over the
cleanup-plan matrix (tests/cleanup_plan_matrix.py) against its numpy transcription, against the
unfused chain (krk_digest_parse_hex -> krk_expiry_bits -> krk_ring_select with or_bits over the
valid-only sublisting), the matrix's own shape, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from kraken_amd import _capi, hashring
from kraken_amd._capi import check, lib
from tests import cleanup_plan_matrix as M

CANARY = M.CANARY


@pytest.fixture(scope="module")
def data():
    return M.Data()


def host_parse(data):
    def parse(n):
        d = np.zeros((n, 32), dtype=np.uint8)
        v = np.zeros(M.words(n), dtype=np.uint64)
        check(lib.krk_digest_parse_hex(data.text.ctypes.data, data.off.ctypes.data_as(M.u64p), n, d.ctypes.data, None,
                                       v.ctypes.data_as(M.u64p) if n else None))
        return d, v
    return parse


def host_select(digests, mask, invert, or_bits):
    return hashring.select_host(digests, mask, invert, or_bits)[1]


def test_matrix_shapes_and_reference(data):
    W, T = M.W, M.T
    assert len(M.INVALID) >= 12 and not set(M.INVALID) & set(M.R.EDGES) and len(M.SPECIAL) >= 6
    assert {data.kinds[p] for p in M.INVALID} == {"byte", "short", "empty"}
    assert any(p in (W - 2, W + 1) for p in M.INVALID) and any(p in (T * W - 2, T * W + 1) for p in M.INVALID)
    assert int(data.off[M.INVALID[1] + 2]) % 2 == 1  # the 63-character name moves the later names to odd offsets
    # the saturating transcription against Python's integers
    t = np.array([M.I64_MIN, M.I64_MAX, 0, -1, 1, M.NOW - M.TTL, M.NOW - M.TTL - 1], dtype=np.int64)
    for now in (M.NOW, M.NEG_NOW, 0, M.I64_MIN, M.I64_MAX):
        want = [min(max(now - int(x), M.I64_MIN), M.I64_MAX) for x in t]
        assert M.sat_sub(now, t).tolist() == want, now
    # the special mtimes do what the contract says, under a mask that selects nothing
    n = M.N_MAX
    _, idx, _ = data.reference(M.Case(n, "zeros", False, "mtime"))
    sel = set(idx.tolist())
    for k, p in enumerate(M.SPECIAL):
        assert (p in sel) == (k % 3 != 0), (p, k)
    assert not sel & set(M.INVALID)
    _, idx, _ = data.reference(M.Case(n, "zeros", False, "negative now"))
    sel = set(idx.tolist())
    for k, p in enumerate(M.SPECIAL + list(M.R.EDGES)):
        assert (p in sel) == (k % 4 in (1, 2)), (p, k)  # INT64_MAX and now - ttl are not expired
    # ones with every invalid name's mtime expired: everything but the invalid names
    _, idx, valid = data.reference(M.Case(n, "ones", False, "mtime"))
    assert idx.size == n - len(M.INVALID) and not set(idx.tolist()) & set(M.INVALID)
    assert not M.R._unpack(valid, n)[M.INVALID].any()
    # edges without mtimes: exactly the EDGES
    for m in M.SHAPES:
        _, idx, _ = data.reference(M.Case(m, "edges", False, "none"))
        assert idx.tolist() == [e for e in M.R.EDGES if e < m]


def test_host_plan_small_shapes_every_cap(data):
    calls, bad = M.run_cases(M.HostBackend(data), M.cases(M.SMALL))
    assert calls > 0 and bad == [], bad[:5]


def test_host_plan_scan_tile_shapes(data):
    host = M.HostBackend(data)
    every = [c for c in M.cases(M.LARGE) if c.mask == "edges" and c.times == "none"]  # its list is the EDGES below n
    calls, bad = M.run_cases(host, every)
    calls2, bad2 = M.run_cases(host, [c for c in M.cases(M.LARGE) if c not in every], all_caps=False)
    assert calls and calls2 and bad + bad2 == [], (bad + bad2)[:5]


def test_host_plan_equals_the_unfused_chain(data):
    host = M.HostBackend(data)
    for case in M.cases((65, M.W + 1, M.T * M.W + 1)):
        want = data.reference(case)
        idx, valid = M.chain(data, case, host_parse(data), host_select)
        assert np.array_equal(idx, want[1]), case.label
        assert np.array_equal(M.R._pack(valid)[:M.words(case.n)], want[2]), case.label
        cap = int(want[1].size) + M.SPARE
        assert M.compare(case, cap, host.run(case, cap), want) == [], case.label


def test_host_plan_refusals(data):
    mask = data.masks["random"].ctypes.data_as(M.u64p)
    out = np.full(8, CANARY, dtype=np.uint64)
    op = out.ctypes.data_as(M.u64p)
    t, o, mt = data.text.ctypes.data, data.off.ctypes.data_as(M.u64p), data.mtime.ctypes.data_as(M.i64p)
    E = _capi.KRK_EINVAL

    def call(t, o, mask, bits, idx, cap, count):
        return lib.krk_cleanup_plan(t, o, 2, mt, M.NOW, M.TTL, mask, 1, bits, None, idx, cap, count)

    assert call(None, o, mask, op, None, 0, op) == E
    assert call(t, None, mask, op, None, 0, op) == E
    assert call(t, o, None, op, None, 0, op) == E
    assert call(t, o, mask, None, None, 0, op) == E
    assert call(t, o, mask, op, None, 0, None) == E
    assert call(t, o, mask, op, None, 1, op) == E  # NULL idx, cap 1
    assert b"cleanup_plan" in lib.krk_last_error()
    assert (out == CANARY).all()
    assert lib.krk_expiry_bits(mt, None, 2, M.NOW, M.TTL, 0, None) == E
    assert lib.krk_digest_parse_hex(None, o, 2, out.ctypes.data, None, None) == E
    assert lib.krk_digest_parse_hex(t, None, 2, out.ctypes.data, None, None) == E
    assert lib.krk_digest_parse_hex(t, o, 2, None, None, None) == E
    assert lib.krk_digest_format_hex(None, 2, out.ctypes.data) == E
    assert lib.krk_digest_format_hex(t, 2, None) == E
    assert (out == CANARY).all()
    # n == 0 with NULL arrays: the count is written, 0
    assert lib.krk_cleanup_plan(None, None, 0, None, M.NOW, M.TTL, mask, 1, None, None, None, 0, op) == _capi.KRK_OK
    assert out.tolist() == [0] + [int(CANARY)] * 7


def test_dev_entry_points_without_a_device(data):
    """A refusal needs no device; a real call needs a gfx950 device: KRK_ENODEV here when there is
    none, never a fall-back to the host forms (with one, tests/test_gpu_cleanup_plan_matrix.py and
    tests/test_gpu_digest_hex_matrix.py)."""
    from kraken_amd import device as D
    mask = data.masks["random"].ctypes.data_as(M.u64p)
    out = np.full(64, CANARY, dtype=np.uint64)
    o = out.ctypes.data
    t, off = data.text.ctypes.data, data.off.ctypes.data
    E = _capi.KRK_EINVAL
    assert lib.krk_cleanup_plan_dev(t, off, 2, None, M.NOW, M.TTL, None, 1, o, None, None, 0, o + 64, None) == E
    assert lib.krk_cleanup_plan_dev(None, off, 2, None, M.NOW, M.TTL, mask, 1, o, None, None, 0, o + 64, None) == E
    assert lib.krk_cleanup_plan_dev(t, off, 2, None, M.NOW, M.TTL, mask, 1, o, None, None, 3, o + 64, None) == E
    assert lib.krk_digest_parse_hex_dev(None, off, 2, o, None, None, None) == E
    assert lib.krk_digest_parse_hex_dev(t, off, 2, None, None, None, None) == E
    assert lib.krk_digest_format_hex_dev(None, 2, o, None) == E
    assert lib.krk_digest_format_hex_dev(o, 2, None, None) == E
    if D.device_count() == 0:
        N = _capi.KRK_ENODEV
        assert lib.krk_cleanup_plan_dev(t, off, 2, None, M.NOW, M.TTL, mask, 1, o, None, None, 0, o + 64, None) == N
        assert lib.krk_cleanup_plan_dev(None, None, 0, None, M.NOW, M.TTL, mask, 1, None, None, None, 0, o, None) == N
        assert lib.krk_digest_parse_hex_dev(t, off, 2, o, None, None, None) == N
        assert lib.krk_digest_format_hex_dev(o, 2, o + 128, None) == N
        assert (out == CANARY).all()
