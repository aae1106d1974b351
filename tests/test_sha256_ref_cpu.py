"""The plain-Python SHA-256 reference (tests/sha256_ref.py) against hashlib, and the production
library's host continuation (krk_sha256_resume_host) against it at 64-bit absorbed counts.  No
device: the library is loaded, no device call is made."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from kraken_amd._capi import check, lib
from tests import sha256_ref as R

LENS = list(range(0, 201)) + [255, 256, 257, 1000, 4096 + 3]


@pytest.fixture(scope="module")
def data():
    return np.random.default_rng(2024).integers(0, 256, size=8192, dtype=np.uint8).tobytes()


def test_resume_from_iv_is_sha256(data):
    for n in LENS:
        d = data[:n]
        assert R.resume(R.IV, 0, d, True) == hashlib.sha256(d).digest(), n


def test_compress_kat():
    """FIPS 180-4 'abc': one padded block from the IV."""
    block = b"abc\x80" + b"\x00" * 59 + b"\x18"
    h = R.compress(R.IV, block)
    assert b"".join(x.to_bytes(4, "big") for x in h).hex() == \
        "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"


def test_resume_chained_at_every_block_boundary(data):
    for n in (0, 1, 63, 64, 65, 119, 120, 128, 200, 640, 1000):
        d = data[7:7 + n]
        want = hashlib.sha256(d).digest()
        for cut in range(0, n + 1, 64):
            mid = R.resume(R.IV, 0, d[:cut], False)
            assert R.resume(mid, cut, d[cut:], True) == want, (n, cut)
        # ... and block by block
        h, pos = R.IV, 0
        while n - pos >= 64:
            h = R.resume(h, pos, d[pos:pos + 64], False)
            pos += 64
        assert R.resume(h, pos, d[pos:], True) == want, n


ABSORBED = [64, (1 << 29) - 64, 1 << 29, (1 << 32) - 64, 1 << 32, (1 << 32) + (1 << 29), 1 << 40, 1 << 60]
FINAL_LENS = [0, 1, 55, 56, 63, 64, 119, 120, 200]


def _resume_host(state, absorbed, d, final):
    st = np.array(state, dtype=np.uint32)
    buf = np.frombuffer(d, dtype=np.uint8).copy() if d else np.zeros(1, dtype=np.uint8)
    dg = np.full(32, 0xA5, dtype=np.uint8)
    check(lib.krk_sha256_resume_host(st.ctypes.data_as(C.POINTER(C.c_uint32)), absorbed, C.c_void_p(buf.ctypes.data),
                                     len(d), int(final), dg.ctypes.data_as(C.POINTER(C.c_uint8))))
    return tuple(int(x) for x in st), dg.tobytes()


@pytest.mark.parametrize("absorbed", ABSORBED)
def test_resume_host_matches_reference(data, absorbed):
    """krk_sha256_resume_host from random midstates: the final form at every tail shape (the
    bit length's high word is nonzero from 2^29 absorbed bytes on) and the non-final form,
    whose state is updated in place and whose digest buffer stays untouched."""
    rng = np.random.default_rng(absorbed % 1000003)
    for k, n in enumerate(FINAL_LENS):
        state = tuple(int(x) for x in rng.integers(0, 1 << 32, size=8, dtype=np.uint64))
        d = data[100 * k:100 * k + n]
        _, dg = _resume_host(state, absorbed, d, True)
        assert dg == R.resume(state, absorbed, d, True), (absorbed, n)
    for blocks in (0, 1, 2, 3):
        state = tuple(int(x) for x in rng.integers(0, 1 << 32, size=8, dtype=np.uint64))
        d = data[3000:3000 + 64 * blocks]
        st, dg = _resume_host(state, absorbed, d, False)
        assert st == R.resume(state, absorbed, d, False), (absorbed, blocks)
        assert dg == b"\xa5" * 32, (absorbed, blocks)
