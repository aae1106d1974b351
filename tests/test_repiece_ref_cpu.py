"""tests/repiece_ref.py, the plain-Python GF(2) reference group F of the re-piece matrix is
judged by, pinned to zlib.crc32 on real bytes: the combine identity, and re-pieced sums against
sums computed over the bytes at the new piece length."""
import zlib

import numpy as np
import pytest

from tests import repiece_ref as R

DATA = np.random.default_rng(20261021).integers(0, 256, size=70_000, dtype=np.uint8).tobytes()


def _sums(blob, piece):
    return [zlib.crc32(blob[a:a + piece]) for a in range(0, len(blob), piece)]


def test_shift_and_combine_against_zlib():
    assert R.shift(0x12345678, 0) == 0x12345678 and R.shift(0, 1000) == 0
    for la, lb in [(0, 0), (0, 5), (5, 0), (1, 1), (3, 4096), (4096, 3), (12345, 54321)]:
        a, b = DATA[:la], DATA[la:la + lb]
        assert R.combine(zlib.crc32(a), zlib.crc32(b), lb) == zlib.crc32(a + b), (la, lb)
    # shifting is linear and composes: shift(shift(c, m), n) == shift(c, m + n)
    c, d = 0xDEADBEEF, 0x0BADF00D
    assert R.shift(c ^ d, 777) == R.shift(c, 777) ^ R.shift(d, 777)
    assert R.shift(R.shift(c, 1 << 33), (1 << 40) + 5) == R.shift(c, (1 << 33) + (1 << 40) + 5)


@pytest.mark.parametrize("po", [1, 3, 64, 4096])
def test_repiece_against_zlib(po):
    for ratio in (1, 2, 3, 5, 63, 64, 65, 129):
        for length in (0, 1, po - 1, po, po + 1, po * ratio - 1, po * ratio, po * ratio + 1, 2 * po * ratio + po // 2 + 1,
                       min(len(DATA), 3 * po * ratio + 7)):
            if length < 0 or length > len(DATA) or length > 40_000 * po:
                continue
            blob = DATA[:length]
            assert R.repiece(_sums(blob, po), length, po, po * ratio) == _sums(blob, po * ratio), (po, ratio, length)
    blob = DATA[:9999]
    assert R.repiece(_sums(blob, po), len(blob), po, po * 10_000) == [zlib.crc32(blob)]
