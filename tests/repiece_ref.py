"""A plain-Python GF(2) reference for re-piecing stored CRC-32 piece sums to a coarser piece
length, independent of the library's arithmetic: polynomials are Python integers in the NORMAL
bit order (bit i = the coefficient of x^i, P = 0x104C11DB7), the library's are bit-reflected
32-bit words; a new piece's sum is folded left to right, acc = shift(acc, |piece|) ^ sum(piece)
(crc(A || B) = shift(crc(A), |B|) ^ crc(B) on finalised sums), where the library shifts every old
sum to the new piece's end in one step.  tests/test_repiece_ref_cpu.py pins this module to
zlib.crc32 on real bytes.  A helper module, not a test file."""
from functools import lru_cache

P = 0x104C11DB7


def _rev32(v: int) -> int:
    return int(f"{v:032b}"[::-1], 2)


def _mod(a: int) -> int:
    while a.bit_length() > 32:
        a ^= P << (a.bit_length() - 33)
    return a


def _mul(a: int, b: int) -> int:
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        b >>= 1
    return _mod(r)


@lru_cache(maxsize=None)
def x_pow_8n(n: int) -> int:
    """x^(8 n) mod P, normal bit order."""
    r, base, e = 1, 2, 8 * n
    while e:
        if e & 1:
            r = _mul(r, base)
        base = _mul(base, base)
        e >>= 1
    return r


def shift(c: int, n: int) -> int:
    """c * x^(8 n) mod P on a finalised (reflected) CRC value."""
    return _rev32(_mul(_rev32(c), x_pow_8n(n)))


def combine(crc_a: int, crc_b: int, len_b: int) -> int:
    """crc(A || B) from crc(A), crc(B) and |B|."""
    return shift(crc_a, len_b) ^ crc_b


def num_pieces(length: int, piece_length: int) -> int:
    return (length + piece_length - 1) // piece_length


def repiece(sums, length: int, piece_length: int, new_piece_length: int) -> list:
    """The sums of the pieces of new_piece_length bytes from those of piece_length bytes."""
    assert piece_length > 0 and new_piece_length % piece_length == 0 and length >= 0
    k = new_piece_length // piece_length
    n_old = num_pieces(length, piece_length)
    assert len(sums) == n_old
    out = []
    for first in range(0, n_old, k):
        acc = 0
        for i in range(first, min(first + k, n_old)):
            acc = combine(acc, int(sums[i]), min(piece_length, length - i * piece_length))
        out.append(acc)
    return out
