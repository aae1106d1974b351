"""SHA-256 in plain Python integers: the independent reference for midstates, which hashlib
cannot export (FIPS 180-4 sections 4.1.2, 5.1.1, 6.2.2).  A helper module for the tests,
no library calls; meant for inputs of a few KiB."""

M32 = 0xFFFFFFFF

IV = (0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19)

K = (
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
    0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
    0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2,
)


def _rotr(x, n):
    return ((x >> n) | (x << (32 - n))) & M32


def compress(h8, block64):
    """One compression: the 8-word chaining value after the 64-byte block."""
    assert len(h8) == 8 and len(block64) == 64
    w = [int.from_bytes(block64[4 * i:4 * i + 4], "big") for i in range(16)]
    for i in range(16, 64):
        s0 = _rotr(w[i - 15], 7) ^ _rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)
        s1 = _rotr(w[i - 2], 17) ^ _rotr(w[i - 2], 19) ^ (w[i - 2] >> 10)
        w.append((w[i - 16] + s0 + w[i - 7] + s1) & M32)
    a, b, c, d, e, f, g, h = (int(x) for x in h8)
    for i in range(64):
        # the rotations written out (a call per rotation doubles the time of a block)
        s1 = ((e >> 6 | e << 26) ^ (e >> 11 | e << 21) ^ (e >> 25 | e << 7)) & M32
        s0 = ((a >> 2 | a << 30) ^ (a >> 13 | a << 19) ^ (a >> 22 | a << 10)) & M32
        t1 = h + s1 + ((e & f) ^ (~e & g)) + K[i] + w[i]
        t2 = s0 + ((a & b) ^ (a & c) ^ (b & c))
        a, b, c, d, e, f, g, h = (t1 + t2) & M32, a, b, c, (d + t1) & M32, e, f, g
    return tuple((int(x) + y) & M32 for x, y in zip(h8, (a, b, c, d, e, f, g, h)))


def resume(h8, absorbed, data, final):
    """Continue a chain whose midstate after `absorbed` bytes (a multiple of 64) is h8.
    Non-final: data is whole blocks, the 8-word midstate after them is returned.  Final: the
    32-byte digest, padded with 0x80, zeros and the 64-bit big-endian bit length of
    absorbed + len(data)."""
    data = bytes(data)
    assert absorbed % 64 == 0
    h = tuple(int(x) for x in h8)
    if not final:
        assert len(data) % 64 == 0
    else:
        total = absorbed + len(data)
        data += b"\x80" + b"\x00" * ((55 - len(data)) % 64) + ((total * 8) & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "big")
        assert len(data) % 64 == 0
    for o in range(0, len(data), 64):
        h = compress(h, data[o:o + 64])
    return b"".join(x.to_bytes(4, "big") for x in h) if final else h
