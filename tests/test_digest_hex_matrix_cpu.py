"""The SHA-256 hex codec where no GPU is: the host forms krk_digest_parse_hex and
krk_digest_format_hex over the digest-hex matrix (tests/digest_hex_matrix.py) against its
plain-Python transcription -- every byte value, every position, the lengths, every text alignment
-- and the matrix's own shape."""
import numpy as np
import pytest

from tests import digest_hex_matrix as M


@pytest.fixture(scope="module")
def data():
    return M.Data()


def test_matrix_shapes_and_content(data):
    G = M.G
    assert G % 256 == 0 and M.N_MAX == 3 * G + 37
    st = [s for s, _ in data.ref["injected"]]
    assert st[0] == M.KRK_DHEX_LEN | 63
    sweep = st[1:257]
    assert [s == 0 for s in sweep] == [bytes([b]) in (b"0123456789abcdefABCDEF"[i:i + 1] for i in range(22))
                                       for b in range(256)]
    assert all(s == M.KRK_DHEX_BYTE | (b & 63) << 8 | b for b, s in enumerate(sweep) if s)
    for b in b"/:@G`g\x00\x80\xff":
        assert sweep[b] != 0
    assert st[257:321] == [M.KRK_DHEX_BYTE | p << 8 | 0x67 for p in range(64)]
    assert st[321] == M.KRK_DHEX_BYTE | 9 << 8 | 0x2F
    assert st[322:327] == [M.KRK_DHEX_LEN | k for k in (0, 1, 65, 66, 128)]
    assert st[327] == M.KRK_DHEX_LEN | 40 and st[328] == M.KRK_DHEX_BYTE | 0x67
    # the mixed listing: an odd-length name early, so later names start at odd offsets
    _, off = data.pack("mixed", 65, 0)
    assert off[2] % 2 == 0 and off[3] % 2 == 1 and off[64] % 2 == 1
    assert all(s == 0 for s, _ in data.ref["aligned"])


def test_host_parse_every_shape_lead_and_listing(data):
    calls, bad = M.run_parse(M.HostBackend(data), M.cases())
    assert calls > 0 and bad == [], bad[:5]


def test_host_parse_text_and_digests_at_odd_addresses(data):
    calls, bad = M.run_parse(M.HostBackend(data, text_shift=1, out_shift=1), M.cases((65, M.G + 1)))
    assert calls > 0 and bad == [], bad[:5]


def test_host_format_and_round_trip(data):
    for b in (M.HostBackend(data), M.HostBackend(data, text_shift=1, out_shift=3)):
        calls, bad = M.run_format(b)
        assert calls > 0 and bad == [], bad[:5]
        assert M.run_round_trip(b) == []


def test_a_decreasing_offset_pair_is_a_length_error():
    """len is the unsigned difference: nothing of that name is read, the next name is unharmed."""
    b = M.HostBackend(None)
    off = np.array([64, 0, 64], dtype=np.uint64)
    n, dig, status, valid = b.parse_text(b"a" * 64, off, 2)
    assert status[:2].tolist() == [M.KRK_DHEX_LEN | 0x3FFFFFFF, 0] and int(valid[0]) == 2
    assert not dig[:32].any() and (dig[32:64] == 0xAA).all()
