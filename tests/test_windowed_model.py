"""kraken_amd.windowed's host-side pieces, pinned (no device): the window plan, the host-lane
planner and the tail-handoff simulator on rank 0's shard of an 8-GPU C3 at 1/64 scale, to the
values they gave before the module's schedule wrapper, window-time model and handover rule
were each made one; the chain-piece splitter and the window layout at their edges.  The rates
are injected, so nothing here depends on the machine."""
import json
import os

import numpy as np
import pytest

from kraken_amd import windowed as WN
from kraken_amd.shard import lpt_shard

RATES = {"sha_stream_bps": [58.5e6, 52.3e6, 35.2e6], "d2h_bps": 56e9, "h2d_bps": 56e9, "host_sha_bps": 2.1e9,
         "host_crc_bps": 17e9, "host_copy_bps": 30e9, "cus": 256, "source": 2}
CHUNK = 64 << 10


@pytest.fixture(scope="module")
def shard():
    L = WN.c3_lengths(20000, scale=64)
    lens = [L[i] for i in lpt_shard(L, 8)[0]]
    assert len(lens) == 2500
    return lens


def test_window_plan_pinned(shard):
    """1,758 windows at 200 live; the first, the middle and the last window's blob indices,
    offsets and chunk lengths equal the recorded ones (tests/golden/window_plan_c3_shard.json)."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "window_plan_c3_shard.json")) as f:
        want = json.load(f)
    wins = WN.window_plan(shard, 200 * CHUNK, 200)
    assert len(wins) == want["windows"] == 1758
    assert sorted(want["picked"]) == ["0", "1757", "879"]
    for k, (blobs, offs, take) in want["picked"].items():
        got = wins[int(k)]
        assert np.array_equal(got[0], np.array(blobs, dtype=np.int64)), k
        assert np.array_equal(got[1], np.array(offs, dtype=np.uint64)), k
        assert np.array_equal(got[2], np.array(take, dtype=np.uint64)), k


def test_host_lane_plan_pinned(shard):
    k, t, t0 = WN.host_lane_plan(None, shard, 48 << 24, 200, 15, rates=RATES)
    assert k == 1440
    assert t == pytest.approx(0.5682950961904758, rel=1e-9, abs=0)
    assert t0 == pytest.approx(2.385831914529915, rel=1e-9, abs=0)


@pytest.mark.parametrize("H,cap,end_s,host_bytes,takeovers", [
    (0, 2500, 0.28676266666666833, 0, 0),
    (0, 200, 1.9880566837606308, 0, 0),
    (3, 2500, 0.25546523076923205, 1745763731, 297),
    (3, 200, 1.2303624957264718, 8796819594, 1065),
    (15, 2500, 0.1857669743589749, 6469936756, 966),
    (15, 200, 0.4842935441036893, 17373103160, 2100)])
def test_tail_handoff_model_pinned(shard, H, cap, end_s, host_bytes, takeovers):
    m = WN.simulate_tail_handoff(shard, cap * CHUNK, cap, H, RATES, launch_s=0.0, max_chunk=CHUNK)
    assert m["end_s"] == pytest.approx(end_s, rel=1e-9, abs=0)
    assert (m["host_bytes"], m["takeovers"]) == (host_bytes, takeovers)
    if (H, cap) == (15, 200):
        assert m["gpu_end_s"] == pytest.approx(0.4839581538461577, rel=1e-9, abs=0)


FIRST = WN.TAIL_FIRST_PIECE


@pytest.mark.parametrize("y,L,piece,first", [
    (4096, 4096, 64 << 20, 0),                                   # y == L: one empty piece
    (64, 64 + FIRST - 1, 64 << 20, FIRST - 1),                   # L - y below the first piece
    (64, 64 + FIRST, 64 << 20, FIRST),                           # equal to it
    (64, 64 + FIRST + 1, 64 << 20, FIRST),                       # one above: a 1-byte second piece
    (0, 5 * (1 << 20) + 3, 1 << 20, 1 << 20),                    # piece < TAIL_FIRST_PIECE: the first is `piece`
    (128, 128 + 4 * (1 << 20), 1 << 20, 1 << 20),                # L - y an exact multiple of piece
    (192, 192 + FIRST + 3 * (16 << 20), 16 << 20, FIRST),        # ... after the short first piece
])
def test_chain_pieces_tile_the_chain(y, L, piece, first):
    pieces = WN.chain_pieces(y, L, piece)
    assert pieces[0] == (y, first)
    pos = y
    for o, m in pieces:  # in order, no gap, no overlap
        assert o == pos and 0 <= m <= piece
        pos += m
    assert pos == L
    if y == L:
        assert pieces == [(y, 0)]
    else:
        assert all(m > 0 for _, m in pieces)
        assert all(m == piece for _, m in pieces[1:-1])  # whole pieces between the first and the last


@pytest.mark.parametrize("align", [16, 256])
def test_pack_aligned_disjoint_from_the_base(align):
    lengths = [0, 1, 15, 16, 17, 255, 256, 257]
    for base in (0x7F0000000000, 0xFFFFFFFF00):  # the second: addresses cross 2^40 carries
        for ln in (lengths, lengths[::-1], [257], []):
            dev = WN._pack(base, np.array(ln, dtype=np.uint64), align)
            assert dev.dtype == np.uint64 and dev.size == len(ln)
            if not ln:
                continue
            assert int(dev[0]) == base
            assert all(int(a) % align == 0 for a in dev)
            for j in range(len(ln) - 1):  # spans in order, none overlapping the next
                assert int(dev[j]) + ln[j] <= int(dev[j + 1])
                assert int(dev[j + 1]) - int(dev[j]) < ln[j] + align  # and packed: less than `align` of padding
