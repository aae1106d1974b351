"""The CRC matrix harness (tests/crc_matrix.py) checked where no GPU is: its case lists are
what the module says they are, and the same blobs, as host views through krk_piece_sums_host
on the HOST placement, pass the same comparison code -- the expected values, the layout
decoding and the mismatch reporting are right before a kernel is involved."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from kraken_amd import _capi
from kraken_amd._capi import check, lib
from tests import crc_matrix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host():
    check(lib.krk_set_crc_placement(_capi.KRK_PLACE_HOST))
    yield M.HostBackend(cus=256)
    check(lib.krk_set_crc_placement(_capi.KRK_PLACE_AUTO))


def _inside(blobs):
    return all(0 <= b.off and b.off + b.L + M.SPARE <= M.ARENA_BYTES and b.L > 0 for b in blobs)


def test_group_a_cases():
    ls = M.lengths_a()
    assert len(ls) == len(set(ls)) == 11 * 19 - 1 + 3 and 0 not in ls
    # one item each (at most kItemBytes) but the two lengths past it, which take two items
    assert sorted(L for L in ls if L > M.K_ITEM) == [M.K_ITEM + 1, M.K_ITEM + M.K_STEP + 3]
    assert {L // M.K_STEP for L in ls if L <= M.K_ITEM} == set(range(9)) | {62, 63, 64}
    blobs = M.cases_a()
    n_short = sum(1 for L in ls if L // M.K_STEP < 62)
    assert len(blobs) == 2 * (9 * n_short + 3 * (len(ls) - n_short)) == 3306
    assert _inside(blobs)
    # every length at every alignment of its set, once a whole piece and once a partial one
    for L in ls:
        mine = [b for b in blobs if b.L == L]
        al = M.ALIGNS_LONG if L // M.K_STEP >= 62 else M.ALIGNS
        assert sorted(b.off % 16 for b in mine if b.P == L) == sorted(al), L
        assert sorted(b.off % 16 for b in mine if b.P == L + 1) == sorted(al), L
        assert len(mine) == 2 * len(al)
    # every tail in the list at every alignment (the step counts below 62 carry all nine)
    for t in M.TAILS:
        for al in M.ALIGNS:
            assert any(b.L % M.K_STEP == t and b.off % 16 == al for b in blobs), (t, al)
    assert 100e6 < sum(b.L for b in blobs) < 250e6


def test_group_b_cases():
    blobs = M.cases_b()
    assert len(blobs) == 10 * 3 * 2 == 60 and _inside(blobs)
    assert {b.P for b in blobs} == set(M.B_PIECES) and {b.off % 16 for b in blobs} == {0, 5}
    for P in M.B_PIECES:
        assert sorted(b.L for b in blobs if b.P == P) == sorted(2 * [3 * P, 3 * P + 1, 4 * P - 1])
    # more than one item a piece with a short last item, but for 262143 and 262144
    assert sum(1 for P in M.B_PIECES if P > M.K_ITEM and P % M.K_ITEM) == 7


def test_group_c_cases():
    assert M.populations(256) == [1, 15, 16, 17, 4095, 4096, 4097, 8191, 8193, 12293, 16385]
    cases = M.cases_c(256)
    assert [(n, kind) for n, kind, _ in cases] == [(n, k) for n in M.populations(256) for k in ("run", "items")]
    for n, kind, blobs in cases:
        assert _inside(blobs)
        if kind == "run":
            assert len(blobs) == 1 and blobs[0].P == 64 and M.n_pieces(blobs[0]) == n and blobs[0].L == 64 * n
        else:
            assert len(blobs) == n == len({b.off for b in blobs})
            assert all(b.L == 100 and b.P == 101 for b in blobs)
    assert sum(len(b) for _, _, b in cases) == 11 + sum(M.populations(256)) == 57410


def test_group_d_and_e_cases():
    blobs = M.cases_d()
    assert len(blobs) == 6 and _inside(blobs) and all(b.L == 3 * b.P + 777 for b in blobs)
    rng = np.random.default_rng(1)
    for b in blobs:
        cuts = M.cuts_d(b, rng)
        assert cuts[0] == 0 and cuts[-1] == b.L and cuts == sorted(set(cuts))
        assert all(c % 64 == 0 for c in cuts[:-1])
        for k in range(1, M.n_pieces(b)):  # a cut within 32 bytes of every piece boundary
            assert min(abs(c - k * b.P) for c in cuts) <= 32
        for k in range(M.n_pieces(b)):
            if k * b.P + M.K_ITEM < b.L:
                assert min(abs(c - (k * b.P + M.K_ITEM)) for c in cuts) <= 32
    e = M.cases_e()
    assert len(e) == 5 * 13 == 65 and all(off + n + M.SPARE <= M.ARENA_BYTES for _, n, off in e)
    assert {off % 16 for _, _, off in e} == set(range(16))


@pytest.mark.parametrize("group,count", [("A", 3306), ("B", 3306 + 2 * 60), ("C", 57410)])
def test_groups_pass_on_the_host(host, group, count):
    n, bad = M.run_group_counted(group, host)
    assert n == count
    assert bad == []


@pytest.mark.parametrize("group", ["A", "B", "C"])
def test_reporting_detects_one_flipped_sum(host, group):
    bad = M.run_group(group, host, flip=0)
    assert len(bad) == 1, bad[:3]
    desc, got, want = bad[0]
    assert desc.startswith(group) and "blob 0 " in desc and "piece 0" in desc and got ^ want == 1


def test_reporting_names_guards_and_gaps():
    blobs = [M.Blob(0, 10, 4), M.Blob(64, 5, 5)]
    offs = [M.GUARD, M.GUARD + 3]
    want = np.arange(M.GUARD * 2 + 4, dtype=np.uint32)
    got = want.copy()
    got[0] ^= 1           # a guard word
    got[M.GUARD + 1] ^= 1  # blob 0, piece 1
    got[M.GUARD + 2] ^= 1  # blob 0 again: reported once
    got[M.GUARD + 3] ^= 2  # blob 1
    bad = M.compare("X", blobs, offs, got, want)
    assert [d.split(" off=")[0] for d, _, _ in bad] == ["X word 0 outside every blob's sums (guard or gap)",
                                                        "X blob 0", "X blob 1"]
    assert "piece 1" in bad[1][0] and bad[2][1] ^ bad[2][2] == 2


def test_command_line_on_the_host():
    r = subprocess.run([sys.executable, "-m", "tests.crc_matrix", "--host"], capture_output=True, text=True,
                       cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert [x["group"] for x in lines] == ["A", "B", "C"]
    assert all(x["variant"] is None and x["n_mismatches"] == 0 and x["mismatches"] == [] for x in lines)
    assert [x["cases"] for x in lines] == [3306, 3426, 57410]
