"""The engine matrix harness (tests/engine_matrix.py) checked where no GPU is: every edge its
docstring names is in the lists, the groups stay within their byte and reference-call caps, and the
same plans on KRK_PLACE_HOST pass the same comparison code -- the references, the step decoding and
the mismatch reporting are right before the engine is involved, and host_meta.cpp's tail buffer and
the host piece loop are pinned at the same edges."""
import json
import os
import subprocess
import sys

import pytest

from kraken_amd._capi import KRK_PLACE_HOST
from tests import engine_matrix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, Q, I = M.S, M.Q, M.I


def _inside(plans):
    return all(0 <= p.off and p.off + p.total <= M.ARENA_BYTES for p in plans)


def _writes(p):
    return [s[1] for s in p.steps if s[0] == "w"]


def _paths(p):
    """The branches of krk_digester_write (GPU placement) plan p takes, from the code: `direct` a
    whole slot from the caller's buffer (fill == 0, n >= S), `fill` a write that ends inside the
    slot or exactly fills it, `cross` a write that starts inside a slot and goes on past its end."""
    out, fill = set(), 0
    for n in _writes(p):
        first = True
        while n:
            if fill == 0 and n >= S:
                out.add("direct")
                n -= S
            else:
                take = min(n, S - fill)
                if first and fill and n > take:
                    out.add("cross")
                if fill + take == S:
                    out.add("fill")
                fill = (fill + take) % S
                n -= take
            first = False
    return out


def test_constants():
    assert (M.S, M.B, M.I, M.Q) == (524288, 64, 262144, 8)
    assert M.ARENA_BYTES >= max(M.C_SIZES) and M.ARENA_BYTES >= M.A4_TOTAL


def test_group_a1_tails():
    a1 = M.plans_a1()
    iv = [p for p in a1 if p.name.startswith("A1 iv")]
    row = [p for p in a1 if p.name.startswith("A1 row")]
    assert [p.total for p in iv] == list(range(131))
    assert [p.total - S for p in row] == list(range(64)) + [119, 120]
    # every padding residue, and both sides of the one-block / two-block padding edge (55 | 56)
    for ps in (iv, row):
        assert {p.total % 64 for p in ps} == set(range(64))
        assert {55, 56, 64 + 55, 64 + 56} <= {p.total % S for p in ps}
    # one call each, then one sum; the empty message is a zero-length write
    assert all(len(_writes(p)) == (1 if p.total else 0) and p.steps[-1] == M.SUM for p in a1)
    assert iv[0].steps == (M.Z_PTR, M.SUM)
    assert _inside(a1)


def test_group_a2_slot_edge():
    a2 = M.plans_a2()
    assert M.A2_TOTALS == (S - 1, S, S + 1, 2 * S, 2 * S + 1, 3 * S + 17)
    assert len(a2) == 6 * 9 and _inside(a2)
    for T in M.A2_TOTALS:
        mine = {p.name.split(" ", 2)[2]: p for p in a2 if p.total == T}
        assert set(mine) == set(M.A2_SPLITS) and len(M.A2_SPLITS) == 9
        w = {k: _writes(p) for k, p in mine.items()}
        assert all(sum(x) == T and 0 not in x for x in w.values())
        assert w["whole"] == [T] and w["zeros"] == [T]
        assert w["1+rest"] == [1, T - 1]
        assert w["S-1+rest"][0] == S - 1 and w["S-1+1+rest"][:2] == [S - 1, 1][:len(w["S-1+1+rest"])]
        assert w["S+rest"][0] == min(S, T) and w["S+1+rest"][0] == min(S + 1, T)
        assert w["63+1+rest"] == [63, 1, T - 64]
        assert w["130x1+rest"] == [1] * 130 + [T - 130]
        z = mine["zeros"].steps
        k = z.index(M.W(T))
        assert {M.Z_NULL, M.Z_PTR} <= set(z[:k]) and {M.Z_NULL, M.Z_PTR} <= set(z[k + 1:])
        assert z[-1] == M.SUM and z.count(M.SUM) == 2 and M.Z_NULL in z[z.index(M.SUM):]
        assert all(p.steps[-1] == M.SUM for p in mine.values())
    assert set().union(*[_paths(p) for p in a2]) == {"direct", "fill", "cross"}
    assert _paths(next(p for p in a2 if p.name == f"A2 T={2 * S} whole")) == {"direct"}
    assert "cross" in _paths(next(p for p in a2 if p.name == f"A2 T={S + 1} 1+rest"))


def test_group_a3_sum_placement():
    a3 = M.plans_a3()
    assert len(a3) == 6 * 2 + 5 and _inside(a3)
    for T in M.A2_TOTALS:
        for split in ("S-1+1+rest", "1+rest"):
            p = next(p for p in a3 if p.name.startswith(f"A3 T={T} {split} "))
            assert _writes(p) == M.split_writes(T, split)
            assert [s[0] for s in p.steps] == ["w", "s"] * len(_writes(p))
    named = {p.name: p.steps for p in a3[12:]}
    assert named == {
        "A3 sum; sum": (M.SUM, M.SUM),
        "A3 sum at 0, writes, sum": (M.SUM, M.W(100), M.W(S), M.SUM),
        "A3 sum at S, one byte, sum": (M.W(S), M.SUM, M.W(1), M.SUM),
        "A3 sum at 2S, one byte, sum": (M.W(2 * S), M.SUM, M.W(1), M.SUM),
        "A3 sum at S-1 pending, write(1), sum": (M.W(S - 1), M.SUM, M.W(1), M.SUM),
    }


def test_groups_a4_a5_and_the_cap():
    a4 = M.plans_a4()
    assert [p.total for p in a4] == [(Q + 2) * S + 1] * 2 and M.A4_TOTAL // S > Q
    assert _writes(a4[0]) == [M.A4_TOTAL]
    assert set(_writes(a4[1])[:-1]) == {S // 2 + 1} and sum(_writes(a4[1])) == M.A4_TOTAL
    a5 = M.plans_a5()
    assert [p.steps for p in a5] == [(M.W(2 * S),), (M.W(S + 1), M.SUM), (M.SUM,)]
    everything = M.plans_a() + a5
    assert len(M.plans_a()) == 197 + 54 + 17 + 2 and _inside(everything)
    assert M.CAP_A_BYTES == 192 << 20 and sum(p.total for p in everything) <= M.CAP_A_BYTES


def test_group_b_cases():
    assert set(M.B_PIECES) == {1, 3, 63, 64, 65, 4096, 65536, I - 1, I, I + 1, S // 2, S - 1, S, S + 1, 2 * S,
                               2 * S + 1, 4 * S}
    assert len(M.B_PIECES) == len(set(M.B_PIECES)) == 16  # S / 2 is I
    b = M.plans_b()
    assert _inside(b) and {p.P for p in b} == set(M.B_PIECES)
    for P in M.B_PIECES:
        mine = [p for p in b if p.P == P and p.total != M.A4_TOTAL]
        want = {0, 1, P - 1, P, P + 1, S, S + 1, 2 * S + P + 1} | ({2 * S} if S % P == 0 else set())
        if P <= 3:
            want = {t for t in want if t <= S + 3}
        want = {min(t, 3 * S + 17) for t in want}
        assert {p.total for p in mine} == want, P
        for T in want:
            ws = {p.name.rsplit(" ", 1)[1]: list(p.writes) for p in mine if p.total == T}
            assert ws["whole"] == ([T] if T else [])
            assert all(sum(x) == T and 0 not in x for x in ws.values())
            # each split is there unless its writes equal an earlier one's
            distinct = []
            for split in M.B_SPLITS:
                x = M.piece_writes(T, P, split)
                if x is not None and x not in distinct:
                    distinct.append(x)
                    assert ws[split] == x, (P, T, split)
            assert len(ws) == len(distinct) <= 4
            if T > S:
                assert any(x[:T // S] == [S] * (T // S) for x in ws.values())
            if T > 1:
                assert [1, T - 1] in ws.values()
            if P >= 4096 and T > P:
                assert any(x[:T // P] == [P] * (T // P) for x in ws.values())
            assert len({p.off for p in mine if p.total == T}) == 1  # one view, one reference a total
        assert sum(1 for p in mine if p.erange) == 1 and all(p.total > 0 for p in mine if p.erange)
    big = [p for p in b if p.total == M.A4_TOTAL]
    assert len(big) == 1 and big[0].P == S + 1 and big[0].writes == ((Q + 2) * S + 1,)
    assert len(b) == 285
    assert (M.CAP_B_BYTES, M.CAP_B_CRC_CALLS) == (256 << 20, 3_000_000)
    assert sum(p.total for p in b) <= M.CAP_B_BYTES and M.crc_calls_b(b) <= M.CAP_B_CRC_CALLS


def test_group_c_cases():
    assert M.C_SIZES == (Q * S - 1, Q * S, Q * S + 1, (Q + 1) * S + 5, 12 * S)
    assert M.C_SEEDS == (0, 1, 0x80000000, 0xFFFFFFFF)
    c = M.cases_c()
    assert all(0 <= x.off and x.off + x.n <= M.ARENA_BYTES for x in c)
    for n in M.C_SIZES:
        assert len({x.seed for x in c if x.n == n}) == 2
    for seed in M.C_SEEDS:
        assert sum(1 for x in c if x.seed == seed) >= 2
    # requests a call: exactly Q (nothing retired early) and more (retired while submitting)
    assert sorted({-(-x.n // S) for x in c}) == [Q, Q + 1, Q + 2, 12]
    assert M.CAP_C_BYTES == 64 << 20 and sum(x.n for x in c) <= M.CAP_C_BYTES


def test_group_d_and_e_cases():
    dig, pcs = M.crowd_d()
    assert len(dig) == len(set(dig)) == 32 and len(pcs) == len(set(pcs)) == 32
    assert {p.P for p in pcs} == set(M.B_PIECES)
    assert {p.name.split(" ", 2)[2] for p in dig if p.name.startswith("A2")} == set(M.A2_SPLITS)
    assert sum(1 for p in dig if p.name.startswith("A3")) == 17
    e = M.plans_e()
    assert len(e) == 54 + 17 + 2 and M.E_LIVE == 40


@pytest.mark.parametrize("group,count", [("A", 273), ("B", 285), ("C", 10)])
def test_groups_pass_on_the_host(group, count):
    n, nbytes, _, bad = M.run_group_counted(group, KRK_PLACE_HOST)
    assert n == count and nbytes > 0
    assert bad == []


def test_crowd_harness_runs_on_the_host():
    """Group D's barrier and job code, where the placement has no engine to coalesce anything (the
    coalescing condition is the GPU test's)."""
    n, nbytes, _, bad = M.run_group_counted("D", KRK_PLACE_HOST)
    assert n == 32 + 32 + 4 and nbytes > 0
    assert bad == []


@pytest.mark.parametrize("group", ["A", "B", "C"])
def test_reporting_detects_one_flipped_value(group):
    bad = M.run_group_counted(group, KRK_PLACE_HOST, flip=True)[3]
    assert len(bad) == 1, bad[:3]
    desc, got, want = bad[0]
    assert desc.startswith(group)
    if group == "A":
        assert int(got, 16) ^ int(want, 16) == 1 << 248
    else:
        assert got ^ want == 1


def test_command_line_on_the_host():
    r = subprocess.run([sys.executable, "-m", "tests.engine_matrix", "--host"], capture_output=True, text=True,
                       cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert [x["group"] for x in lines] == ["A", "B", "C"]
    assert all(x["n_mismatches"] == 0 and x["mismatches"] == [] for x in lines)
    assert [x["cases"] for x in lines] == [273, 285, 10]
