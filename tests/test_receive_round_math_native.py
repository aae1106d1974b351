"""tests/native/receive_round_main.cpp: receive_round_math.hpp as a stand-alone CPU program (its own
main, nothing of the library linked) under ASan + UBSan, run directly over the small cases of
tests/receive_round_cases.py, every span in a heap block of exactly its size, against the reference."""
import os
import subprocess

from tests import receive_round_cases as M
from tests import receive_round_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_receive_round_math_under_asan_ubsan(tmp_path):
    src = os.path.join(ROOT, "tests", "native", "receive_round_main.cpp")
    exe = str(tmp_path / "receive_round_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    ts = [t for ts in M.cases().values() for t in ts if len(t.pays) <= M.CHUNK + 1]
    lines, want = [], []
    for t in ts:
        nums = [t.n, t.slots, t.length, t.piece_length, len(t.pays), M.NOW, *M.words(t.have).view("i8").tolist(), *t.expected,
                *(x & 0xFFFFFFFF for q in t.pays for x in q), *t.sums]  # as signed 64-bit or unsigned 32-bit: scanf reads long long
        lines.append(" ".join(str(int(x)) for x in nums))
        have, touched = list(t.have), {}
        out, arrived, marks, good, dup, totals = R.round_torrent(have, t.n, t.length, t.piece_length, t.pays, t.sums, t.expected, M.NOW, touched)
        want.append([len(arrived), len(marks), *totals, *(x for o in out for x in o), *(x for a in arrived for x in a),
                     *(x for m in marks for x in m), *(x for p in range(t.slots) for x in (good.get(p, 0), dup.get(p, 0), touched.get(p, -1))),
                     *M.words(have).tolist()])
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr
    assert [[int(x) for x in line.split()] for line in r.stdout.splitlines()] == want
