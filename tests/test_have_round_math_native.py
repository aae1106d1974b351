"""tests/native/have_round_main.cpp: have_round_math.hpp as a stand-alone CPU program (its own main,
nothing of the library linked) under ASan + UBSan, run directly over the small cases of
tests/have_round_cases.py, every span in a heap block of exactly its size, against the reference."""
import os
import subprocess

from tests import have_round_cases as M
from tests import have_round_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_have_round_math_under_asan_ubsan(tmp_path):
    src = os.path.join(ROOT, "tests", "native", "have_round_main.cpp")
    exe = str(tmp_path / "have_round_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    ts = [t for label, (ts, _) in M.cases().items() if label != "above the unit cap" for t in ts if t.n <= 130]
    lines, want = [], []
    for t in ts:
        status = t.status if t.flags & R.RESTORE else b""
        nums = [t.n, t.flags, t.piece_length, t.length, *t.caps, len(status), *status]
        nums += M.words(t.row).view("i8").tolist() + M.words(t.ok).view("i8").tolist()  # as signed: scanf reads long long
        lines.append(" ".join(str(int(x)) for x in nums))
        row, o = R.round_torrent(t.row, t.n, t.flags, t.piece_length, t.length, t.status, t.ok, *t.caps)
        want.append([o["flags"], o["n_unexpected"], o["n_changed"], o["n_complete"], o["bytes"], *o["changed"], *(o["missing"] or []),
                     *(o["status_out"] or b""), *(o["wire_out"] or b""), *M.words(row).tolist()])
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr
    assert [[int(x) for x in line.split()] for line in r.stdout.splitlines()] == want
