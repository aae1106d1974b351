"""tests/native/request_table_main.cpp: the request table round's host arithmetic
(kraken_amd/csrc/request_table_math.hpp, what krk_request_table_round runs and request_table.hip
equals) as a stand-alone CPU program (its own main, nothing of the library linked) built with
AddressSanitizer and UndefinedBehaviorSanitizer and run directly over the named cases of
tests/request_table_matrix.py: what it prints is held against the hand-worked values and against
tests/request_table_ref.py."""
import os
import subprocess

from tests import request_table_matrix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_request_table_math_under_asan_ubsan(tmp_path):
    src = os.path.join(ROOT, "tests", "native", "request_table_main.cpp")
    exe = str(tmp_path / "request_table_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    named, lines = M.named(), []
    for b, _ in named:
        t, o, a = b.torrents[0], b.offs[0], b.arrays
        W = (t.n + 63) // 64
        nums = [t.n, t.P, t.flags, t.cap, b.limit, b.now, b.timeout, int(b.has_picks), len(t.table)]
        nums += [x for e in t.table for x in e]
        for name in M.LISTS:
            nums += [len(t.ev[name])] + b.lists[name][o[name] * M.WIDTH[name]:].tolist()[:len(t.ev[name]) * M.WIDTH[name]]
        nums += a["bits"][o["w"]:o["w"] + (1 + 2 * t.P) * W].view("i8").tolist()  # as signed: scanf reads long long
        nums += a["picks"][o["p"] * b.limit:(o["p"] + t.P) * b.limit].tolist()
        lines.append(" ".join(str(int(x)) for x in nums + a["n_picked"][o["p"]:o["p"] + t.P].tolist()))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(named)
    for (b, hand), line in zip(named, out):
        t, o, w, got = b.torrents[0], b.offs[0], b.want(), [int(x) for x in line.split()]
        ne, nd, quota, nf = got[0], got[1], got[2:2 + t.P], got[2 + t.P]
        failed = got[3 + t.P:3 + t.P + 3 * nf]
        mine = {"n_entries": ne, "n_dropped": nd, "quota": quota, "failed": [tuple(failed[k:k + 3]) for k in range(0, 3 * nf, 3)]}
        assert all(mine[k] == v for k, v in hand.items()), (b.label, mine, hand)
        want = [int(w["n_entries"][0]), int(w["n_dropped"][0])] + w["quota"][o["p"]:o["p"] + t.P].astype("i4").tolist()
        want += [int(w["n_failed"][0])] + w["failed"][3 * o["e"]:3 * (o["e"] + nf)].tolist()
        want += [int(x) for e in w["entries"][o["e"]:o["e"] + ne].tolist() for x in (e[0], e[1], e[2], e[4])]
        want += w["bits"][o["w"]:o["w"] + (1 + 2 * t.P) * ((t.n + 63) // 64)].tolist()
        assert got == want, b.label
