"""tests/native/peer_round_main.cpp: the peer round's host arithmetic
(kraken_amd/csrc/peer_round_math.hpp, what krk_peer_round runs and peer_round.hip equals) as a
stand-alone CPU program (its own main, nothing of the library linked) built with AddressSanitizer
and UndefinedBehaviorSanitizer and run directly over the named cases of tests/peer_round_cases.py --
the byte offsets, the malformed spans -- each span in a heap block of exactly its own size: what it
prints is held against tests/peer_round_ref.py."""
import os
import subprocess

from tests import peer_round_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_peer_round_math_under_asan_ubsan(tmp_path):
    src = os.path.join(ROOT, "tests", "native", "peer_round_main.cpp")
    exe = str(tmp_path / "peer_round_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    named, lines = M.named(), []
    for b, _ in named:
        t, o = b.torrents[0], b.offs[0]
        nums = [t.n, t.P, t.threshold, t.flags] + M.Batch.rows(b.arrays["bits"], t, o).view("i8").reshape(-1).tolist()
        nums += b.live[o["l"]:o["l"] + (t.P + 63) // 64].view("i8").tolist() + [len(t.joins)]  # as signed: scanf reads long long
        for p, span in t.joins:
            nums += [p, len(span), *span]
        lines.append(" ".join(str(int(x)) for x in nums + [len(t.fulls)] + t.fulls))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(named)
    for (b, _), line in zip(named, out):
        t, o, w = b.torrents[0], b.offs[0], b.want()
        per_slot = zip(*(w[name][o["p"]:o["p"] + t.P].tolist() for name in ("held", "wanted", "status")))
        want = [int(w["remaining"][0]), int(w["tflags"][0])] + [x for slot in per_slot for x in slot]
        assert [int(x) for x in line.split()] == want + M.Batch.rows(w["bits"], t, o).reshape(-1).tolist(), b.label
