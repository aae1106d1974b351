"""tests/native/conn_round_main.cpp: the connection round's host arithmetic
(kraken_amd/csrc/conn_math.hpp, what krk_conn_round and krk_conn_preempt run and conn_round.hip
equals) as a stand-alone CPU program (its own main, nothing of the library linked) built with
AddressSanitizer and UndefinedBehaviorSanitizer and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_conn_math_under_asan_ubsan(tmp_path):
    src = os.path.join(ROOT, "tests", "native", "conn_round_main.cpp")
    exe = str(tmp_path / "conn_round_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
