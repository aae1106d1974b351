"""tests/native/repiece_math_main.cpp: the re-piece arithmetic (kraken_amd/csrc/repiece_math.hpp,
what krk_repiece_sums, krk_repiece_batch and piece_repiece.hip run) as a stand-alone CPU program
(its own main, nothing of the library linked) built with AddressSanitizer and
UndefinedBehaviorSanitizer and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_repiece_math_under_asan_ubsan(tmp_path):
    src = os.path.join(ROOT, "tests", "native", "repiece_math_main.cpp")
    exe = str(tmp_path / "repiece_math_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
