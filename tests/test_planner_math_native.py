"""tests/native/planner_math_main.cpp: the placement planners' arithmetic
(kraken_amd/csrc/planner_math.hpp: offload_plan, tail_plan, digester_crossover, what every default
placement of the library is decided by) as a stand-alone CPU program (its own main, nothing of the
library linked) built with AddressSanitizer and UndefinedBehaviorSanitizer and run directly.
float-cast-overflow is named as well: g++ leaves it out of -fsanitize=undefined, and the planners
turn quotients of injected rates into integers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planner_math_under_asan_ubsan(tmp_path):
    src = os.path.join(ROOT, "tests", "native", "planner_math_main.cpp")
    exe = str(tmp_path / "planner_math_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
