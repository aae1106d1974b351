"""tests/native/window_math_main.cpp: the two schedules and the per-thread span cutting of the host-resident window
passes (kraken_amd/csrc/window_math.hpp: WindowSched and PackSched, what window_pass.cpp runs every window by, and
cut_span, what par_copy and par_read of staging.hpp split a window's fill with) as a stand-alone CPU program (its own main, nothing
of the library linked) built with AddressSanitizer and UndefinedBehaviorSanitizer and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_math_under_asan_ubsan(tmp_path):
    src = os.path.join(ROOT, "tests", "native", "window_math_main.cpp")
    exe = str(tmp_path / "window_math_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
