"""tests/native/direct_read_main.cpp: direct_pread of kraken_amd/csrc/direct_read.hpp -- the O_DIRECT read of a window
request, its bounce loop, the process-wide switch and the diag build's simulated refusal -- as a stand-alone CPU
program (its own main, nothing of the library linked), built plain and with AddressSanitizer and
UndefinedBehaviorSanitizer and run directly.  Its files go under the repository's build tree, where O_DIRECT usually
opens (a tmpfs refuses it); where it does not, the program says so (exit status 77) and the tests skip."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "build", "native")


@pytest.fixture(scope="module")
def programs():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "native"), "direct_read"])
    return {"plain": os.path.join(OUT, "direct_read"), "san": os.path.join(OUT, "direct_read_san")}


def _run(exe, name, *args, env=None):
    d = os.path.join(ROOT, "build", "direct_read_files", name)
    os.makedirs(d, exist_ok=True)
    try:
        r = subprocess.run([exe, d, *args], capture_output=True, text=True, timeout=300, env=env)
    finally:
        for f in os.listdir(d):
            os.unlink(os.path.join(d, f))
    if r.returncode == 77:
        pytest.skip("no filesystem here accepts O_DIRECT (" + r.stdout.strip() + ")")
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


@pytest.mark.parametrize("build", ["plain", "san"])
def test_direct_pread_matches_buffered_reads(programs, build):
    """Request sizes around the 1 MiB bounce buffer at three file offsets, files that end inside the request, a
    request at EOF, bad descriptors, the switch off, and four threads each with its own bounce buffer."""
    _run(programs[build], "all_" + build)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("build", ["plain", "san"])
def test_simulated_refusal_flips_the_switch_at_read_n(programs, build, n):
    """KRK_DIRECT_REFUSE=N: reads before the N-th go straight in, the N-th flips the switch and returns the right
    bytes through the bounce buffer, and the switch stays on."""
    _run(programs[build], "seam%d_%s" % (n, build), "seam", env=dict(os.environ, KRK_DIRECT_REFUSE=str(n)))
