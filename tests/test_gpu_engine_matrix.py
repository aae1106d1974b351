"""GPU parity: the submission engine (engine.cpp, digester.cpp, piece_stream.cpp) at its slot, block and piece edges, bit-exact
against hashlib and zlib (the plans, the references and the runner live in tests/engine_matrix.py):

1. groups A to D in process on KRK_PLACE_GPU -- Digester tails, splits around the slot and sums at
   every pending state; piece streams at piece lengths in a structural relation to the slot and the
   CRC item; crc32_update around Q requests in flight; one coalesced crowd of all three;
2. group E, the pend-buffer path, in one fresh child whose first engine call puts the slot pool at
   its minimum cap (tests/engine_matrix.py says why that forces the path)."""
import json
import os
import subprocess
import sys

import pytest

from kraken_amd._capi import KRK_PLACE_GPU
from tests import engine_matrix as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The child moves 68 MiB through 16 slots, two requests an owner in flight; interpreter, library and
# device start-up are most of its time.  The limit leaves room for a loaded machine.
CHILD_TIMEOUT_S = 120


@pytest.mark.parametrize("group", M.GROUPS)
def test_engine_matrix_group(gpu, group):
    n, nbytes, seconds, bad = M.run_group_counted(group, KRK_PLACE_GPU)
    print(f"group {group}: {n} cases, {nbytes} bytes, {seconds:.3f} s")
    assert n > 0
    assert bad == [], f"group {group}: {len(bad)} mismatches in {n} cases, first {bad[:5]}"


def test_engine_matrix_pend_buffer_path(gpu):
    r = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, "-m", "tests.engine_matrix",
                        "--pend"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode in (0, 1), f"the child ended with {r.returncode}: {r.stdout[-2000:]} {r.stderr[-2000:]}"
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:] + r.stderr[-2000:]
    rec = lines[0]
    print(rec)
    assert rec["group"] == "E" and rec["cases"] == len(M.plans_e())
    # one 16-slot chunk: no digester could hold a slot between calls
    assert rec["cap"] == 16 * M.S and 0 < rec["pinned"] <= rec["cap"]
    assert rec["n_mismatches"] == 0 and r.returncode == 0, rec["mismatches"][:5]
