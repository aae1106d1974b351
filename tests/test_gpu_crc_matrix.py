"""GPU parity: the CRC-32 piece kernel (crc32_pieces.hip) at its lane, step, item and run
edges, bit-exact against zlib (the cases and the comparison live in tests/crc_matrix.py):

1. every group in process on the production library, which must run launch variant 16;
2. the whole matrix again under every other bit-exact launch variant -- the production
   alternatives 7, 8, 14, 15, 17 and the diag build's layouts -- one fresh child a variant
   (KRK_CRC_VARIANT is read once per device context, and only by the diag build).  Variants 4,
   10, 11 and 13 are load-only timing kernels with wrong sums by design and stay out."""
import json
import os
import subprocess
import sys

import pytest

from tests import crc_matrix as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = [7, 8, 14, 15, 17, 0, 1, 2, 3, 5, 6, 9, 12, 20, 21, 22, 23]
# A child measured 0.6 - 0.8 s: interpreter, library and device start-up plus 0.25 s of matrix
# (tests/crc_matrix.py prints each group's seconds).  The limit leaves room for a loaded machine.
CHILD_TIMEOUT_S = 30

_died = []  # the variant whose child ended by a signal or at its timeout: no further child starts


@pytest.fixture(scope="module")
def device(gpu):
    b = M.DeviceBackend()
    yield b
    b.close()


@pytest.mark.parametrize("group", M.GROUPS)
def test_crc_matrix_group(device, group):
    assert device.variant() == 16, "the production library runs launch variant 16"
    n, bad = M.run_group_counted(group, device)
    assert n > 0
    assert bad == [], f"group {group}: {len(bad)} of {n} cases differ from zlib, first {bad[:5]}"


@pytest.mark.parametrize("v", VARIANTS)
def test_crc_matrix_variant(gpu, v):
    from tests.conftest import diag_lib
    assert not _died, f"the child of variant {_died[0]} ended by a signal or at its timeout: no further child is started"
    env = dict(os.environ, KRK_LIB_PATH=diag_lib(), KRK_CRC_VARIANT=str(v))
    try:
        r = subprocess.run([sys.executable, "-m", "tests.crc_matrix"], capture_output=True, text=True, cwd=ROOT,
                           env=env, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired as e:
        _died.append(v)
        pytest.fail(f"variant {v}: the child did not end within {CHILD_TIMEOUT_S} s; output so far: {e.stdout!r}")
    if r.returncode < 0:
        _died.append(v)
        pytest.fail(f"variant {v}: the child ended by signal {-r.returncode}: {r.stdout[-2000:]} {r.stderr[-2000:]}")
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert [x["group"] for x in lines] == list(M.GROUPS), r.stdout[-2000:] + r.stderr[-2000:]
    assert [x["variant"] for x in lines] == [v] * len(lines), "the child ran another launch variant"
    bad = [(x["group"], x["n_mismatches"], x["mismatches"][:3]) for x in lines if x["n_mismatches"]]
    assert bad == [] and r.returncode == 0, f"variant {v}: {bad} {r.stderr[-2000:]}"
