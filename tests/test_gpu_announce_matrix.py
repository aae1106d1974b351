"""GPU parity: the announce kernels (announce_round.hip) at their word, lane-stride, window and
limit edges through krk_announce_round_dev -- the updated bits, handout, n_out and the label counts
against tests/announce_ref.py's restatement, against tests/golden/announce_rounds.json and, bit for
bit, against the host form krk_announce_round (the cases and the comparison live in
tests/announce_matrix.py; tests/test_announce_matrix_cpu.py proves them on the host forms).  Every
buffer is prefilled with a poison value, so a case passes only when every owned element is stored
and nothing else is touched."""
import numpy as np
import pytest

from tests import announce_matrix as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device(gpu):
    return M.DeviceBackend()


@pytest.mark.parametrize("p", M.PS)
def test_matrix_in_device_memory(device, p):
    """P x limit x W, cur_row, O and the policy cycling: one P a test."""
    some = [c for c in M.cases() if c.label.startswith(f"matrix P={p} ")]
    calls, bad = M.run_cases(device, some)
    assert calls == len(M.LIMITS) * len(M.WS) and bad == [], f"{len(bad)} mismatches of {calls} calls, first {bad[:5]}"


def test_named_cases(device):
    some = M.named()
    calls, bad = M.run_cases(device, some)
    assert calls == len(some) and bad == [], bad[:5]


@pytest.mark.parametrize("label", ["A=1 over three torrents", "A=257 over three torrents"])
def test_batches(device, label):
    assert M.compare(M.case(label), device.run(M.case(label))) == []


def test_outputs_in_page_locked_memory(device):
    some = [M.case("A=257 over three torrents"), M.case("all ones, more than one stride of words")] + M.cases()[:45:7]
    calls, bad = M.run_cases(device, some, pinned=True)
    assert calls == len(some) and bad == [], bad[:5]


def test_device_equals_the_host_form_bit_for_bit(device):
    host = M.HostBackend()
    for c in M.cases():
        g, h = device.run(c), host.run(c)
        assert all(np.array_equal(x, y) for x, y in zip(g, h)), c.label


def test_device_equals_the_golden_file(device):
    gold = M.golden()
    for c in M.cases()[::4] + M.named():
        assert M.got_entry(c, device.run(c)) == gold[c.label], c.label
