"""GPU parity: the connection kernels (conn_round.hip) at their word, step and
one-register-a-lane edges through krk_conn_round_dev and krk_conn_preempt_dev -- the rows, the
expiries, the capacities and every output against tests/conn_ref.py's restatement, against
tests/golden/conn_rounds.json and, bit for bit, against the host forms (the cases and the comparison
live in tests/conn_matrix.py; tests/test_conn_matrix_cpu.py proves them on the host forms).  Every
buffer is prefilled with a poison value and every region is fenced by canaries, so a case passes
only when every owned element is stored and nothing else is touched."""
import numpy as np
import pytest

from tests import conn_matrix as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device(gpu):
    return M.DeviceBackend()


@pytest.mark.parametrize("p", M.PS)
def test_matrix_in_device_memory(device, p):
    """Six torrents a P, the three lists cycling through the lengths 0, 1, 63, 64, 65 and 129."""
    assert M.compare(M.case(f"matrix P={p}"), device.run(M.case(f"matrix P={p}"))) == []


def test_named_cases(device):
    some = M.named()
    calls, bad = M.run_cases(device, some)
    assert calls == len(some) >= 30 and bad == [], bad[:5]


def test_outputs_in_page_locked_memory(device):
    some = [M.case("matrix P=65"), M.case("matrix P=4097")] + M.named()[::3]
    calls, bad = M.run_cases(device, some, pinned=True)
    assert calls == len(some) and bad == [], bad[:5]


def test_device_equals_the_host_form_bit_for_bit(device):
    host = M.HostBackend()
    for c in M.cases():
        g, h = device.run(c), host.run(c)
        assert all(np.array_equal(x, y) for x, y in zip(g, h)), c.label
    for c in M.sweeps():
        g, h = device.sweep(c), host.sweep(c)
        assert all(np.array_equal(x, y) for x, y in zip(g, h)), c.label


def test_device_equals_the_golden_file(device):
    gold = M.golden()
    for c in M.cases():
        assert M.entry_of(c, device.run(c)) == gold[c.label], c.label
    for c in M.sweeps():
        assert M.sweep_entry(c, device.sweep(c)) == gold[c.label], c.label


def test_sweeps(device):
    some = M.sweeps()
    calls, bad = M.run_sweeps(device, some)
    assert calls == len(some) and bad == [], bad[:5]
    assert M.sweeps()[0].closed() == [1, 3, 5, 7, 10]
