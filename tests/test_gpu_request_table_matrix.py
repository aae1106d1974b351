"""krk_request_table_round_dev (request_table.hip) over tests/request_table_matrix.py: against the host
form and against tests/request_table_ref.py, whole prefilled buffers, state and outputs, in device
memory and in page-locked host memory."""
import pytest

from tests import request_table_matrix as M

pytestmark = pytest.mark.gpu


def test_matrix_equals_the_reference_and_the_host_form(gpu):
    dev, host = M.Backend(dev=True), M.Backend()
    bad = M.run_cases(dev, M.cases())
    for b in M.cases()[::7]:  # the two forms byte for byte, the entries past the count included
        (_, d), (_, h) = dev.run(b), host.run(b)
        bad += M.compare(b, d, want=h)
    assert not bad, bad[:10]


@pytest.mark.parametrize("k", [0, 1, 3, 70])
@pytest.mark.parametrize("pinned", [False, True])
def test_batches(gpu, k, pinned):
    bad = M.run_cases(M.Backend(dev=True, pinned=pinned), [M.batch(k)])
    assert not bad, bad[:10]


def test_named_cases_by_hand(gpu):
    for b, hand in M.named():
        rc, got = M.Backend(dev=True).run(b)
        bad = M.compare(b, got) + M.hand_mismatches(b, got, hand)
        assert rc == 0 and not bad, bad


def test_refusals_touch_nothing_and_a_count_above_cap_is_read_as_cap(gpu):
    bad = M.check_refusals(M.Backend(dev=True))
    assert not bad, bad
    b = M.count_above_cap()
    rc, got = M.Backend(dev=True).run(b)
    assert rc == 0 and not M.compare(b, got), M.compare(b, got)
