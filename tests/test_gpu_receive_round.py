"""krk_receive_round_dev (receive_round.hip) over tests/receive_round_cases.py, against
tests/receive_round_ref.py: whole prefilled buffers, the rows, received and the twelve outputs, in
device memory and once with the outputs in page-locked host memory."""
import pytest

from tests import receive_round_cases as M

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("label", list(M.cases()))
def test_case_equals_the_reference(gpu, label):
    assert not M.check_case(M.cases()[label], dev=True)


def test_outputs_in_page_locked_memory(gpu):
    assert not M.check_case(M.cases()[f"n_pays={2 * M.CHUNK + 1}"], dev=True, pinned=True)


def test_hand_worked_vector(gpu):
    assert not M.hand(True)


def test_refusals_touch_nothing(gpu):
    assert not M.refusals(dev=True)
