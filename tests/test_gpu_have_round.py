"""krk_have_round_dev (have_round.hip) over tests/have_round_cases.py, against
tests/have_round_ref.py: whole prefilled buffers, the rows and the nine outputs, in device memory
and once with the outputs in page-locked host memory."""
import pytest

from tests import have_round_cases as M

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("label", list(M.cases()))
def test_case_equals_the_reference(gpu, label):
    ts, skew = M.cases()[label]
    assert not M.check_case(ts, True, skew)


def test_outputs_in_page_locked_memory(gpu):
    ts, skew = M.cases()["n=65"]
    assert not M.check_case(ts, True, skew, pinned=True)


def test_hand_worked_vector(gpu):
    assert not M.hand(True)


def test_round_trips(gpu):
    assert not M.round_trips(True)


def test_refusals_touch_nothing(gpu):
    assert not M.refusals(dev=True)
