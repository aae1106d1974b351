"""krk_receive_round (receive_round_math.hpp on the host) over tests/receive_round_cases.py, against
tests/receive_round_ref.py: whole prefilled buffers, the rows, received and the twelve outputs."""
import pytest

from tests import receive_round_cases as M


@pytest.mark.parametrize("label", list(M.cases()))
def test_case_equals_the_reference(label):
    assert not M.check_case(M.cases()[label], dev=False)


def test_hand_worked_vector():
    assert not M.hand(False)


def test_refusals_touch_nothing():
    assert not M.refusals(dev=False)
