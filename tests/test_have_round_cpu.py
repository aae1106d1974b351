"""krk_have_round (have_round_math.hpp on the host) over tests/have_round_cases.py, against
tests/have_round_ref.py: whole prefilled buffers, the rows and the nine outputs."""
import pytest

from tests import have_round_cases as M


@pytest.mark.parametrize("label", list(M.cases()))
def test_case_equals_the_reference(label):
    assert not M.check_case(*M.cases()[label][:1], False, M.cases()[label][1])


def test_hand_worked_vector():
    assert not M.hand(False)


def test_round_trips():
    assert not M.round_trips(False)


def test_refusals_touch_nothing():
    assert not M.refusals()
