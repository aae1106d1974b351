"""krk_serve_round (serve_round_math.hpp on the host) over tests/serve_round_cases.py, against
tests/serve_round_ref.py: whole prefilled buffers, the rows, sent and the ten outputs."""
import pytest

from tests import serve_round_cases as M


@pytest.mark.parametrize("label", list(M.cases()))
def test_case_equals_the_reference(label):
    assert not M.check_case(*M.cases()[label], dev=False)


def test_hand_worked_vector():
    assert not M.hand(False)


def test_refusals_touch_nothing():
    assert not M.refusals(dev=False)
