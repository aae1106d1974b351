"""krk_serve_round_dev (serve_round.hip) over tests/serve_round_cases.py, against
tests/serve_round_ref.py: whole prefilled buffers, the rows, sent and the ten outputs, in device
memory and once with the outputs in page-locked host memory."""
import pytest

from tests import serve_round_cases as M

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("label", list(M.cases()))
def test_case_equals_the_reference(gpu, label):
    assert not M.check_case(*M.cases()[label], dev=True)


def test_outputs_in_page_locked_memory(gpu):
    assert not M.check_case(*M.cases()[f"n_reqs={2 * M.CHUNK + 1}"], dev=True, pinned=True)


def test_hand_worked_vector(gpu):
    assert not M.hand(True)


def test_refusals_touch_nothing(gpu):
    assert not M.refusals(dev=True)
