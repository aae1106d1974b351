"""krk_peer_round (peer_round_math.hpp on the calling thread) over tests/peer_round_cases.py: against
tests/peer_round_ref.py, whole prefilled buffers, the rows and the five outputs.  No device."""
import pytest

from kraken_amd import piecerequest as PR
from tests import peer_round_cases as M


def test_marshal_bitfield_is_the_hand_worked_vector():
    assert PR.marshal_bitfield([i in (0, 9) for i in range(10)]) == M.HAND


def test_matrix_equals_the_reference():
    bad = [m for b in M.matrix() for m in M.mismatches(b, *M.run(b))]
    assert not bad, bad[:10]


@pytest.mark.parametrize("k", [0, 1, 3, 70])
def test_batches(k):
    b = M.batch(k)
    assert not M.mismatches(b, *M.run(b))


def test_named_cases_by_hand():
    for b, hand in M.named():
        rc, got = M.run(b)
        bad = M.mismatches(b, rc, got) + M.hand_mismatches(b, got, hand)
        assert not bad, bad


def test_refusals_touch_nothing():
    assert not M.refusals()
