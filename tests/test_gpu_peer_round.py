"""krk_peer_round_dev (peer_round.hip) over tests/peer_round_cases.py: against tests/peer_round_ref.py
and, byte for byte, against the host form; whole prefilled buffers, the rows and the five outputs,
in device memory and once with the outputs and the wire in page-locked host memory."""
import pytest

from tests import peer_round_cases as M

pytestmark = pytest.mark.gpu


def both(b, pinned=False):
    """Mismatches of the device form against the reference and against the host form."""
    rc, got = M.run(b, dev=True, pinned=pinned)
    return M.mismatches(b, rc, got) + M.mismatches(b, rc, got, want=M.run(b)[1])


def test_matrix_equals_the_reference_and_the_host_form(gpu):
    bad = [m for b in M.matrix() for m in both(b)]
    assert not bad, bad[:10]


@pytest.mark.parametrize("k,pinned", [(0, False), (1, False), (3, False), (70, False), (70, True)])
def test_batches(gpu, k, pinned):
    assert not both(M.batch(k), pinned)


def test_named_cases_by_hand(gpu):
    for b, hand in M.named():
        rc, got = M.run(b, dev=True)
        bad = both(b) + M.hand_mismatches(b, got, hand)
        assert not bad, bad


def test_refusals_touch_nothing(gpu):
    assert not M.refusals(dev=True)
