"""krk_request_table_round, the host form of the request table round, over tests/request_table_matrix.py
against tests/request_table_ref.py: whole prefilled buffers, state and outputs.  No device."""
import pytest

from kraken_amd import _capi
from tests import request_table_matrix as M

HOST = M.Backend()


def test_matrix():
    bad = M.run_cases(HOST, M.cases())
    assert not bad, bad[:10]


@pytest.mark.parametrize("k", [0, 1, 3, 70])
def test_batches(k):
    bad = M.run_cases(HOST, [M.batch(k)])
    assert not bad, bad[:10]


def test_named_cases_by_hand():
    for b, hand in M.named():
        rc, got = HOST.run(b)
        bad = M.compare(b, got) + M.hand_mismatches(b, got, hand)
        assert rc == 0 and not bad, bad


def test_refusals_touch_nothing():
    bad = M.check_refusals(HOST)
    assert not bad, bad
    b = M.count_above_cap()  # the host form reads n_entries: a count above cap is refused
    rc, got = HOST.run(b)
    assert rc == _capi.KRK_EINVAL and not M.compare(b, got, want=b.arrays)
