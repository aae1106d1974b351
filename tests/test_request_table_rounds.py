"""piecerequest.RequestTable against ReserveRound / ResendRound over Manager: the drive of
tests/test_gpu_piece_resend_round.py (1,000, 65 and 1 piece, five peers, one dead peer, the clock
stepped past the timeout, both policies, endgame on and off) run through the resident tables must
equal the Manager's drive round for round.  The drive removes no peer; the one deliberate
difference, ClearPeer, is pinned against tests/request_table_ref.py on its own.  Placement "host"
runs without a GPU; "gpu" is marked gpu."""
import numpy as np
import pytest

from kraken_amd import device as D
from kraken_amd import piecerequest as PR
from tests import request_table_ref as R
from tests.test_gpu_piece_resend_round import DEAD, EVERY, TIMEOUT, dispatchers, drive

POLICIES = [PR.RarestFirstPolicy, PR.DefaultPolicy]


def table_drive(placement, policy, disable_endgame):
    ds = dispatchers(policy, disable_endgame)
    tbl = PR.RequestTable(ds, placement=placement)
    rounds = []
    for k in range(2000):
        if all(h.all() for h in tbl.have):
            break
        got = tbl.Reserve()
        rounds.append(("reserve", got))
        for t, g in enumerate(got):
            tbl.Arrived(t, [i for peerID, pieces in g.items() if peerID != DEAD for i in pieces])
        if k % EVERY == EVERY - 1:
            for d in ds:
                d.manager.clock.Add(TIMEOUT + 1)
        again = tbl.Resend()
        rounds.append(("resend", [[(r.Piece, r.PeerID, r.Status, t) for r, t in g] for g in again]))
        for t, g in enumerate(again):
            tbl.Arrived(t, [r.Piece for r, target in g if target is not None and target != DEAD])
    assert all(h.all() for h in tbl.have)
    return rounds


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("disable_endgame", [True, False])
def test_host_table_drive_equals_the_manager_drive(policy, disable_endgame):
    assert table_drive("host", policy, disable_endgame) == drive("host", policy, disable_endgame)


@pytest.mark.gpu
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("disable_endgame", [True, False])
def test_gpu_table_drive_equals_the_manager_drive(gpu, policy, disable_endgame):
    assert table_drive("gpu", policy, disable_endgame) == drive("host", policy, disable_endgame)


def test_gone_drops_every_entry_where_clear_peer_leaves_one():
    """Peer 0 holds two requests for piece 5: the reference's ClearPeer ejects the first only, the
    table round drops both (and the reference file says the same of the round)."""
    assert R.clear_peer_reference({5: [(0,), (1,), (0,)]}, 0) == {5: [(0,), (1,)]}
    batch = D.RequestBatch([65], [2])
    table = D.TableBatch(batch, 8).events(gone={0: [0]})
    bits, entries = np.zeros(batch.total_words, np.uint64), np.zeros(8, D.RT_ENTRY)
    entries[:3] = [(5, 0, 0, 0, 0), (5, 1, 0, 0, 0), (5, 0, 0, 0, 0)]
    n_entries = np.array([3], np.uint32)
    quota, _, _, _ = D.request_table_round(batch, table, bits, entries, n_entries, 0, 10, 3)
    want = R.round_torrent(65, 2, 0, (), [(), ()], [(5, 0, 0, 0), (5, 1, 0, 0), (5, 0, 0, 0)], 8, gone=[0], timeout=10, limit=3)
    assert n_entries[0] == 1 and entries[0].tolist() == (5, 1, 0, 0, 0) and quota.tolist() == want[4] == [3, 2]
    assert want[2] == [(5, 1, 0, 0)]
