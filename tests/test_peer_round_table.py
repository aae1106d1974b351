"""piecerequest.RequestTable with a peer set that changes where the rows lie: one drive at 65 pieces.
Three peers start, three more join by AddPeer in later rounds, one is removed and its slot reused two
rounds on, one join is malformed, one peer sends Complete, and pieces arrive until the torrent
completes.  Placement "host" runs without a GPU and is held against what the test knows of the
peers; "gpu" is marked gpu and must equal the host drive round for round, picks and Progress()."""
import numpy as np
import pytest

from kraken_amd import piecerequest as PR

N, TIMEOUT = 65, 10


def drive(placement):
    rng = np.random.default_rng(20261126)
    field = lambda: rng.random(N) < 0.7  # noqa: E731
    d = PR.Dispatcher(N, PR.NewManager(PR.MockClock(), TIMEOUT, PR.RarestFirstPolicy, 1), endgame_threshold=4)
    for peerID in "ABC":
        d.AddPeer(peerID, field())
    tbl = PR.RequestTable([d], placement, spare_peers=3)
    log = []
    for k in range(100):
        if k == 1:
            tbl.AddPeer(0, "D", PR.marshal_bitfield(np.ones(N, bool)))
        if k == 2:
            tbl.RemovePeer(0, "B")
            with pytest.raises(ValueError, match="peer already exists"):
                tbl.AddPeer(0, "D", b"")
        if k == 3:
            tbl.AddPeer(0, "X", PR.marshal_bitfield(np.ones(N + 1, bool)))  # a bitfield of another torrent: refused
        if k == 4:
            for peerID in "EFG":
                tbl.AddPeer(0, peerID, PR.marshal_bitfield(field()))
            assert tbl.index[0]["E"] == 1  # B's slot, two rounds after the removal
            with pytest.raises(ValueError, match="no free peer slot"):
                tbl.AddPeer(0, "H", b"")
            tbl.RemovePeer(0, "G")  # never joined: free at once
        if k == 5:
            tbl.PeerComplete(0, "A")
        got = tbl.Reserve()
        tbl.Arrived(0, [i for pieces in got[0].values() for i in pieces])
        again = tbl.Resend()
        prog = tbl.Progress()[0]
        assert prog["endgame"] == tbl.endgame(0) and prog["remaining"] == N - int(tbl.have[0].sum())
        log.append((got, [[(r.Piece, r.PeerID, r.Status, t) for r, t in g] for g in again], prog))
        if prog["complete"]:
            break
    return log


def check(log):
    progs = [p for _, _, p in log]
    assert progs[-1]["complete"] and len(log) > 6
    assert [p["refused"] for p in progs[:5]] == [[], [], [], ["X"], []]
    assert [sorted(g[0]) for g, _, _ in log[:6]] == [list(x) for x in ("ABC", "ABCD", "ACD", "ACD", "ACDEF", "ACDEF")]
    assert progs[1]["held"]["D"] == N and progs[4]["held"]["A"] < N and progs[5]["held"]["A"] == N
    # complete() closes the peers that hold everything and sends Complete to the others
    assert sorted(progs[-1]["close"]) == ["A", "D"] and sorted(progs[-1]["notify"]) == ["C", "E", "F"]
    assert all(not p["close"] and not p["notify"] for p in progs[:-1])


def test_host_drive():
    check(drive("host"))


@pytest.mark.gpu
def test_gpu_drive_equals_the_host_drive(gpu):
    log = drive("gpu")
    check(log)
    assert log == drive("host")
