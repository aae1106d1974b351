"""The serve round through the public classes: a 65-piece torrent's RequestTable answers queued
piece requests, the served bits count in the next Reserve's request round, and LastPieceSent feeds
PreemptionSweep's idle rule; host placement against values worked out by hand, "gpu" (marked gpu)
equal to the host."""
import numpy as np
import pytest

from kraken_amd import connstate as CS
from kraken_amd import device as D
from kraken_amd import piecerequest as PR

N, P = 65, 64  # the last piece has 54 bytes


def drive(placement):
    clk = PR.MockClock(100)
    d = PR.Dispatcher(N, PR.NewManager(clk, 10, PR.RarestFirstPolicy, 1))
    d.length, d.piece_length = N * P - 10, P
    d.have[[0, 63, 64]] = True
    for peerID, held in (("A", ()), ("B", (5,)), ("C", ())):
        d.AddPeer(peerID, [i in held for i in range(N)])
    tbl = PR.RequestTable([d], placement)
    for q in (("A", 0, 0, 64), ("B", 64, 0, 54), ("A", 64, 0, 64), ("A", 1, 0, 64), ("B", 65, 0, 0), ("C", 63, 0, 64)):
        tbl.Requested(0, *q)
    tbl.RemovePeer(0, "C")
    first, picks = tbl.Serve(token_size=100), tbl.Reserve()
    if placement == "gpu":  # the counts of a request round on the resident rows
        counts = D.piece_request_round_dev(tbl.batch, tbl.bits, tbl.out.quota, tbl.limit, counts=True)[0]
    else:
        counts = D.piece_request_round(tbl.batch, tbl.bits, np.zeros(3, np.int32), tbl.limit, counts=True)[0]
    clk.Add(50)
    tbl.Requested(0, "A", 63, 0, 64)
    second = tbl.Serve()
    s = CS.State(CS.Config(), clk, "local")
    for peerID in "AB":
        assert s.AddPending(peerID, "h") is None and s.MovePendingToActive(CS.Conn(peerID, "h", createdAt=90)) is None
    clk.Add(20)  # now 170, tti 60: both conns are idle but for what they were sent
    sweeps = [[c.PeerID() for c in CS.PreemptionSweep(s, 60, 10_000, None, sent, placement)]
              for sent in (lambda h, p: tbl.LastPieceSent(0, p), None)]
    last = [tbl.LastPieceSent(0, p) for p in "AB"]
    tbl.Requested(0, "B", 0, 0, 64)  # B leaves, a table round frees its slot, E takes it: B's request has no peer
    tbl.RemovePeer(0, "B")
    tbl.Reserve()
    tbl.AddPeer(0, "E", PR.marshal_bitfield(np.zeros(N, bool)))
    late = (tbl.LastPieceSent(0, "E"), tbl.Serve()[0]["gone"], tbl.LastPieceSent(0, "E"))  # B's 100 is not E's
    return first, picks, np.flatnonzero(counts).tolist(), second, last, sweeps, late


def check(got):
    assert got == ([{"sends": [("A", 0, 0, 64, 0), ("B", 64, 4096, 54, 64)],
                     "refusals": [("A", 64, "reading / writing chunk of piece not supported"), ("A", 1, "piece not complete"),
                                  ("B", 65, "invalid piece index 65: num pieces = 65")],
                     "gone": [("C", 63)], "bytes": 118, "tokens": 5 + 4}],
                   [{"A": [], "B": [5]}], [0, 5, 64],
                   [{"sends": [("A", 63, 63 * 64, 64, 0)], "refusals": [], "gone": [], "bytes": 64, "tokens": 0}],
                   [150, 100], [["B"], ["A", "B"]], (0, [("B", 0)], 0))


def test_host_drive():
    check(drive("host"))
    d = PR.Dispatcher(N, PR.NewManager(PR.MockClock(), 10, PR.RarestFirstPolicy, 1))
    d.AddPeer("A", np.zeros(N, bool))
    tbl = PR.RequestTable([d])
    tbl.Requested(0, "A", 0, 0, 64)
    with pytest.raises(ValueError):  # no length / piece_length on the dispatcher
        tbl.Serve()


@pytest.mark.gpu
def test_gpu_drive_equals_the_host_drive(gpu):
    got = drive("gpu")
    check(got)
    assert got == drive("host")
