"""The receive round through the public classes: a 65-piece torrent's RequestTable reserves a piece
a peer, judges the queued payloads, and the next Resend and Reserve see the verdicts -- the arrived
piece is picked no more, the bad-sum and chunk pairs are failed requests -- and
LastGoodPieceReceived feeds PreemptionSweep's idle rule; host placement against values worked out
by hand, "gpu" (marked gpu) equal to the host."""
import numpy as np
import pytest

from kraken_amd import connstate as CS
from kraken_amd import piecerequest as PR

N, P = 65, 64  # the last piece has 54 bytes


def drive(placement):
    clk = PR.MockClock(100)
    d = PR.Dispatcher(N, PR.NewManager(clk, 1000, PR.RarestFirstPolicy, 1))
    d.length, d.piece_length, d.piece_sums = N * P - 10, P, 500 + np.arange(N)
    d.have[0] = True
    for peerID, held in (("A", (1, 2)), ("B", (2, 3)), ("C", (4,))):  # rarest first: A takes 1, B 3, C 4
        d.AddPeer(peerID, [i in held for i in range(N)])
    tbl = PR.RequestTable([d], placement, spare_peers=1)
    picks = tbl.Reserve()
    clk.Add(50)
    for q in (("A", 1, 0, 64, 501), ("B", 3, 0, 64, 999), ("C", 4, 0, 63, 504), ("A", 0, 0, 64, 500), ("B", 65, 0, 0, 0)):
        tbl.Received(0, *q)
    first = tbl.Receive()
    failed = [r for r, _ in tbl.Resend()[0]]
    again = tbl.Reserve()
    s = CS.State(CS.Config(), clk, "local")
    for peerID in "AB":
        assert s.AddPending(peerID, "h") is None and s.MovePendingToActive(CS.Conn(peerID, "h", createdAt=90)) is None
    clk.Add(20)  # now 170, tti 60: both conns are idle but for what they received
    sweeps = [[c.PeerID() for c in CS.PreemptionSweep(s, 60, 10_000, good, None, placement)]
              for good in (lambda h, p: tbl.LastGoodPieceReceived(0, p), None)]
    last = [tbl.LastGoodPieceReceived(0, p) for p in "AB"]
    tbl.Received(0, "A", 2, 0, 64)  # A leaves, a table round frees its slot, E takes it: the piece is nobody's
    tbl.RemovePeer(0, "A")
    tbl.Reserve()
    tbl.AddPeer(0, "E", PR.marshal_bitfield(np.zeros(N, bool)))
    sums = np.array([502], dtype=np.uint32)
    if placement == "gpu":
        host, sums = sums, PR.D.DeviceBuffer(4)
        sums.from_host(host)
    late = (tbl.LastGoodPieceReceived(0, "E"), tbl.Receive(sums)[0], tbl.LastGoodPieceReceived(0, "E"), tbl.have[0][:4].tolist())
    return picks, first, failed, again, last, sweeps, late


def check(got):
    picks, first, failed, again, last, sweeps, late = got
    assert picks == [{"A": [1], "B": [3], "C": [4]}]
    assert first == [{"writes": [("A", 1, 64)], "duplicates": [("A", 0)],
                      "invalid": [("B", 3, "invalid piece sum"), ("C", 4, "reading / writing chunk of piece not supported"),
                                  ("B", 65, "invalid piece index 65: num pieces = 65")],
                      "announce": [(1, "A")], "complete": False, "completed_now": False, "bytes": 128}]
    assert failed == [PR.Request(3, "B", PR.StatusInvalid), PR.Request(4, "C", PR.StatusInvalid)]
    assert again[0]["A"] == [2] and not any(1 in v for v in again[0].values())
    assert (last, sweeps) == ([150, 0], [["B"], ["A", "B"]])
    assert late == (0, {"writes": [(None, 2, 128)], "duplicates": [], "invalid": [], "announce": [(2, None)], "complete": False,
                        "completed_now": False, "bytes": 192}, 0, [True, True, True, False])


def test_host_drive():
    check(drive("host"))
    d = PR.Dispatcher(N, PR.NewManager(PR.MockClock(), 10, PR.RarestFirstPolicy, 1))
    d.AddPeer("A", np.zeros(N, bool))
    d.length, d.piece_length = N * P, P
    tbl = PR.RequestTable([d])
    tbl.Received(0, "A", 0, 0, 64, 1)
    with pytest.raises(ValueError):  # no piece_sums on the dispatcher
        tbl.Receive()


@pytest.mark.gpu
def test_gpu_drive_equals_the_host_drive(gpu):
    got = drive("gpu")
    check(got)
    assert got == drive("host")
