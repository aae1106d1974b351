"""The have round through the public classes: a 65-piece agentstorage.Torrent reopened with
restore=True, its sidecar into a RequestTable, a recheck that drops one piece, a verify that adds
two; host placement against tests/have_round_ref.py, "gpu" (marked gpu) equal to the host."""
import io

import numpy as np
import pytest

from kraken_amd import agentstorage, core
from kraken_amd import device as D
from kraken_amd import piecerequest as PR
from tests import have_round_ref as R

N, P, HELD = 65, 64, (0, 3, 9, 63, 64)


def drive(placement, tmp_path):
    blob = np.random.default_rng(20261127).integers(0, 256, size=N * P - 10, dtype=np.uint8).tobytes()
    mi = core.NewMetaInfo(core.NewDigester().FromBytes(blob), io.BytesIO(blob), P)
    t = agentstorage.Torrent(mi, str(tmp_path / placement))
    for pi in HELD:
        t._commit(blob[pi * P:pi * P + mi.GetPieceLength(pi)], pi)  # WritePiece past its CRC check, which runs on the GPU
    t = agentstorage.Torrent(mi, t.path, restore=True)
    assert t.MissingPieces() == [i for i in range(N) if i not in HELD] and t.Bitfield().sum() == len(HELD)
    assert t.BytesDownloaded() == min(len(HELD) * P, len(blob))  # torrent.go:126-128 counts whole pieces
    d = PR.Dispatcher(N, PR.NewManager(PR.MockClock(), 10, PR.RarestFirstPolicy, 1))
    d.AddPeer("A", np.ones(N, bool))
    tbl = PR.RequestTable([d], placement)

    def ok(*clear, fill):
        words = np.packbits([i not in clear if fill else i in clear for i in range(128)], bitorder="little").view(np.uint64)
        if placement == "host":
            return words
        buf = D.DeviceBuffer(words.nbytes)
        buf.from_host(words)
        return buf

    with open(t.status_path, "rb") as f:
        restored = tbl.Restore(0, f.read())
    lost, new = tbl.Verified(ok(3, fill=True), "and"), tbl.Verified(ok(0, 1, 2, fill=False), "or")
    return (restored, lost, new, tbl.Handshake(), tbl.Status(), tbl.MissingPieces(), tbl.Progress()[0]["remaining"],
            tbl.have[0].tolist(), tbl.endgame(0))


def check(got):
    row = [i in (0, 1, 2, 9, 63, 64) for i in range(N)]
    assert got == ({"bad_status": False, "unexpected": 0, "complete": 5, "bytes": 0}, [[3]], [[1, 2]], [R.marshal(row)], [bytes(row)],
                   [[i for i in range(N) if not row[i]]], N - 6, row, False)


def test_host_drive(tmp_path):
    check(drive("host", tmp_path))


@pytest.mark.gpu
def test_gpu_drive_equals_the_host_drive(gpu, tmp_path):
    got = drive("gpu", tmp_path)
    check(got)
    assert got == drive("host", tmp_path)
