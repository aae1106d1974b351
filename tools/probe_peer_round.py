"""One new connection a torrent, joined where the rows lie against what a caller pays without peer
rounds (development probe, not the bench contract; no threshold): 1, 10, 100 and 1,000 torrents at
C4's shape (81,920 pieces) and at C2's (25 pieces), 10 peers and one spare slot, random bitfields.
In one session, legs alternated rep by rep:

  peer round   krk_peer_round_dev over the resident rows of a piecerequest.RequestTable(placement=
               "gpu", spare_peers=1): one join a torrent into the spare slot -- the wire bytes
               uploaded, the round launched, one synchronise, the five outputs read back;
  rebuild      a fresh piecerequest.RequestTable(placement="gpu") over dispatchers that hold the
               eleven peers: every row packed and uploaded again, one synchronise.

A leg's time is the host clock around work that ends in a synchronise.  The joined rows are compared
with the bitfields sent.  Writes one JSON object to --out (default profiles/r19/peer_round.json) and
prints it."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from kraken_amd import device as D  # noqa: E402
from kraken_amd import piecerequest as PR  # noqa: E402

SHAPES = {"C4": 81920, "C2": 25}


def spread(t):
    return {"median_us": round(statistics.median(t) * 1e6, 1), "min_us": round(min(t) * 1e6, 1),
            "max_us": round(max(t) * 1e6, 1), "reps": len(t)}


def measure(n_pieces, n_torrents, n_peers, reps, warmup, rng):
    clock = PR.MockClock()
    draw = lambda: rng.integers(0, 2, size=n_pieces, dtype=np.uint8).astype(bool)  # noqa: E731
    ds, fields = [], []
    for _ in range(n_torrents):
        d = PR.Dispatcher(n_pieces, PR.NewManager(clock, 5, PR.RarestFirstPolicy, 3))
        d.have[:] = draw()
        for p in range(n_peers):
            d.AddPeer(p, draw())
        ds.append(d)
        fields.append(draw())
    tbl = PR.RequestTable(ds, placement="gpu", cap=64, spare_peers=1)
    for d, f in zip(ds, fields):  # what the rebuild leg starts from: the new peer in the dispatcher
        d.AddPeer(n_peers, f)
    wires = [PR.marshal_bitfield(f) for f in fields]
    slots = D.PeerBatch(tbl.batch, live=[range(n_peers + 1)] * n_torrents)
    out = D.PeerOutputs(tbl.batch, pinned=True)
    wire_dev = D.DeviceBuffer(sum(len(w) for w in wires))
    times = {"peer round": [], "rebuild": []}
    for rep in range(warmup + reps):
        t0 = time.perf_counter()
        slots.events({t: [(n_peers, w)] for t, w in enumerate(wires)})
        wire_dev.from_host(slots.wire)
        D.peer_round_dev(tbl.batch, slots, tbl.bits, wire_dev, out)
        D.synchronize()
        status = out.to_host()[4]
        t1 = time.perf_counter()
        fresh = PR.RequestTable(ds, placement="gpu", cap=64)
        D.synchronize()
        t2 = time.perf_counter()
        if rep >= warmup:
            times["peer round"].append(t1 - t0)
            times["rebuild"].append(t2 - t1)
    joined = bool((status.reshape(n_torrents, n_peers + 1)[:, n_peers] & D.PE_JOINED).all())
    same = np.array_equal(tbl.bits.to_host(np.uint64, tbl.batch.total_words), fresh.bits.to_host(np.uint64, tbl.batch.total_words))
    return {"torrents": n_torrents, "pieces": n_pieces, "bits_bytes": int(tbl.batch.total_words * 8),
            "wire_bytes": int(slots.wire.size), "every_join_landed": joined, "joined_rows_equal_the_rebuilt_rows": bool(same),
            "legs": {leg: spread(t) for leg, t in times.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 10, 100, 1000])
    ap.add_argument("--peers", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "r19", "peer_round.json"))
    a = ap.parse_args()
    D.set_device(0)
    rng = np.random.default_rng(0xC4)
    res = {"what": "one join a torrent: krk_peer_round_dev over rows resident in HBM (wire upload, launch, synchronise, "
                   "outputs read) against a fresh piecerequest.RequestTable build plus the upload of all rows; one MI355X, "
                   "one session, legs alternated rep by rep",
           "date": time.strftime("%Y-%m-%d"), "cus": D.device_cus(), "peers": a.peers,
           "time": "host clock around work that ends in a synchronise, microseconds", "shapes": {}}
    for name, n_pieces in SHAPES.items():
        points = []
        for k in a.batches:
            t0 = time.perf_counter()
            points.append(measure(n_pieces, k, a.peers, a.reps if k < 1000 else max(3, a.reps // 3), a.warmup, rng))
            print(f"{name} x {k}: {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        res["shapes"][name] = points
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
