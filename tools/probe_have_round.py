"""A restart with the handshake out, through the have round against what a caller pays without it
(development probe, not the bench contract; no threshold): 1, 10, 100 and 1,000 torrents of 1,024
and of 81,920 pieces, each with a random `_status` sidecar.  In one session, legs alternated rep by
rep:

  have round   krk_have_round_dev over the resident rows of a piecerequest.RequestTable(placement=
               "gpu"): the sidecars uploaded, KRK_HV_RESTORE | KRK_HV_EMIT_WIRE for every torrent in
               one launch, one synchronise, the per-torrent outputs and the wire bytes read from
               page-locked memory;
  rebuild      the path without it: every sidecar to a bool array on the host, the dispatchers'
               have set from them, a fresh piecerequest.RequestTable(placement="gpu") -- every row
               packed and uploaded -- one synchronise, the rows downloaded again, and
               piecerequest.marshal_bitfield a torrent in Python.

A leg's time is the host clock around work that ends in a synchronise.  The wire bytes of the two
legs are compared.  Writes one JSON object to --out (default profiles/r20/have_round.json) and
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

SHAPES = {"1024 pieces": 1024, "81920 pieces": 81920}


def spread(t):
    return {"median_us": round(statistics.median(t) * 1e6, 1), "min_us": round(min(t) * 1e6, 1),
            "max_us": round(max(t) * 1e6, 1), "reps": len(t)}


def measure(n_pieces, n_torrents, reps, warmup, rng):
    clock = PR.MockClock()
    ds = [PR.Dispatcher(n_pieces, PR.NewManager(clock, 5, PR.RarestFirstPolicy, 3)) for _ in range(n_torrents)]
    sidecars = [rng.integers(0, 2, size=n_pieces, dtype=np.uint8).tobytes() for _ in ds]
    tbl = PR.RequestTable(ds, placement="gpu", cap=64)
    have = D.HaveBatch(tbl.batch)
    out = D.HaveOutputs(have.plan(D.HV_RESTORE | D.HV_EMIT_WIRE, dict(enumerate(sidecars))), pinned=True)
    side_dev = D.DeviceBuffer(n_pieces * n_torrents)
    times = {"have round": [], "rebuild": []}
    for rep in range(warmup + reps):
        t0 = time.perf_counter()
        have.plan(D.HV_RESTORE | D.HV_EMIT_WIRE, dict(enumerate(sidecars)))
        side_dev.from_host(have.sidecar)
        D.have_round_dev(tbl.batch, have, tbl.bits, side_dev, None, out)
        D.synchronize()
        wire = out.to_host()[7]
        wires = [have.wire_span(wire, t) for t in range(n_torrents)]
        t1 = time.perf_counter()
        for d, s in zip(ds, sidecars):
            d.have[:] = np.frombuffer(s, dtype=np.uint8) == 1
        fresh = PR.RequestTable(ds, placement="gpu", cap=64)
        D.synchronize()
        rows = fresh.bits.to_host(np.uint64, fresh.batch.total_words)
        old = [PR.marshal_bitfield(D.bitfield_bools(fresh.batch.rows(rows, t)[0], n_pieces)) for t in range(n_torrents)]
        t2 = time.perf_counter()
        if rep >= warmup:
            times["have round"].append(t1 - t0)
            times["rebuild"].append(t2 - t1)
    return {"torrents": n_torrents, "pieces": n_pieces, "sidecar_bytes": int(have.sidecar.size), "wire_bytes": int(wire.size),
            "wire_bytes_equal": wires == old, "legs": {leg: spread(t) for leg, t in times.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 10, 100, 1000])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "r20", "have_round.json"))
    a = ap.parse_args()
    D.set_device(0)
    rng = np.random.default_rng(0xC4)
    res = {"what": "restart with handshake: krk_have_round_dev (RESTORE | EMIT_WIRE) over rows resident in HBM (sidecar upload, "
                   "launch, synchronise, outputs read) against bool arrays rebuilt, a fresh piecerequest.RequestTable uploaded, "
                   "the rows downloaded and marshal_bitfield in Python; one MI355X, one session, legs alternated rep by rep",
           "date": time.strftime("%Y-%m-%d"), "cus": D.device_cus(),
           "time": "host clock around work that ends in a synchronise, microseconds", "shapes": {}}
    for name, n_pieces in SHAPES.items():
        points = []
        for k in a.batches:
            t0 = time.perf_counter()
            points.append(measure(n_pieces, k, a.reps if k < 1000 else max(3, a.reps // 3), a.warmup, rng))
            print(f"{name} x {k}: {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        res["shapes"][name] = points
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
