"""Thirty piece requests a torrent answered, through the serve round against the same work done one
message at a time in Python (development probe, not the bench contract; no threshold): 1, 10, 100
and 1,000 torrents of 25 pieces (C2's shape) and of 81,920 (C4's), 10 peers each, have 3/4 full, one
request in ten malformed.  In one session, legs alternated rep by rep:

  device round  piecerequest.RequestTable(placement="gpu"): the requests queued with Requested,
                one Serve() -- krk_serve_round_dev over the rows resident in HBM, one synchronise,
                the outputs read from page-locked memory and turned into the send lists;
  host round    the same calls with placement="host": krk_serve_round over numpy rows;
  per message   handlePieceRequest in plain Python over the dispatchers' bool arrays: the length
                rule, the have bit, the send, the peer's bit and its clock, a message at a time.

A leg's time is the host clock around work that ends in a synchronise (the device leg) or returns
its lists (the others).  The sends of the three legs are compared.  Writes one JSON object to --out
(default profiles/r21/serve_round.json) and prints it."""
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

SHAPES = {"C2 (25 pieces)": 25, "C4 (81,920 pieces)": 81920}
PEERS, REQS, PIECE = 10, 30, 1 << 18


def spread(t):
    return {"median_us": round(statistics.median(t) * 1e6, 1), "min_us": round(min(t) * 1e6, 1),
            "max_us": round(max(t) * 1e6, 1), "reps": len(t)}


def per_message(ds, reqs, now, sent):
    """handlePieceRequest a message: one send list a torrent."""
    out = []
    for t, d in enumerate(ds):
        sends, total = [], 0
        for peerID, i, off, ln in reqs[t]:
            plen = 0 if i < 0 or i >= d.n_pieces else d.length - d.piece_length * i if i == d.n_pieces - 1 else d.piece_length
            if off != 0 or ln != plen or i < 0 or i >= d.n_pieces or not d.have[i]:
                continue
            sends.append((peerID, i, d.piece_length * i, ln, total))
            total += ln
            sent[t, peerID] = now
            d.peers[peerID][i] = True
        out.append(sends)
    return out


def measure(n_pieces, n_torrents, reps, warmup, rng):
    clock = PR.MockClock(1)
    pool = [rng.random(n_pieces) < 0.5 for _ in range(16)]
    ds = []
    for t in range(n_torrents):
        d = PR.Dispatcher(n_pieces, PR.NewManager(clock, 5, PR.RarestFirstPolicy, 3))
        d.length, d.piece_length = n_pieces * PIECE - 5, PIECE
        d.have[:] = rng.random(n_pieces) < 0.75
        for p in range(PEERS):
            d.AddPeer(p, pool[(t + p) % 16])
        ds.append(d)
    tables = {"device round": PR.RequestTable(ds, placement="gpu", cap=64), "host round": PR.RequestTable(ds, placement="host", cap=64)}
    times, same = {leg: [] for leg in (*tables, "per message")}, True
    for rep in range(warmup + reps):
        reqs = [[(int(rng.integers(PEERS)), int(rng.integers(n_pieces)), int(rng.random() < 0.05),
                  PIECE - (1 if rng.random() < 0.05 else 0)) for _ in range(REQS)] for _ in ds]
        got = {}
        for leg, tbl in tables.items():
            t0 = time.perf_counter()
            for t, qs in enumerate(reqs):
                for q in qs:
                    tbl.Requested(t, *q)
            got[leg] = [r["sends"] for r in tbl.Serve()]
            times[leg].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        got["per message"] = per_message(ds, reqs, clock.Now(), {})
        times["per message"].append(time.perf_counter() - t0)
        same = same and got["device round"] == got["host round"] == got["per message"]
    return {"torrents": n_torrents, "pieces": n_pieces, "requests": REQS * n_torrents, "sends_equal": same,
            "legs": {leg: spread(t[warmup:]) for leg, t in times.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 10, 100, 1000])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "r21", "serve_round.json"))
    a = ap.parse_args()
    D.set_device(0)
    rng = np.random.default_rng(0xC4)
    res = {"what": "30 piece requests a torrent answered: RequestTable.Requested + Serve with placement gpu (krk_serve_round_dev over "
                   "rows resident in HBM, one synchronise, outputs read) and host (krk_serve_round), against handlePieceRequest "
                   "a message in plain Python; 10 peers; one MI355X, one session, legs alternated rep by rep",
           "date": time.strftime("%Y-%m-%d"), "cus": D.device_cus(),
           "time": "host clock around work that ends in a synchronise or returns its lists, microseconds", "shapes": {}}
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
