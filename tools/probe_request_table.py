"""One reserve step and one resend step of the download loop, resident tables against the rebuilt
rows (development probe, not the bench contract; no threshold): 1, 10, 100 and 1,000 torrents at
C4's shape (81,920 pieces) and at C2's (25 pieces), 10 peers, pipeline limit 3, rarest first, random
bitfields (have 1/2, peers 1/2).  In one session, legs alternated rep by rep:

  table gpu    piecerequest.RequestTable(placement="gpu", cap=--cap): rows and tables in HBM, a step is table
               round, request (or resend) round, table round, and one synchronise (two for a resend);
  round gpu    piecerequest.ReserveRound / ResendRound(placement="gpu") over Manager: rows rebuilt
               from the dicts and uploaded every step;
  round host   the same with placement="host".

Every rep starts from empty request tables at a clock one timeout later (the Manager's dicts
cleared, the resident counts zeroed, outside the timed region), so each reserve step places 30
requests a torrent into a table of --cap entries (default 64, not the library's most, 4096: the
reference holds 30); before the resend step the requests of peer 0 are marked unsent.  A leg's time
is the host clock around work that ends in a synchronise.  Every leg's picks and targets are
compared.  Writes one JSON object to --out (default profiles/r18/request_table.json) and prints it."""
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
TIMEOUT, LIMIT = 5, 3


def spread(t):
    return {"median_us": round(statistics.median(t) * 1e6, 1), "min_us": round(min(t) * 1e6, 1),
            "max_us": round(max(t) * 1e6, 1), "reps": len(t)}


def measure(n_pieces, n_torrents, n_peers, cap, reps, warmup, rng):
    clock = PR.MockClock()
    ds = []
    for _ in range(n_torrents):
        d = PR.Dispatcher(n_pieces, PR.NewManager(clock, TIMEOUT, PR.RarestFirstPolicy, LIMIT), disable_endgame=True)
        d.have[:] = rng.integers(0, 2, size=n_pieces, dtype=np.uint8).astype(bool)
        for p in range(n_peers):
            d.AddPeer(p, rng.integers(0, 2, size=n_pieces, dtype=np.uint8).astype(bool))
        ds.append(d)
    tbl = PR.RequestTable(ds, placement="gpu", cap=cap)
    zero = np.zeros(n_torrents, dtype=np.uint32)
    got = {}

    def reset():
        clock.Add(TIMEOUT + 1)
        for d in ds:
            d.manager.requests.clear()
            d.manager.requestsByPeer.clear()
        tbl.n_entries.from_host(zero)

    def step(leg):
        if leg == "table gpu":
            picks = tbl.Reserve()
            for t, g in enumerate(picks):
                for i in g[0]:
                    tbl.MarkUnsent(t, 0, i)
            return picks, lambda: [[(r.Piece, r.PeerID, r.Status, to) for r, to in g] for g in tbl.Resend()]
        placement = leg.split()[1]
        picks = PR.ReserveRound(ds, placement=placement)
        for d, g in zip(ds, picks):
            for i in g[0]:
                d.manager.MarkUnsent(0, i)
        return picks, lambda: [[(r.Piece, r.PeerID, r.Status, to) for r, to in g] for g in PR.ResendRound(ds, placement=placement)]

    legs = ("table gpu", "round gpu", "round host")
    times = {(leg, kind): [] for leg in legs for kind in ("reserve", "resend")}
    for rep in range(warmup + reps):
        for leg in legs:
            reset()
            t0 = time.perf_counter()
            picks, resend = step(leg)
            t1 = time.perf_counter()
            targets = resend()
            t2 = time.perf_counter()
            got[leg] = (picks, targets)
            if rep >= warmup:
                times[leg, "reserve"].append(t1 - t0)
                times[leg, "resend"].append(t2 - t1)
    same = all(got[leg] == got["round host"] for leg in legs)
    return {"torrents": n_torrents, "pieces": n_pieces, "bits_bytes": int(tbl.batch.total_words * 8),
            "requests_a_step": sum(len(v) for g in got["round host"][0] for v in g.values()),
            "resent_a_step": sum(1 for g in got["round host"][1] for r in g if r[3] is not None),
            "every_leg_gave_the_same_picks_and_targets": bool(same),
            "legs": {f"{leg}, {kind}": spread(t) for (leg, kind), t in times.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 10, 100, 1000])
    ap.add_argument("--peers", type=int, default=10)
    ap.add_argument("--cap", type=int, default=64, help="entries a table holds (the library's most is 4096)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "r18", "request_table.json"))
    a = ap.parse_args()
    D.set_device(0)
    rng = np.random.default_rng(0xC4)
    res = {"what": "one reserve step and one resend step of the download loop: piecerequest.RequestTable with rows and "
                   "request tables resident in HBM against ReserveRound / ResendRound over Manager on the GPU (rows "
                   "rebuilt and uploaded a step) and on the host; one MI355X, one session, legs alternated rep by rep",
           "date": time.strftime("%Y-%m-%d"), "cus": D.device_cus(), "peers": a.peers, "table_cap": a.cap,
           "limit": LIMIT, "time": "host clock around work that ends in a synchronise, microseconds", "shapes": {}}
    for name, n_pieces in SHAPES.items():
        points = []
        for k in a.batches:
            t0 = time.perf_counter()
            points.append(measure(n_pieces, k, a.peers, a.cap, a.reps if k < 1000 else max(3, a.reps // 3), a.warmup, rng))
            print(f"{name} x {k}: {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        res["shapes"][name] = points
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
