"""One piece request round for a batch of torrents, device against host (development probe, not the
bench contract; no threshold): 1, 10, 100 and 1,000 torrents at C4's shape (81,920 pieces) and at
C2's (25 pieces), 10 peers each, pipeline limit 3, rarest first, random bitfields (have 1/2, peers
1/2, blocked 1/8), every quota 3.  In one session, legs alternated rep by rep:

  host           krk_piece_request_round over host arrays;
  gpu resident   krk_piece_request_round_dev, bits and quota already in HBM, picks and n_picked in
                 page-locked memory, then a synchronise;
  gpu upload     the same after copying bits and quota from pageable memory to HBM: what
                 piecerequest.ReserveRound(placement="gpu") pays a round, since have and blocked
                 change between rounds.

A leg's time is the host clock around work that ends in a synchronise; the kernels' own time comes
from the library's events in a pass of its own.  Every leg's picks are compared.  The crossover is
the smallest batch at which a GPU leg's median is below the host's, if there is one.  Writes one
JSON object to --out (default profiles/r14/piece_requests.json) and prints it."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from kraken_amd import device as D  # noqa: E402
from kraken_amd._capi import check, lib  # noqa: E402

SHAPES = {"C4": 81920, "C2": 25}


def spread(t):
    return {"median_us": round(statistics.median(t) * 1e6, 1), "min_us": round(min(t) * 1e6, 1),
            "max_us": round(max(t) * 1e6, 1), "reps": len(t)}


def measure(n_pieces, n_torrents, n_peers, limit, reps, warmup, rng):
    batch = D.RequestBatch([n_pieces] * n_torrents, n_peers, D.PR_RAREST_FIRST)
    bits = rng.integers(0, 1 << 64, size=batch.total_words, dtype=np.uint64)
    for t in range(n_torrents):  # blocked rows: 1/8
        rows = batch.rows(bits, t)
        rows[2::2] &= rng.integers(0, 1 << 64, size=rows[2::2].shape, dtype=np.uint64)
        rows[2::2] &= rng.integers(0, 1 << 64, size=rows[2::2].shape, dtype=np.uint64)
    quota = np.full(batch.total_peers, limit, dtype=np.int32)
    bits_dev, quota_dev = D.DeviceBuffer(bits.nbytes), D.DeviceBuffer(quota.nbytes)
    bits_dev.from_host(bits)
    quota_dev.from_host(quota)
    up_bits, up_quota = D.DeviceBuffer(bits.nbytes), D.DeviceBuffer(quota.nbytes)
    out = D.RequestOutputs(batch, limit, pinned=True)
    got = {}

    def host():
        got["host"] = D.piece_request_round(batch, bits, quota, limit)[1:]

    def resident():
        D.piece_request_round_dev(batch, bits_dev, quota_dev, limit, out=out)
        check(lib.krk_stream_sync(None))
        got["gpu resident"] = out.to_host()[1:]

    def upload():
        up_bits.from_host(bits)
        up_quota.from_host(quota)
        D.piece_request_round_dev(batch, up_bits, up_quota, limit, out=out)
        check(lib.krk_stream_sync(None))
        got["gpu upload"] = out.to_host()[1:]

    legs = {"host": host, "gpu resident": resident, "gpu upload": upload}
    for f in legs.values():
        for _ in range(warmup):
            f()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, f in legs.items():
            t0 = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t0)
    same = all(np.array_equal(got[k][0], got["host"][0]) and np.array_equal(got[k][1], got["host"][1]) for k in legs)
    with D.KernelTimer():
        for _ in range(max(3, reps // 2)):
            resident()
        D.synchronize()
        calls, ms = D.KernelTimer.stats("piece_request")
    return {"torrents": n_torrents, "pieces": n_pieces, "bits_bytes": int(bits.nbytes), "picks": int(got["host"][1].sum()),
            "every_leg_gave_the_same_picks": bool(same), "kernels_us_events": round(ms / max(calls, 1) * 1e3, 1),
            "legs": {k: spread(t) for k, t in times.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 10, 100, 1000])
    ap.add_argument("--peers", type=int, default=10)
    ap.add_argument("--limit", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--budget-s", type=float, default=6.0, help="host-leg seconds a point may take; reps shrink to fit")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "r14", "piece_requests.json"))
    a = ap.parse_args()
    D.set_device(0)
    rng = np.random.default_rng(0xC4)
    res = {"what": "one piece request round (availability counts + rarest-first picks for every peer of every torrent): "
                   "krk_piece_request_round on the host against krk_piece_request_round_dev with the bitfields "
                   "already in HBM and with their upload; one MI355X, one session, legs alternated rep by rep",
           "date": time.strftime("%Y-%m-%d"), "cus": D.device_cus(), "pci_bus_id": D.device_pci_bus_id(),
           "peers": a.peers, "limit": a.limit, "policy": "rarest_first",
           "time": "host clock around work that ends in a synchronise, microseconds", "shapes": {}, "crossover": {}}
    for name, n_pieces in SHAPES.items():
        points = []
        for k in a.batches:
            t0 = time.perf_counter()
            probe = measure(n_pieces, k, a.peers, a.limit, 1, 1, rng)  # sizes the reps
            per = max(probe["legs"]["host"]["median_us"] * 1e-6, 1e-6)
            reps = int(max(3, min(a.reps, a.budget_s / per)))
            points.append(measure(n_pieces, k, a.peers, a.limit, reps, a.warmup, rng))
            print(f"{name} x {k}: {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        res["shapes"][name] = points
        res["crossover"][name] = {
            leg: next((p["torrents"] for p in points if p["legs"][leg]["median_us"] < p["legs"]["host"]["median_us"]), None)
            for leg in ("gpu resident", "gpu upload")}
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
