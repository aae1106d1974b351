"""One resend round for a batch of torrents, device against host (development probe, not the bench
contract; no threshold): 1, 10, 100 and 1,000 torrents at C4's shape (81,920 pieces) and at C2's
(25 pieces), 10 peers and 30 failed requests each (random pieces, peers and statuses), random
bitfields (have 1/2, peers 1/2, blocked 1/8), every quota 3.  In one session, legs alternated rep by
rep:

  host           krk_piece_resend_round over host arrays;
  gpu resident   krk_piece_resend_round_dev, bits and quota already in HBM (the rows a reserve
                 round uploaded), targets and n_resent in page-locked memory, then a synchronise;
  gpu upload     the same after copying bits and quota from pageable memory to HBM: what
                 piecerequest.ResendRound(placement="gpu") pays a round.

A leg's time is the host clock around work that ends in a synchronise; the kernel's own time comes
from the library's events in a pass of its own.  Every leg's targets are compared.  The crossover
is the smallest batch at which a GPU leg's median is below the host's, if there is one.  Writes one
JSON object to --out (default profiles/r15/piece_resends.json) and prints it."""
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


def measure(n_pieces, n_torrents, n_peers, n_failed, reps, warmup, rng):
    batch = D.RequestBatch([n_pieces] * n_torrents, n_peers)
    bits = rng.integers(0, 1 << 64, size=batch.total_words, dtype=np.uint64)
    for t in range(n_torrents):  # blocked rows: 1/8
        rows = batch.rows(bits, t)
        rows[2::2] &= rng.integers(0, 1 << 64, size=rows[2::2].shape, dtype=np.uint64)
        rows[2::2] &= rng.integers(0, 1 << 64, size=rows[2::2].shape, dtype=np.uint64)
    quota = np.full(batch.total_peers, 3, dtype=np.int32)
    pieces = np.sort(rng.integers(0, n_pieces, size=(n_torrents, n_failed)), axis=1)
    peers = rng.integers(0, n_peers, size=(n_torrents, n_failed))
    status = rng.integers(1, 4, size=(n_torrents, n_failed))
    resend = D.ResendBatch(batch, [list(zip(pieces[t].tolist(), peers[t].tolist(), status[t].tolist()))
                                   for t in range(n_torrents)])
    bits_dev, quota_dev = D.DeviceBuffer(bits.nbytes), D.DeviceBuffer(quota.nbytes)
    bits_dev.from_host(bits)
    quota_dev.from_host(quota)
    up_bits, up_quota = D.DeviceBuffer(bits.nbytes), D.DeviceBuffer(quota.nbytes)
    out = D.ResendOutputs(batch, resend, quota_left=False, pinned=True)
    got = {}

    def host():
        got["host"] = D.piece_resend_round(batch, resend, bits, quota, quota_left=False)

    def resident():
        D.piece_resend_round_dev(batch, resend, bits_dev, quota_dev, out=out)
        check(lib.krk_stream_sync(None))
        got["gpu resident"] = out.to_host()

    def upload():
        up_bits.from_host(bits)
        up_quota.from_host(quota)
        D.piece_resend_round_dev(batch, resend, up_bits, up_quota, out=out)
        check(lib.krk_stream_sync(None))
        got["gpu upload"] = out.to_host()

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
    same = all(np.array_equal(got[k][0], got["host"][0]) and np.array_equal(got[k][2], got["host"][2]) for k in legs)
    with D.KernelTimer():
        for _ in range(max(3, reps // 2)):
            resident()
        D.synchronize()
        calls, ms = D.KernelTimer.stats("piece_resend")
    return {"torrents": n_torrents, "pieces": n_pieces, "bits_bytes": int(bits.nbytes), "failed": int(resend.total_failed),
            "resent": int(got["host"][2].sum()), "every_leg_gave_the_same_targets": bool(same),
            "kernel_us_events": round(ms / max(calls, 1) * 1e3, 1), "legs": {k: spread(t) for k, t in times.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 10, 100, 1000])
    ap.add_argument("--peers", type=int, default=10)
    ap.add_argument("--failed", type=int, default=30)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "r15", "piece_resends.json"))
    a = ap.parse_args()
    D.set_device(0)
    rng = np.random.default_rng(0xC4)
    res = {"what": "one resend round (every failed piece request placed on the first peer that may take it): "
                   "krk_piece_resend_round on the host against krk_piece_resend_round_dev with the bitfields "
                   "already in HBM and with their upload; one MI355X, one session, legs alternated rep by rep",
           "date": time.strftime("%Y-%m-%d"), "cus": D.device_cus(), "pci_bus_id": D.device_pci_bus_id(),
           "peers": a.peers, "failed_a_torrent": a.failed,
           "time": "host clock around work that ends in a synchronise, microseconds", "shapes": {}, "crossover": {}}
    for name, n_pieces in SHAPES.items():
        points = []
        for k in a.batches:
            t0 = time.perf_counter()
            points.append(measure(n_pieces, k, a.peers, a.failed, a.reps, a.warmup, rng))
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
