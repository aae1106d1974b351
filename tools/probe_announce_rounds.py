"""One announce round, device against host (development probe, not the bench contract; no
threshold): a tracker's load in steps up to 1,000 torrents x 2,048 peers x 5 windows and 16,384
announces at limit 50 under the completeness policy, 3 origins a torrent; every older window holds
a quarter of the peers, the current one an eighth, half of them complete; an announce is a random
torrent's random peer, one in eight complete, its own index the source.  In one session, legs
alternated rep by rep:

  host           krk_announce_round over host arrays;
  gpu resident   krk_announce_round_dev, the peer stores already in HBM, handouts, counts and
                 labels in page-locked memory, then a synchronise;
  gpu upload     the same after copying the peer stores from pageable memory to HBM and followed by
                 copying them back: what peerstore.AnnounceRound(placement="gpu") pays a round.

A leg's time is the host clock around work that ends in a synchronise; the kernels' own time comes
from the library's events in a pass of its own.  Every leg's handouts and updated rows are
compared.  The crossover is the smallest load at which a GPU leg's median is below the host's, if
there is one.  Writes one JSON object to --out (default profiles/r16/announce_rounds.json) and
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
from kraken_amd._capi import check, lib  # noqa: E402


def spread(t):
    return {"median_us": round(statistics.median(t) * 1e6, 1), "min_us": round(min(t) * 1e6, 1),
            "max_us": round(max(t) * 1e6, 1), "reps": len(t)}


def measure(n_torrents, n_announces, n_peers, n_windows, limit, reps, warmup, rng):
    tors = rng.integers(0, n_torrents, size=n_announces)
    peers = rng.integers(0, n_peers, size=n_announces)
    flags = (rng.integers(0, 8, size=n_announces) == 0).astype(np.int64)
    seeds = rng.integers(0, 1 << 63, size=n_announces)
    batch = D.AnnounceBatch([(n_peers, n_windows, int(rng.integers(0, n_windows)), 3) for _ in range(n_torrents)],
                            list(zip(tors.tolist(), peers.tolist(), flags.tolist(), peers.tolist(), seeds.tolist())))
    word = lambda k: np.bitwise_and.reduce(rng.integers(0, 1 << 64, size=(k, batch.total_words), dtype=np.uint64))  # noqa: E731
    wp = (n_peers + 63) // 64
    bits = word(2).reshape(n_torrents, 2 * n_windows, wp)  # members 1/4
    bits[:, 1::2] = rng.integers(0, 1 << 64, size=bits[:, 1::2].shape, dtype=np.uint64)  # complete 1/2
    for t in range(n_torrents):  # the current window is filling up: 1/8
        cur = batch.structs[t].cur_row
        bits[t, 2 * cur] &= rng.integers(0, 1 << 64, size=wp, dtype=np.uint64)
    bits = np.ascontiguousarray(bits.reshape(-1))
    start = bits.copy()
    bits_dev, up_bits = D.DeviceBuffer(bits.nbytes), D.DeviceBuffer(bits.nbytes)
    bits_dev.from_host(bits)
    out = D.AnnounceOutputs(batch, limit, pinned=True)
    got, rows = {}, {}
    host_bits, upload_bits = start.copy(), start.copy()

    def host():
        got["host"] = D.announce_round(batch, host_bits, limit, D.AN_COMPLETENESS)
        rows["host"] = host_bits

    def resident():
        D.announce_round_dev(batch, bits_dev, limit, D.AN_COMPLETENESS, out=out)
        check(lib.krk_stream_sync(None))
        got["gpu resident"] = out.to_host()

    def upload():
        up_bits.from_host(upload_bits)
        D.announce_round_dev(batch, up_bits, limit, D.AN_COMPLETENESS, out=out)
        check(lib.krk_stream_sync(None))
        upload_bits[:] = up_bits.to_host(np.uint64, upload_bits.size)
        got["gpu upload"] = out.to_host()
        rows["gpu upload"] = upload_bits

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
    rows["gpu resident"] = bits_dev.to_host(np.uint64, bits.size)
    same = all(all(np.array_equal(x, y) for x, y in zip(got[k], got["host"])) and np.array_equal(rows[k], rows["host"])
               for k in legs)
    with D.KernelTimer():
        for _ in range(max(3, reps // 2)):
            resident()
        D.synchronize()
        calls, ms = D.KernelTimer.stats("announce_round")
    n_out = got["host"][1]
    return {"torrents": n_torrents, "announces": n_announces, "bits_bytes": int(bits.nbytes),
            "peers_handed_out": int(n_out.sum()), "full_handouts": int((n_out == limit + 3).sum()),
            "every_leg_gave_the_same_handouts_and_rows": bool(same),
            "kernels_us_events": round(ms / max(calls, 1) * 1e3, 1), "legs": {k: spread(t) for k, t in times.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--loads", type=int, nargs="+", default=[1, 16, 10, 160, 100, 1638, 1000, 16384],
                    help="pairs: torrents announces")
    ap.add_argument("--peers", type=int, default=2048)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--limit", type=int, default=50)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "r16", "announce_rounds.json"))
    a = ap.parse_args()
    D.set_device(0)
    rng = np.random.default_rng(0xA22)
    res = {"what": "one announce round (every announcer written into its torrent's current peer-set window, then "
                   "every handout sampled, origins appended, ordered by completeness): krk_announce_round on the host "
                   "against krk_announce_round_dev with the peer stores already in HBM and with their upload and "
                   "download; one MI355X, one session, legs alternated rep by rep",
           "date": time.strftime("%Y-%m-%d"), "cus": D.device_cus(), "pci_bus_id": D.device_pci_bus_id(),
           "peers": a.peers, "windows": a.windows, "limit": a.limit, "origins": 3,
           "time": "host clock around work that ends in a synchronise, microseconds", "loads": [], "crossover": {}}
    for n_torrents, n_announces in zip(a.loads[::2], a.loads[1::2]):
        t0 = time.perf_counter()
        res["loads"].append(measure(n_torrents, n_announces, a.peers, a.windows, a.limit, a.reps, a.warmup, rng))
        print(f"{n_torrents} torrents x {n_announces} announces: {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    res["crossover"] = {
        leg: next((p["announces"] for p in res["loads"] if p["legs"][leg]["median_us"] < p["legs"]["host"]["median_us"]), None)
        for leg in ("gpu resident", "gpu upload")}
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
