"""One connection round, device against host (development probe, not the bench contract; no
threshold): 16, 1,000 and 16,384 torrents of 1,024 known peers, each with one announce handout of 72
dials, 16 incoming handshakes with neighbour rows and 16 transitions; a quarter of a torrent's peers
are active or pending, one in sixteen is blacklisted, the capacity is 40.  In one session, legs
alternated rep by rep, every rep from the same state (restored outside the timed region):

  host           krk_conn_round over host arrays;
  gpu resident   krk_conn_round_dev, rows, expiries, capacities and neighbour rows already in HBM,
                 statuses and counts in page-locked memory, then a synchronise;
  gpu copied     the same after copying the state and the neighbour rows from pageable memory to HBM
                 and followed by copying the state back: what connstate.ConnRound(placement="gpu")
                 pays a round.

A leg's time is the host clock around work that ends in a synchronise; the kernel's own time comes
from the library's events in a pass of its own.  Every leg's outputs and state are compared.  Writes
one JSON object to --out (default profiles/r17/conn_rounds.json) and prints it."""
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

NOW, DURATION, MAX_MUTUAL, CAPACITY = 1000, 30, 40, 40


def spread(t):
    return {"median_us": round(statistics.median(t) * 1e6, 1), "min_us": round(min(t) * 1e6, 1),
            "max_us": round(max(t) * 1e6, 1), "reps": len(t)}


def measure(n_torrents, n_peers, n_dial, n_in, n_trans, reps, warmup, rng):
    wp = (n_peers + 63) // 64
    lists = []
    for _ in range(n_torrents):
        tr = np.sort(rng.choice(n_peers, size=n_trans, replace=False))
        kinds = rng.integers(0, 4, size=n_trans)
        rows = rng.integers(0, 1 << 64, size=(n_in, wp), dtype=np.uint64) & rng.integers(0, 1 << 64, size=(n_in, wp), dtype=np.uint64)
        lists.append((list(zip(tr.tolist(), kinds.tolist())),
                      [(int(p), rows[j]) for j, p in enumerate(rng.integers(0, n_peers, size=n_in))],
                      rng.integers(0, n_peers, size=n_dial).tolist()))
    batch = D.ConnBatch([(n_peers, 0, 0)] * n_torrents, lists)
    word = lambda k: np.bitwise_and.reduce(rng.integers(0, 1 << 64, size=(k, n_torrents, wp), dtype=np.uint64))  # noqa: E731
    active = word(3)                 # 1/8
    pending = word(3) & ~active      # about 1/8, disjoint
    start = [np.ascontiguousarray(np.stack([active, pending], axis=1).reshape(-1)),
             np.where(rng.integers(0, 16, size=batch.total_peers) == 0, NOW + 5, 0).astype(np.int64),
             np.full(n_torrents, CAPACITY, dtype=np.uint32)]
    dev = [D.DeviceBuffer(a.nbytes) for a in start]
    copied = [D.DeviceBuffer(a.nbytes) for a in start]
    neigh_dev, neigh_copied = D.DeviceBuffer(batch.neighbors.nbytes), D.DeviceBuffer(batch.neighbors.nbytes)
    neigh_dev.from_host(batch.neighbors)
    out = D.ConnOutputs(batch, pinned=True)
    got, state = {}, {}
    host_state, copied_state = [a.copy() for a in start], [a.copy() for a in start]

    def restore(leg):
        if leg == "host":
            for a, s in zip(host_state, start):
                a[:] = s
        elif leg == "gpu resident":
            for b, s in zip(dev, start):
                b.from_host(s)
        else:
            for a, s in zip(copied_state, start):
                a[:] = s

    def host():
        got["host"] = D.conn_round(batch, *host_state, NOW, DURATION, MAX_MUTUAL)
        state["host"] = host_state

    def resident():
        D.conn_round_dev(batch, *dev, neigh_dev, NOW, DURATION, MAX_MUTUAL, out=out)
        check(lib.krk_stream_sync(None))
        got["gpu resident"] = out.to_host()

    def copied_leg():
        for b, a in zip(copied, copied_state):
            b.from_host(a)
        neigh_copied.from_host(batch.neighbors)
        D.conn_round_dev(batch, *copied, neigh_copied, NOW, DURATION, MAX_MUTUAL, out=out)
        check(lib.krk_stream_sync(None))
        for b, a in zip(copied, copied_state):
            a[:] = b.to_host(a.dtype, a.size)
        got["gpu copied"] = out.to_host()
        state["gpu copied"] = copied_state

    legs = {"host": host, "gpu resident": resident, "gpu copied": copied_leg}
    for k, f in legs.items():
        for _ in range(warmup):
            restore(k)
            f()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, f in legs.items():
            restore(k)
            t0 = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t0)
    state["gpu resident"] = [b.to_host(a.dtype, a.size) for b, a in zip(dev, start)]
    same = all(all(np.array_equal(x, y) for x, y in zip(got[k], got["host"])) and
               all(np.array_equal(x, y) for x, y in zip(state[k], state["host"])) for k in legs)
    with D.KernelTimer():
        for _ in range(max(3, reps // 2)):
            restore("gpu resident")
            resident()
        D.synchronize()
        calls, ms = D.KernelTimer.stats("conn_round")
    ts, ins, ds, n_adm, n_freed = got["host"]
    return {"torrents": n_torrents, "state_bytes": int(sum(a.nbytes for a in start)),
            "neighbour_bytes": int(batch.neighbors.nbytes), "entries": int(ts.size + ins.size + ds.size),
            "incoming_admitted": int(n_adm[:, 0].sum()), "dials_admitted": int(n_adm[:, 1].sum()), "freed": int(n_freed.sum()),
            "every_leg_gave_the_same_outputs_and_state": bool(same),
            "kernel_us_events": round(ms / max(calls, 1) * 1e3, 1), "legs": {k: spread(t) for k, t in times.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--torrents", type=int, nargs="+", default=[16, 1000, 16384])
    ap.add_argument("--peers", type=int, default=1024)
    ap.add_argument("--dials", type=int, default=72)
    ap.add_argument("--incoming", type=int, default=16)
    ap.add_argument("--transitions", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "r17", "conn_rounds.json"))
    a = ap.parse_args()
    D.set_device(0)
    rng = np.random.default_rng(0xC0)
    res = {"what": "one connection round (transitions, then incoming handshakes under the capacity and the mutual "
                   "limit, then one announce handout's dials): krk_conn_round on the host against krk_conn_round_dev "
                   "with the state already in HBM and with the state copied both ways; one MI355X, one session, legs "
                   "alternated rep by rep",
           "date": time.strftime("%Y-%m-%d"), "cus": D.device_cus(), "pci_bus_id": D.device_pci_bus_id(),
           "peers": a.peers, "dials": a.dials, "incoming": a.incoming, "transitions": a.transitions,
           "capacity": CAPACITY, "max_mutual": MAX_MUTUAL,
           "time": "host clock around work that ends in a synchronise, microseconds", "loads": [], "crossover": {}}
    for n in a.torrents:
        t0 = time.perf_counter()
        res["loads"].append(measure(n, a.peers, a.dials, a.incoming, a.transitions, a.reps, a.warmup, rng))
        print(f"{n} torrents: {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    res["crossover"] = {
        leg: next((p["torrents"] for p in res["loads"] if p["legs"][leg]["median_us"] < p["legs"]["host"]["median_us"]), None)
        for leg in ("gpu resident", "gpu copied")}
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
