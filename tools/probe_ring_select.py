"""Ownership answered as owner lists against ownership answered as a bitset (development probe,
not the bench contract): over the same device-resident digests (C5's: 1,000,000 seeded random
32-byte digests, 16 origins, MaxReplica 3), in one session, legs alternated rep by rep,

  locations_u8     krk_ring_locations_u8_dev: R + 1 bytes a digest (owner lists + counts), which a
                   caller then scans on the host for its own address (the scan is not timed);
  select f=0|1/N|1 krk_ring_select_dev with a mask that selects none, the shards one origin owns on
                   a MaxReplica-1 ring (1/N of them) and all: 1/8 byte a digest plus, with the
                   index list, 8 bytes a selected one (`bits_only` legs pass no index list),

each with its outputs in page-locked host memory (on the host when the stream ends, no copy) and
in device memory (no copy back timed).  A leg's time is the host clock around the call and the
wait for its stream; the kernels' own time comes from the library's events in passes of their own.
Prints one JSON object."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from kraken_amd import device as D  # noqa: E402
from kraken_amd import hashring  # noqa: E402
from kraken_amd._capi import check, lib  # noqa: E402

u64p = C.POINTER(C.c_uint64)


def spread(t):
    return {"median_us": round(statistics.median(t) * 1e6, 1), "min_us": round(min(t) * 1e6, 1),
            "max_us": round(max(t) * 1e6, 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--digests", type=int, default=1_000_000)
    ap.add_argument("--nodes", type=int, default=16)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    D.set_device(0)
    n, N, R = a.digests, a.nodes, 3
    labels = [f"origin-{i:03d}.kraken.test:15002" for i in range(N)]
    healthy = np.ones(N, dtype=np.uint8)
    dig = np.random.default_rng(0xC5).integers(0, 256, size=(n, 32), dtype=np.uint8)
    dbuf = D.DeviceBuffer(32 * n)
    dbuf.from_host(dig.reshape(-1))
    words = (n + 63) // 64
    masks = {"0": np.zeros(1024, dtype=np.uint64),
             "1/N": hashring.Ring(labels, labels, 1).ShardMaskOwns(labels[0]),
             "1": np.full(1024, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)}

    def outputs(pinned):
        mk = (lambda k, dt: D.PinnedArray((k,), dt)) if pinned else (lambda k, dt: D.DeviceBuffer(k * np.dtype(dt).itemsize))
        return {"locs": mk(n * R, np.uint8), "counts": mk(n, np.uint8), "bits": mk(words, np.uint64),
                "idx": mk(n, np.uint64), "count": mk(1, np.uint64)}

    legs, selected = {}, {}
    for where in ("pinned", "device"):
        o = outputs(where == "pinned")

        def loc(o=o):
            D.ring_locations_u8_dev(dbuf, n, labels, healthy, R, o["locs"], o["counts"])

        legs[f"locations_u8 {where}"] = (loc, "hrw_gather", o)
        for f, mask in masks.items():
            for bits_only in (False, True):
                def sel(o=o, mask=mask, bits_only=bits_only):
                    check(lib.krk_ring_select_dev(dbuf.ptr, n, mask.ctypes.data_as(u64p), 0, None, o["bits"].ptr,
                                                  None if bits_only else o["idx"].ptr, 0 if bits_only else n,
                                                  o["count"].ptr, None))

                legs[f"select f={f}{' bits_only' if bits_only else ''} {where}"] = (sel, "ring_select", o)
    for name, (f, _, o) in legs.items():  # warm: owner table built, scratch blocks and staging allocated
        for _ in range(a.warmup):
            f()
        D.synchronize()
        if name.startswith("select"):
            c = o["count"]
            selected[name] = int(c.a[0] if isinstance(c, D.PinnedArray) else c.to_host(np.uint64, 1)[0])
    times = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, (f, _, _) in legs.items():
            t0 = time.perf_counter()
            f()
            check(lib.krk_stream_sync(None))
            times[k].append(time.perf_counter() - t0)
    kern = {}
    for k, (f, kname, _) in legs.items():  # the kernels' own time, a pass of its own a leg
        with D.KernelTimer():
            for _ in range(20):
                f()
            D.synchronize()
            cnt, ms = D.KernelTimer.stats(kname)
        kern[k] = round(ms / max(cnt, 1) * 1e3, 1)
    res = {"what": "krk_ring_locations_u8_dev against krk_ring_select_dev over the same device-resident digests, "
                   "one MI355X, one session, legs alternated rep by rep",
           "date": time.strftime("%Y-%m-%d"), "cus": D.device_cus(), "pci_bus_id": D.device_pci_bus_id(),
           "digests": n, "nodes": N, "max_replica": R, "reps": a.reps,
           "time": "host clock around the call and the wait for its stream, microseconds",
           "legs": {}}
    for k in legs:
        if k.startswith("locations"):
            out_bytes = n * (R + 1)
        else:
            out_bytes = 8 * words + 8 + (0 if "bits_only" in k else 8 * selected[k])
        res["legs"][k] = {**spread(times[k]), "kernel_us_events": kern[k], "output_bytes": out_bytes,
                          **({"selected": selected[k]} if k in selected else {}),
                          "digests_per_s": round(n / statistics.median(times[k]))}
    print(json.dumps(res, indent=1), flush=True)


if __name__ == "__main__":
    main()
