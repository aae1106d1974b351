"""A forced-cleanup plan from a raw cache listing, end to end (development probe, not the bench
contract): C5's 1,000,000 seeded random digests as hex names with mtimes, 16 origins, MaxReplica
3, one origin's share (`expired || !owns` with that origin's owns mask), in one session, legs
alternated rep by rep:

  parent            castore.force_cleanup_plan: a Python loop a character, numpy expiry bits, then
                    Ring.Select -- over the first --parent-names names only (it takes seconds a
                    100,000), in the first --parent-reps reps;
  listing host      castore.Listing.force_cleanup_plan(placement="host"): krk_cleanup_plan;
  listing gpu pageable / pinned
                    placement="gpu": krk_cleanup_plan_dev, the text, offsets and mtimes uploaded by
                    every call from pageable memory, or read in place from page-locked memory
                    (Listing.pin()); results in page-locked memory either way;
  listing gpu first call
                    the pageable leg on a Listing packed just before (not timed): the call also
                    allocates the listing's device buffers and page-locked outputs; in the first
                    --first-reps reps;
  hbm fused / hbm unfused
                    text, offsets and mtimes already in HBM: krk_cleanup_plan_dev against
                    krk_digest_parse_hex_dev + krk_ring_select_dev (the expired bitset for the
                    latter is computed beforehand and waits in HBM, which favours the unfused
                    chain), results in device memory.

A leg's time is the host clock around work that ends in a synchronise; the kernels' own time comes
from the library's events in passes of their own.  Packing the listing (castore.Listing(...)) is
timed once, apart.  Writes one JSON object to --out (default profiles/r12/cleanup_plan.json) and
prints it."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from kraken_amd import castore, hashring  # noqa: E402
from kraken_amd import device as D  # noqa: E402
from kraken_amd._capi import check, lib  # noqa: E402

u64p, i64p = C.POINTER(C.c_uint64), C.POINTER(C.c_int64)


def spread(t):
    return {"median_us": round(statistics.median(t) * 1e6, 1), "min_us": round(min(t) * 1e6, 1),
            "max_us": round(max(t) * 1e6, 1), "reps": len(t)}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--names", type=int, default=1_000_000)
    ap.add_argument("--nodes", type=int, default=16)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-names", type=int, default=100_000)
    ap.add_argument("--parent-reps", type=int, default=3)
    ap.add_argument("--first-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "r12", "cleanup_plan.json"))
    a = ap.parse_args()
    D.set_device(0)
    n, N, R = a.names, a.nodes, 3
    labels = [f"origin-{i:03d}.kraken.test:15002" for i in range(N)]
    ring = hashring.Ring(labels, labels, R)
    addr = labels[0]
    mask = ring.ShardMaskOwns(addr)
    rng = np.random.default_rng(0xC5)
    dig = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    names = [bytes(r).hex() for r in dig]
    now, ttl = 1_700_000_000 * 10**9, 3600 * 10**9
    mtime = now - rng.integers(0, ttl * 8 // 7, size=n)  # one in eight expired
    t0 = time.perf_counter()
    pageable = castore.Listing(names, mtime_ns=mtime)
    pack_s = time.perf_counter() - t0
    pinned = castore.Listing(names, mtime_ns=mtime).pin()
    pn = min(a.parent_names, n)
    p_names, p_mtime = names[:pn], mtime[:pn]

    # text already in HBM
    words = (n + 63) // 64
    hbm = {"text": D.DeviceBuffer(pageable.text.nbytes), "off": D.DeviceBuffer(pageable.off.nbytes),
           "mtime": D.DeviceBuffer(8 * n), "digests": D.DeviceBuffer(32 * n), "valid": D.DeviceBuffer(8 * words),
           "expired": D.DeviceBuffer(8 * words), "bits": D.DeviceBuffer(8 * words), "idx": D.DeviceBuffer(8 * n),
           "count": D.DeviceBuffer(8)}
    hbm["text"].from_host(pageable.text)
    hbm["off"].from_host(pageable.off)
    hbm["mtime"].from_host(pageable.mtime_ns)
    expired = np.zeros(words, dtype=np.uint64)
    check(lib.krk_expiry_bits(pageable.mtime_ns.ctypes.data_as(i64p), None, n, now, ttl, 0, expired.ctypes.data_as(u64p)))
    hbm["expired"].from_host(expired)
    mp = mask.ctypes.data_as(u64p)

    def fused():
        check(lib.krk_cleanup_plan_dev(hbm["text"].ptr, hbm["off"].ptr, n, hbm["mtime"].ptr, now, ttl, mp, 1,
                                       hbm["bits"].ptr, hbm["valid"].ptr, hbm["idx"].ptr, n, hbm["count"].ptr, None))
        check(lib.krk_stream_sync(None))

    def unfused():
        check(lib.krk_digest_parse_hex_dev(hbm["text"].ptr, hbm["off"].ptr, n, hbm["digests"].ptr, None,
                                           hbm["valid"].ptr, None))
        check(lib.krk_ring_select_dev(hbm["digests"].ptr, n, mp, 1, hbm["expired"].ptr, hbm["bits"].ptr,
                                      hbm["idx"].ptr, n, hbm["count"].ptr, None))
        check(lib.krk_stream_sync(None))

    results = {}

    def listing_leg(ls, placement):
        def f():
            results[placement if placement == "host" else f"gpu {id(ls)}"] = ls.force_cleanup_plan(now, ttl, ring, addr,
                                                                                                 placement=placement)
        return f

    legs = {"listing host": listing_leg(pageable, "host"),
            "listing gpu pageable": listing_leg(pageable, "gpu"),
            "listing gpu pinned": listing_leg(pinned, "gpu"),
            "hbm fused": fused, "hbm unfused": unfused}

    def parent():
        results["parent"] = castore.force_cleanup_plan(p_names, p_mtime, now, ttl, ring, addr)

    for f in legs.values():  # warm: owner table built, scratch blocks, staging and the listings' buffers allocated
        for _ in range(a.warmup):
            f()
    times = {k: [] for k in ["parent", "listing gpu first call", *legs]}
    for rep in range(a.reps):
        order = (["parent"] if rep < a.parent_reps else []) + list(legs)
        for k in order:
            f = parent if k == "parent" else legs[k]
            t0 = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t0)
        if rep < a.first_reps:
            fresh = castore.Listing(names, mtime_ns=mtime)
            t0 = time.perf_counter()
            results["first"] = fresh.force_cleanup_plan(now, ttl, ring, addr, placement="gpu")
            times["listing gpu first call"].append(time.perf_counter() - t0)
            del fresh
    # every leg gave the same plan
    want = results["host"][0]
    same = all(np.array_equal(v[0], want) for k, v in results.items() if k != "parent")
    same = same and np.array_equal(results["parent"][0], want[want < pn])
    fused()
    c = int(hbm["count"].to_host(np.uint64, 1)[0])
    same = same and c == want.size and np.array_equal(hbm["idx"].to_host(np.uint64, c).astype(np.int64), want)
    unfused()
    c2 = int(hbm["count"].to_host(np.uint64, 1)[0])
    same = same and c2 == c and np.array_equal(hbm["idx"].to_host(np.uint64, c2).astype(np.int64), want)
    kern = {}
    for k, kn in (("hbm fused", ["cleanup_plan"]), ("hbm unfused", ["digest_parse_hex", "ring_select"])):
        with D.KernelTimer():
            for _ in range(20):
                legs[k]()
            D.synchronize()
            kern[k] = {x: round(D.KernelTimer.stats(x)[1] / max(D.KernelTimer.stats(x)[0], 1) * 1e3, 1) for x in kn}
    res = {"what": "a forced-cleanup plan (expired || !owns) from a raw listing of hex names and mtimes, end to end: "
                   "castore.force_cleanup_plan (the parent's code) against castore.Listing on the host, on the GPU "
                   "from pageable and from page-locked memory, and the fused device call against parse + ring_select "
                   "with the text already in HBM; one MI355X, one session, legs alternated rep by rep",
           "date": time.strftime("%Y-%m-%d"), "cus": D.device_cus(), "pci_bus_id": D.device_pci_bus_id(),
           "names": n, "nodes": N, "max_replica": R, "selected": int(want.size), "errors": len(results["host"][1]),
           "every_leg_gave_the_same_plan": bool(same),
           "time": "host clock around work that ends in a synchronise, microseconds",
           "pack_listing_once_us": round(pack_s * 1e6, 1),
           "parent_note": f"the parent leg runs over the first {pn} names only, in the first {a.parent_reps} reps; "
                          f"names_per_s makes the legs comparable",
           "legs": {}, "kernel_us_events": kern}
    for k, t in times.items():
        m = pn if k == "parent" else n
        res["legs"][k] = {**spread(t), "names": m, "names_per_s": round(m / statistics.median(t))}
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
