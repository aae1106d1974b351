"""Re-piecing a cache against regenerating it (development probe, not the bench contract):
seconds of Generator.RepieceAll on the host placement, on the GPU placement, and of
Generator.RegenerateAll, each bringing the same DirCAS of synthetic files from 1 MiB to 4 MiB
pieces, legs alternated rep by rep, the 1 MiB sidecars put back (untimed) before every leg.  Warm
page cache: the files were just written.  Then the re-piece kernel's own time, from the library's
events, for a batch of stored sums alone: C3's length law (20,000 blobs of 100 MiB + rng mod
968,884,225 B, about 2.8 M sums at 4 MiB) re-pieced to 16 MiB, beside the host form's wall time."""
import argparse
import ctypes as C
import hashlib
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from kraken_amd import core, metainfogen  # noqa: E402
from kraken_amd import device as D  # noqa: E402
from kraken_amd._capi import check, krk_repiece_blob, lib  # noqa: E402

MIB = 1 << 20


def spread(t):
    return {"median_s": round(statistics.median(t), 5), "min_s": round(min(t), 5), "max_s": round(max(t), 5)}


def cache_legs(a):
    root = tempfile.mkdtemp(dir=a.dir)
    try:
        cas = metainfogen.DirCAS(root)
        base = np.random.default_rng(1).integers(0, 256, size=a.mb << 20, dtype=np.uint8)
        for i in range(a.files):
            base[:8] = np.frombuffer(np.uint64(i).tobytes(), np.uint8)
            cas.WriteCacheFileAs(core.NewSHA256DigestFromHex(hashlib.sha256(base).hexdigest()), base)
        total = a.files * (a.mb << 20)
        metainfogen.New({0: MIB}, cas).RegenerateAll()
        old = {n: cas.GetCacheFileMetadata(n) for n in cas.ListNames()}
        g = metainfogen.New({0: 4 * MIB}, cas)
        g.RegenerateAll()
        want = {n: cas.GetCacheFileMetadata(n) for n in old}

        def restore():
            for n, raw in old.items():
                with open(os.path.join(os.path.dirname(cas.GetCacheFilePath(n)), "_torrentmeta"), "wb") as f:
                    f.write(raw)

        legs = {"repiece_all_host": lambda: g.RepieceAll("host"), "repiece_all_gpu": lambda: g.RepieceAll("gpu"),
                "regenerate_all": lambda: g.RegenerateAll()}
        for f in legs.values():  # warm: staging pinned, rates measured, scratch blocks allocated
            restore()
            f()
        times = {k: [] for k in legs}
        for _ in range(a.reps):
            for k, f in legs.items():
                restore()
                t0 = time.perf_counter()
                r = f()
                times[k].append(time.perf_counter() - t0)
                assert r["changed"] == a.files and r.get("reread", 0) == 0, (k, r)
                assert {n: cas.GetCacheFileMetadata(n) for n in old} == want, k
        res = {"files": a.files, "mb": a.mb, "bytes": total, "reps": a.reps, "page_cache": "warm",
               "change": "1 MiB -> 4 MiB"}
        for k, t in times.items():
            res[k] = spread(t)
        res["regenerate_all"]["median_GBps"] = round(total / statistics.median(times["regenerate_all"]) / 1e9, 2)
        return res
    finally:
        shutil.rmtree(root, ignore_errors=True)


def kernel_leg(a):
    rng = np.random.default_rng(0xC3)
    L = 100 * MIB + rng.integers(0, 968_884_225, a.blobs)
    po, pn = 4 * MIB, 16 * MIB
    n_old, n_new = (L + po - 1) // po, (L + pn - 1) // pn
    so = np.concatenate([[0], np.cumsum(n_old)[:-1]])
    oo = np.concatenate([[0], np.cumsum(n_new)[:-1]])
    arr = (krk_repiece_blob * a.blobs)()
    for i in range(a.blobs):
        arr[i] = krk_repiece_blob(int(L[i]), po, pn, int(so[i]), int(oo[i]))
    old = rng.integers(0, 1 << 32, size=int(n_old.sum()), dtype=np.uint64).astype(np.uint32)
    u32p = C.POINTER(C.c_uint32)
    host_out = np.zeros(int(n_new.sum()), dtype=np.uint32)
    host_t = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        check(lib.krk_repiece_batch(arr, a.blobs, old.ctypes.data_as(u32p), host_out.ctypes.data_as(u32p)))
        host_t.append(time.perf_counter() - t0)
    d_old, d_out = D.DeviceBuffer(old.nbytes), D.DeviceBuffer(host_out.nbytes)
    d_old.from_host(old)
    check(lib.krk_repiece_batch_dev(arr, a.blobs, d_old.ptr, d_out.ptr, None))  # warm
    D.synchronize()
    kern_ms, call_t = [], []
    for _ in range(a.reps):
        with D.KernelTimer():
            t0 = time.perf_counter()
            check(lib.krk_repiece_batch_dev(arr, a.blobs, d_old.ptr, d_out.ptr, None))
            D.synchronize()
            call_t.append(time.perf_counter() - t0)
            n, ms = D.KernelTimer.stats("piece_repiece")
            assert n == 1
            kern_ms.append(ms / 1e3)
    assert np.array_equal(d_out.to_host(np.uint32, host_out.size), host_out)
    return {"blobs": a.blobs, "old_sums": int(old.size), "new_sums": int(host_out.size), "change": "4 MiB -> 16 MiB",
            "kernel": spread(kern_ms), "device_call_and_sync": spread(call_t), "host_form": spread(host_t),
            "kernel_old_sums_per_s": round(old.size / statistics.median(kern_ms))}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--mb", type=int, default=32)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blobs", type=int, default=20_000)
    a = ap.parse_args()
    D.set_device(0)
    print(json.dumps({"cache": cache_legs(a), "sums_batch": kernel_leg(a)}), flush=True)


if __name__ == "__main__":
    main()
