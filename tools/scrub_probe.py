"""Whole-cache scrub against regeneration (development probe, not the bench contract): seconds
and GB/s of Generator.VerifyAll (read-only: piece sums alone, and with the SHA-256 pass) beside
Generator.RegenerateAll over the same DirCAS of synthetic files, legs alternated rep by rep.
Warm page cache: the files were just written.  RegenerateAll is the code the scrub's parent
commit has (the scrub adds entry points, it changes none), so its leg is the parent's number
for this cache.  Ends with what each tool says about one flipped byte."""
import argparse
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


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--mb", type=int, default=32)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    D.set_device(0)
    root = tempfile.mkdtemp(dir=a.dir)
    try:
        cas = metainfogen.DirCAS(root)
        base = np.random.default_rng(1).integers(0, 256, size=a.mb << 20, dtype=np.uint8)
        names = []
        for i in range(a.files):
            base[:8] = np.frombuffer(np.uint64(i).tobytes(), np.uint8)
            d = core.NewSHA256DigestFromHex(hashlib.sha256(base).hexdigest())
            cas.WriteCacheFileAs(d, base)
            names.append(d.Hex())
        total = a.files * (a.mb << 20)
        g = metainfogen.New({0: 4 << 20}, cas)
        legs = {"regenerate_all": lambda: g.RegenerateAll(),
                "verify_all_sums": lambda: g.VerifyAll(check_digest=False),
                "verify_all_sums_and_digest": lambda: g.VerifyAll(check_digest=True)}
        for f in legs.values():  # warm: sidecars written, staging pinned, rates measured
            f()
        times = {k: [] for k in legs}
        for _ in range(a.reps):
            for k, f in legs.items():
                t0 = time.perf_counter()
                r = f()
                times[k].append(time.perf_counter() - t0)
                assert r.get("changed", 0) == 0 and not r.get("corrupt"), (k, r)
        res = {"files": a.files, "mb": a.mb, "bytes": total, "reps": a.reps, "page_cache": "warm",
               "crc_split_last_call": D.crc_host_split()[:2]}
        for k, t in times.items():
            res[k] = {"median_s": round(statistics.median(t), 4), "min_s": round(min(t), 4), "max_s": round(max(t), 4),
                      "median_GBps": round(total / statistics.median(t) / 1e9, 2)}
        # one flipped byte: the scrub names the piece and leaves the evidence; regeneration
        # overwrites the sidecar, after which only the digest pass still sees the damage
        victim = sorted(names)[len(names) // 2]
        with open(cas.GetCacheFilePath(victim), "r+b") as f:
            f.seek((a.mb << 20) // 2 + 1)
            b = f.read(1)
            f.seek((a.mb << 20) // 2 + 1)
            f.write(bytes([b[0] ^ 1]))
        res["flipped_byte"] = {"scrub_before_regen": g.VerifyAll()["corrupt"], "regenerate_all": g.RegenerateAll(),
                               "scrub_sums_after_regen": g.VerifyAll(check_digest=False)["corrupt"],
                               "scrub_digest_after_regen": g.VerifyAll()["corrupt"]}
        print(json.dumps(res), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
