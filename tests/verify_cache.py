"""The six-blob CAS cache the VerifyAll tests scrub (tests/test_verify_cpu.py without the
digest pass, tests/test_gpu_verify.py with it), built from the oracle's sums and digests, and
the numpy reference for bitfield words."""
import os

import numpy as np

from kraken_amd import core, metainfogen

PIECE = 1024
CONFIG = {0: PIECE}
SIZES = {"good": 5000, "flipped": 7001, "regenerated": 4096, "no_meta": 3000, "truncated": 6000, "garbage": 2500}
FLIP_AT = 2 * PIECE + 17  # a byte of piece 2


def ref_words(ok) -> np.ndarray:
    """willf/bitset words of a bool-per-piece array, from numpy alone."""
    ok = np.asarray(ok, dtype=bool)
    padded = np.zeros((ok.size + 63) // 64 * 64, dtype=np.uint8)
    padded[:ok.size] = ok
    return np.packbits(padded, bitorder="little").view("<u8").astype(np.uint64)


def _metainfo(orc, data: np.ndarray, name: str) -> core.MetaInfo:
    sums = orc.calc_piece_sums(data, PIECE)[1]
    sums = np.asarray(sums, dtype=np.uint32) if data.size else None
    ih = core._info_hash(PIECE, sums if sums is not None else np.zeros(0, np.uint32), name, int(data.size))
    return core.MetaInfo(PIECE, sums, name, int(data.size), core.NewSHA256DigestFromHex(name), ih)


def build_cache(orc, root: str, only_good: bool = False):
    """A DirCAS under `root` and {case: blob name}: one blob untouched; one with a flipped data
    byte; one whose _torrentmeta was rewritten from the flipped bytes (the sums agree, the
    digest does not); one without its sidecar; one truncated; one with garbage in the sidecar.
    only_good: the same six blobs, all intact."""
    cas = metainfogen.DirCAS(root)
    names = {}
    for k, (case, size) in enumerate(SIZES.items()):
        data = orc.synth(8800 + k, size)
        name = orc.sha256(data).hex()
        names[case] = name
        d = core.NewSHA256DigestFromHex(name)
        cas.WriteCacheFileAs(d, data)
        cas.SetCacheFileMetadata(name, _metainfo(orc, data, name))
        if only_good:
            continue
        path = cas.GetCacheFilePath(name)
        meta = os.path.join(os.path.dirname(path), "_torrentmeta")
        if case in ("flipped", "regenerated"):
            rotten = data.copy()
            rotten[FLIP_AT] ^= 0x40
            with open(path, "wb") as f:
                f.write(memoryview(rotten))
            if case == "regenerated":  # what RegenerateAll leaves behind over rotten bytes
                cas.SetCacheFileMetadata(name, _metainfo(orc, rotten, name))
        elif case == "no_meta":
            os.remove(meta)
        elif case == "truncated":
            with open(path, "r+b") as f:
                f.truncate(size - 1500)
        elif case == "garbage":
            with open(meta, "wb") as f:
                f.write(b"\x00not json at all{")
    return cas, names


def snapshot(root: str) -> dict:
    """{relative path: (bytes, mtime_ns)} of every file under root."""
    out = {}
    for dirpath, _, files in os.walk(root):
        for fn in files:
            p = os.path.join(dirpath, fn)
            with open(p, "rb") as f:
                out[os.path.relpath(p, root)] = (f.read(), os.stat(p).st_mtime_ns)
    return out


def expected_report(names: dict, check_digest: bool) -> dict:
    """What VerifyAll must return for build_cache's cache, entry by entry (bad_meta's error
    text is checked by the caller)."""
    dg = (lambda v: v) if check_digest else (lambda v: None)
    corrupt = [
        {"name": names["flipped"], "reason": "pieces", "bad_pieces": [FLIP_AT // PIECE], "digest_ok": dg(False)},
        {"name": names["no_meta"], "reason": "missing_meta", "bad_pieces": [], "digest_ok": None},
        {"name": names["truncated"], "reason": "length", "bad_pieces": [], "digest_ok": None},
        {"name": names["garbage"], "reason": "bad_meta", "bad_pieces": [], "digest_ok": None},
    ]
    if check_digest:  # only the digest catches a sidecar regenerated over rotten bytes
        corrupt.append({"name": names["regenerated"], "reason": "digest", "bad_pieces": [], "digest_ok": False})
    corrupt.sort(key=lambda c: c["name"])
    return {"blobs": len(names), "ok": len(names) - len(corrupt), "corrupt": corrupt}


def check_report(got: dict, names: dict, check_digest: bool):
    want = expected_report(names, check_digest)
    assert got["blobs"] == want["blobs"] and got["ok"] == want["ok"], got
    assert [c["name"] for c in got["corrupt"]] == [c["name"] for c in want["corrupt"]], got
    for g, w in zip(got["corrupt"], want["corrupt"]):
        g = dict(g)
        err = g.pop("error", None)
        assert g == w, (g, w)
        if w["reason"] == "bad_meta":
            assert err and err.startswith("json: "), err
        else:
            assert err is None
