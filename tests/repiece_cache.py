"""A small DirCAS for the re-piece tests (tests/test_repiece_cpu.py, tests/test_gpu_repiece.py): a
dozen blobs of 0 bytes to 1 MiB with their _torrentmeta under OLD, to be brought to NEW.  A helper
module, not a test file."""
import hashlib
import os

import numpy as np

from kraken_amd import core, metainfogen

KIB = 1024
OLD = {0: 64 * KIB}
NEW = {0: 256 * KIB, 512 * KIB: 1024 * KIB}
SIZES = (0, 3000, 64 * KIB, 64 * KIB + 1, 200_000, 256 * KIB, 256 * KIB + 1, 400_000, 512 * KIB - 1, 512 * KIB, 700_000,
         1024 * KIB)


def blob(seed, size):
    """(bytes, their core.Digest)."""
    data = np.random.default_rng(seed).integers(0, 256, size=size, dtype=np.uint8).tobytes()
    return data, core.NewSHA256DigestFromHex(hashlib.sha256(data).hexdigest())


def build_cache(root):
    """(DirCAS under root, blob names in SIZES' order), the sidecars regenerated under OLD."""
    cas = metainfogen.DirCAS(root)
    names = []
    for k, size in enumerate(SIZES):
        data, d = blob(9000 + k, size)
        cas.WriteCacheFileAs(d, data)
        names.append(d.Hex())
    assert metainfogen.New(OLD, cas).RegenerateAll() == {"blobs": len(SIZES), "changed": len(SIZES)}
    return cas, names


def sidecars(cas):
    return {name: cas.GetCacheFileMetadata(name) for name in cas.ListNames()}


def meta_path(cas, name):
    return os.path.join(os.path.dirname(cas.GetCacheFilePath(name)), "_torrentmeta")


def zero_data(cas, name):
    """The blob's bytes replaced by zeros of the same size: a sidecar computed from a read of this
    file can no longer equal the one computed from the real bytes."""
    size = cas.GetCacheFileStat(name).st_size
    with open(cas.GetCacheFilePath(name), "wb") as f:
        f.write(bytes(size))
