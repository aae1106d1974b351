"""castore.Listing, LastAccessTime and DirCAS.Listing(): the checks shared by
tests/test_cleanup_listing_cpu.py (placement "host") and tests/test_gpu_cleanup_listing.py
(placement "gpu").  A helper module, not a test file.  Expectations are name-by-name
transcriptions of maybeDelete (origin/blobserver/server.go:686-759) and readyForDeletion
(lib/store/cleanup.go:112-155) and the oracle's owner tables, never the library's batch calls."""
import hashlib
import os

import numpy as np

from kraken_amd import castore, hashring

HEX = "0123456789abcdefABCDEF"
GOLDEN = [(0, "0000000000000000"), (1, "0200000000000000"), (63, "7e00000000000000"), (64, "8001000000000000"),
          (-1, "0100000000000000"), (1_700_000_000, "80c49fd50c000000")]


class _Digest:
    def __init__(self, hex_):
        self.hex = hex_

    def ShardID(self):
        return self.hex[:4]


def labels_of(n):
    return [f"origin-{i:03d}.kraken.test:15002" for i in range(n)]


def ring_of(orc, labels, max_replica):
    """A Ring whose owner table comes from the device when there is one, else from the oracle."""
    from kraken_amd import device as D
    ring = hashring.Ring(labels, labels, max_replica)
    if D.device_count() == 0:
        ring._table = orc.ring_owner_table(labels, [100] * len(labels), np.ones(len(labels), dtype=np.uint8), max_replica)
    return ring


def listing_300(ring, addr):
    """The 300-name listing of test_force_cleanup_plan_equals_maybe_delete_name_by_name: one
    non-hex name, one short name, one upper-case name; (names, mtimes, now, ttl, owned)."""
    rng = np.random.default_rng(11)
    names = [hashlib.sha256(bytes([i & 255, i >> 8])).hexdigest() for i in range(300)]
    names[17] = names[17][:-1] + "g"  # not hex
    names[203] = names[203][:40]      # not 64 characters
    names[250] = names[250].upper()   # hex.DecodeString takes upper case
    now, ttl = 1_700_000_000, 3600
    mtimes = now - rng.integers(0, 2 * ttl, size=300)
    mtimes[5] = now - ttl  # not expired: the comparison is strict
    owned = next(i for i, n in enumerate(names) if i not in (17, 203) and addr in ring.Locations(_Digest(n.lower())))
    mtimes[owned] = now - ttl - 1  # expired and owned: deleted all the same
    return names, mtimes, now, ttl, owned


def check_force_cleanup_plan(orc, placement):
    labels = labels_of(5)
    ring = ring_of(orc, labels, 3)
    addr = labels[2]
    names, mtimes, now, ttl, owned = listing_300(ring, addr)
    deleted, errs = [], []  # forceCleanupHandler's loop over maybeDelete, a name at a time
    for i, name in enumerate(names):
        if len(name) != 64 or any(c not in HEX for c in name):
            errs.append(name)
            continue
        expired = now - int(mtimes[i]) > ttl
        owns_ = addr in set(ring.Locations(_Digest(name.lower())))
        if expired or not owns_:
            deleted.append(i)
    s = 1_000_000_000
    ls = castore.Listing(names, mtime_ns=mtimes * s)
    idx, errors = ls.force_cleanup_plan(now * s, ttl * s, ring, addr, placement=placement)
    assert idx.dtype == np.int64 and idx.tolist() == deleted and owned in deleted and 0 < len(deleted) < 298
    assert [e.split(":")[0] for e in errors] == errs == [names[17], names[203]]
    assert errors[0] == f"{names[17]}: parse digest: invalid sha256: hex: encoding/hex: invalid byte: U+0067 'g'"
    assert errors[1] == f'{names[203]}: parse digest: invalid sha256: expected 64 characters, got 40 from "{names[203]}"'
    # the parent's plan on the same listing
    old_idx, old_errors = castore.force_cleanup_plan(names, mtimes, now, ttl, ring, addr)
    assert old_idx.tolist() == idx.tolist() and old_errors == errors
    # parse: digests of the valid names, zero rows and error strings of the others
    digests, valid, perrors = ls.parse(placement=placement)
    assert perrors == errors and np.flatnonzero(~valid).tolist() == [17, 203]
    for i, name in enumerate(names):
        assert bytes(digests[i]) == (bytes.fromhex(name) if valid[i] else bytes(32)), i
    # every name bad: nothing to select, every name an error, each textually _parse_sha256_hex's
    bad = ["zz", "", "g" * 64, "\udcff" * 3, "A" * 63 + "\x7f"]
    idx, errors = castore.Listing(bad, mtime_ns=[0] * len(bad)).force_cleanup_plan(now * s, ttl * s, ring, addr,
                                                                                 placement=placement)
    assert idx.size == 0 and errors == [f"{b}: parse digest: {castore._parse_sha256_hex(b)[1]}" for b in bad]
    # an empty listing
    idx, errors = castore.Listing([], mtime_ns=[]).force_cleanup_plan(now * s, ttl * s, ring, addr, placement=placement)
    assert idx.size == 0 and errors == []


def ready_for_deletion(now, mtime, atime, tti, ttl):
    """cleanupManager.readyForDeletion, one file: atime None is a missing _last_access_time."""
    if ttl > 0 and now - mtime > ttl:
        return True
    if atime is None:
        return False
    return now - atime > tti


def check_cleanup_scan_plan():
    rng = np.random.default_rng(12)
    n = 200
    now, tti, ttl = 1_700_000_000_000_000_000, 6 * 3600 * 10**9, 24 * 3600 * 10**9
    names = [hashlib.sha256(bytes([i])).hexdigest() for i in range(n)]
    mtime = now - rng.integers(0, 2 * ttl, size=n)
    atime = [None if rng.random() < 0.3 else int(now - rng.integers(0, 2 * tti)) for _ in range(n)]
    mtime[0], atime[0] = now - ttl, None          # strict: not expired, no access time
    mtime[1], atime[1] = now - ttl - 1, None      # a TTL hit fires regardless of access time
    mtime[2], atime[2] = now - ttl - 1, now       # ... and with a fresh one
    mtime[3], atime[3] = now, now - tti           # strict
    mtime[4], atime[4] = now, now - tti - 1
    mtime[5], atime[5] = now, None                # a missing access time never fires the TTI term
    size = rng.integers(0, 1 << 30, size=n)
    col = np.array([castore.KRK_NO_TIME if a is None else a for a in atime], dtype=np.int64)
    ls = castore.Listing(names, mtime_ns=mtime, size=size, atime_ns=col)
    for t in (ttl, 0):  # TTL 0 disables the TTL term
        want = [i for i in range(n) if ready_for_deletion(now, int(mtime[i]), atime[i], tti, t)]
        idx, usage = ls.cleanup_scan_plan(now, tti, t)
        assert idx.dtype == np.int64 and idx.tolist() == want and 0 < len(want) < n
        assert usage == int(size.sum())  # every file counts, the deleted ones included
        assert (0 in want, 3 in want, 4 in want, 5 in want) == (False, False, True, False)
        assert (1 in want) == (2 in want) == (t > 0)


def check_last_access_time():
    for value, hex_ in GOLDEN:
        b = castore.LastAccessTime(value).Serialize()
        assert b.hex() == hex_ and len(b) == 8
        t = castore.LastAccessTime()
        t.Deserialize(b)
        assert t.Time == value
    for value in (-(1 << 40), (1 << 40) + 12345, -64, -65, 127, 128):
        t = castore.LastAccessTime()
        t.Deserialize(castore.LastAccessTime(value).Serialize())
        assert t.Time == value
    for bad, text in ((b"", "unmarshal last access time: "), (b"\x80" * 8, "unmarshal last access time: " + "\udc80" * 8)):
        try:
            castore.LastAccessTime().Deserialize(bad)
        except ValueError as e:
            assert str(e) == text
        else:
            raise AssertionError(f"no error for {bad!r}")


def check_dircas_listing(tmp_path, orc, placement):
    from kraken_amd import core
    from kraken_amd.metainfogen import DirCAS
    cas = DirCAS(str(tmp_path / "cache"))
    blobs = [bytes([i]) * (100 + i) for i in range(6)]
    hexes = [cas.WriteCacheFile(b).Hex() for b in blobs]
    now = 1_700_000_000
    want_atime = {}
    for k, h in enumerate(hexes):
        os.utime(cas.GetCacheFilePath(h), ns=((now - 100 * k) * 10**9 + 7, (now - 100 * k) * 10**9 + 7))
        if k % 2 == 0:  # a sidecar beside `data`
            with open(os.path.join(os.path.dirname(cas.GetCacheFilePath(h)), "_last_access_time"), "wb") as f:
                f.write(castore.LastAccessTime(now - 10 * k).Serialize())
            want_atime[h] = (now - 10 * k) * 10**9
    ls = cas.Listing()
    assert ls.names == sorted(hexes) and len(ls) == 6
    for i, h in enumerate(ls.names):
        k = hexes.index(h)
        assert int(ls.mtime_ns[i]) == (now - 100 * k) * 10**9 + 7 and int(ls.size[i]) == 100 + k
        assert int(ls.atime_ns[i]) == want_atime.get(h, castore.KRK_NO_TIME)
    # the scan: tti 25 s -> the files with a sidecar older than that; ttl 350 s -> the oldest mtimes
    idx, usage = ls.cleanup_scan_plan(now * 10**9, 25 * 10**9, 350 * 10**9)
    want = [i for i, h in enumerate(ls.names)
            if ready_for_deletion(now * 10**9, int(ls.mtime_ns[i]), want_atime.get(h), 25 * 10**9, 350 * 10**9)]
    assert idx.tolist() == want and 0 < len(want) < 6 and usage == sum(100 + k for k in range(6))
    # and the forced cleanup over the same listing: every name parses, expired || !owns
    labels = labels_of(4)
    ring = ring_of(orc, labels, 2)
    idx, errors = ls.force_cleanup_plan(now * 10**9, 250 * 10**9, ring, labels[1], placement=placement)
    want = [i for i, h in enumerate(ls.names)
            if now * 10**9 - int(ls.mtime_ns[i]) > 250 * 10**9 or labels[1] not in ring.Locations(core.NewSHA256DigestFromHex(h))]
    assert errors == [] and idx.tolist() == want
