"""Weighted rendezvous placement of the CAS store's 256 shard directories over
volumes (lib/store/ca_store.go:137-171, initCASVolumes): for subdir "%02X" the
top node of GetOrderedNodes(subdir, 1) over the volumes (murmur3 +
UInt64ToFloat64, per-volume weights) owns it; the store symlinks
<dir>/<subdir> -> <volume>/<basename(dir)>/<subdir>.  The ordering runs on the
GPU through the same HRW kernel as the hashring (krk_hrw_ordered)."""
from __future__ import annotations

import os
import posixpath

from .hrw import NewRendezvousHash


class Volume:
    def __init__(self, Location: str, Weight: int):
        self.Location, self.Weight = Location, int(Weight)


def volume_subdirs(volumes) -> dict:
    """{subdir "%02X": volume location} for the 256 shard directories."""
    rh = NewRendezvousHash()
    for v in volumes:
        rh.AddNode(v.Location, v.Weight)
    keys = [f"{i:02X}" for i in range(256)]
    order = rh.GetOrderedNodesBatch(keys, 1)
    return {k: rh.Nodes[int(order[i, 0])].Label for i, k in enumerate(keys)}


def initCASVolumes(dir_: str, volumes) -> None:
    """ca_store.go:137-171 with the same error strings."""
    if not volumes:
        return
    for v in volumes:
        if not os.path.exists(v.Location):
            raise OSError(f"verify volume: stat {v.Location}: no such file or directory")
    base = posixpath.basename(posixpath.normpath(dir_)) if dir_ else "."  # Go path.Base
    for sub, loc in volume_subdirs(volumes).items():
        src = posixpath.join(loc, base, sub)
        try:
            os.makedirs(src, mode=0o775, exist_ok=True)
        except OSError as e:
            raise OSError(f"volume source path: {e}") from e
        tgt = posixpath.join(dir_, sub)
        try:
            _create_or_update_symlink(src, tgt)
        except OSError as e:
            raise OSError(f"symlink to volume: {e}") from e


def _create_or_update_symlink(src: str, tgt: str) -> None:
    """createOrUpdateSymlink (lib/store/utils.go:25-47): an existing target that is not
    a symlink (a regular file, a real directory) is an error and is left in place;
    a symlink to another source is replaced; a missing target is created."""
    try:
        os.stat(tgt)  # follows links, like os.Stat
    except FileNotFoundError:
        os.symlink(src, tgt)
        return
    existing = os.readlink(tgt)  # OSError (EINVAL) when tgt is not a symlink
    if existing != src:
        os.remove(tgt)
        os.symlink(src, tgt)


def _parse_sha256_hex(name: str):
    """core.NewSHA256DigestFromHex (core/digest.go:57-68, 152-161): (32 raw bytes, None) or
    (None, the reference's error text)."""
    import json
    raw = name.encode("utf-8", "surrogateescape")
    if len(raw) != 64:
        return None, f"invalid sha256: expected 64 characters, got {len(raw)} from {json.dumps(name)}"
    for c in raw:  # hex.DecodeString reports the first byte that is no hex digit
        if chr(c) not in "0123456789abcdefABCDEF":
            shown = f"U+{c:04X} '{chr(c)}'" if 0x20 <= c < 0x7F else f"U+{c:04X}"
            return None, f"invalid sha256: hex: encoding/hex: invalid byte: {shown}"
    return bytes.fromhex(name), None


def force_cleanup_plan(names, mtimes, now, ttl, ring, addr):
    """What forceCleanupHandler -> maybeDelete (origin/blobserver/server.go:686-759) would delete
    from a cache listing, as a plan: (delete_idx, errors).  delete_idx are the positions in
    `names`, in listing order, of the files with expired || !owns, where expired is
    now - mtime > ttl and owns is addr in ring.Locations(digest); a name that is no SHA-256 hex
    goes to errors as "<name>: parse digest: ..." and is never selected.  Nothing is deleted: the
    persist / writeback handling and the deletion stay with the caller.  One shard mask
    (Ring.ShardMaskOwns) and one selection over all digests (Ring.Select) instead of a
    Locations call a file."""
    import numpy as np
    names = list(names)
    mt = np.asarray(mtimes)
    assert mt.shape == (len(names),)
    errors, good, digests = [], [], []
    for i, name in enumerate(names):
        raw, err = _parse_sha256_hex(name)
        if err is not None:
            errors.append(f"{name}: parse digest: {err}")
        else:
            good.append(i)
            digests.append(raw)
    good = np.asarray(good, dtype=np.int64)
    if not good.size:
        return np.empty(0, dtype=np.int64), errors
    d = np.frombuffer(b"".join(digests), dtype=np.uint8).reshape(-1, 32)
    expired = (now - mt[good]) > ttl
    or_bits = np.packbits(expired, bitorder="little")
    or_bits = np.concatenate([or_bits, np.zeros(-or_bits.size % 8, dtype=np.uint8)]).view(np.uint64)
    _, idx = ring.Select(d, ring.ShardMaskOwns(addr), invert=True, or_bits=or_bits)
    return good[idx.astype(np.int64)], errors


# ---------------------------------------------------------------- cleanup plans from a raw listing
KRK_DHEX_LEN, KRK_DHEX_BYTE = 0x40000000, 0x80000000
KRK_NO_TIME = -(1 << 63)  # a missing _last_access_time in an access-time column


class LastAccessTime:
    """metadata.LastAccessTime (lib/store/metadata/last_access_time.go:55-70): the
    _last_access_time sidecar, Unix seconds as binary.PutVarint into 8 zero-padded bytes."""
    Suffix = "_last_access_time"

    def __init__(self, Time: int = 0):
        self.Time = int(Time)

    def Serialize(self) -> bytes:
        x = self.Time
        ux = ((x << 1) ^ (x >> 63)) & 0xFFFFFFFFFFFFFFFF  # zigzag
        out = bytearray()
        while ux >= 0x80:
            out.append((ux & 0x7F) | 0x80)
            ux >>= 7
        out.append(ux)
        if len(out) > 8:
            raise IndexError("index out of range")  # PutVarint panics past the 8-byte buffer
        return bytes(out) + bytes(8 - len(out))

    def Deserialize(self, b: bytes) -> None:
        ux, n = 0, 0  # binary.Uvarint
        for i, c in enumerate(b):
            if i == 10 or (i == 9 and c > 1):
                n = -(i + 1)  # overflow
                break
            ux |= (c & 0x7F) << (7 * i)
            if c < 0x80:
                n = i + 1
                break
        if n <= 0:
            raise ValueError("unmarshal last access time: " + bytes(b).decode("utf-8", "surrogateescape"))
        x = ux >> 1
        self.Time = ~x if ux & 1 else x


class Listing:
    """A cache listing as ListCacheFiles() and GetCacheFileStat give it: names, and columns of
    mtime (ns), size and last access time (ns, KRK_NO_TIME where the sidecar is missing).  The
    names are packed once into the library's listing layout (bytes back to back and n + 1
    offsets); parsing, expiry and ring selection then run in the library over the whole listing,
    on the host (placement "host", the default) or on the device ("gpu": a missing device is an
    error, never a fall-back)."""

    def __init__(self, names, mtime_ns=None, size=None, atime_ns=None):
        import numpy as np
        self.names = list(names)
        n = len(self.names)
        raw = [nm.encode("utf-8", "surrogateescape") for nm in self.names]
        self.off = np.zeros(n + 1, dtype=np.uint64)
        if n:
            np.cumsum(np.fromiter(map(len, raw), dtype=np.uint64, count=n), out=self.off[1:])
        self.text = np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8)  # one spare byte, never read

        def column(a):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.int64)
            assert a.shape == (n,)
            return a

        self.mtime_ns, self.size, self.atime_ns = column(mtime_ns), column(size), column(atime_ns)
        self._pinned = None
        self._gpu = None

    def __len__(self):
        return len(self.names)

    # ------------------------------------------------------------ memory
    def pin(self) -> "Listing":
        """Keep the text, the offsets and the mtimes in page-locked memory (krk_host_alloc), which
        the device reads in place: the "gpu" placement then uploads nothing."""
        from . import device as D
        if self._pinned is None:
            cols = {"text": self.text, "off": self.off}
            if self.mtime_ns is not None:
                cols["mtime"] = self.mtime_ns
            self._pinned = {}
            for k, a in cols.items():
                p = D.PinnedArray(a.shape, a.dtype)
                p.a[:] = a
                self._pinned[k] = p
        return self

    def _device_inputs(self, with_mtime: bool):
        """(text, off, mtime or None) pointers the device reads: the pinned copies, or device
        buffers (allocated once) the columns are uploaded into by this call."""
        from . import device as D
        if self._pinned is not None:
            p = self._pinned
            return p["text"].ptr, p["off"].ptr, p["mtime"].ptr if with_mtime else None
        if self._gpu is None:
            self._gpu = {"text": D.DeviceBuffer(self.text.nbytes), "off": D.DeviceBuffer(self.off.nbytes)}
        g = self._gpu
        g["text"].from_host(self.text)
        g["off"].from_host(self.off)
        if with_mtime:
            if "mtime" not in g:
                g["mtime"] = D.DeviceBuffer(max(self.mtime_ns.nbytes, 8))
            g["mtime"].from_host(self.mtime_ns)
        return g["text"].ptr, g["off"].ptr, g["mtime"].ptr if with_mtime else None

    def _outputs(self, key, shape, dtype):
        """A page-locked output of the "gpu" placement, allocated once a listing."""
        from . import device as D
        if self._gpu is None:
            self._gpu = {}
        if key not in self._gpu:
            self._gpu[key] = D.PinnedArray(shape, dtype)
        return self._gpu[key]

    @staticmethod
    def _check_placement(placement):
        if placement not in ("host", "gpu"):
            raise ValueError(f"placement must be 'host' or 'gpu', not {placement!r}")
        if placement == "gpu":
            from . import device as D
            if D.device_count() == 0:
                from ._capi import KRK_ENODEV, KrakenError
                raise KrakenError(KRK_ENODEV, "placement 'gpu': no gfx950 device")

    def _errors(self, valid):
        """The reference's error text of every invalid name, in listing order."""
        import numpy as np
        out = []
        for i in np.flatnonzero(~valid):
            name = self.names[int(i)]
            out.append(f"{name}: parse digest: {_parse_sha256_hex(name)[1]}")
        return out

    # ------------------------------------------------------------ calls
    def parse(self, placement="host"):
        """core.NewSHA256DigestFromHex of every name: (digests32 uint8 [n, 32] -- zero rows for the
        invalid names --, valid bool [n], errors: "<name>: parse digest: ..." of the invalid names)."""
        import ctypes as C

        import numpy as np

        from ._capi import check, lib
        self._check_placement(placement)
        n = len(self)
        words = (n + 63) // 64
        if placement == "host":
            digests = np.zeros((n, 32), dtype=np.uint8)
            vbits = np.zeros(words, dtype=np.uint64)
            check(lib.krk_digest_parse_hex(self.text.ctypes.data, self.off.ctypes.data_as(C.POINTER(C.c_uint64)), n,
                                           digests.ctypes.data, None, vbits.ctypes.data_as(C.POINTER(C.c_uint64))))
        else:
            text, off, _ = self._device_inputs(False)
            d = self._outputs("digests", (n, 32), np.uint8)
            v = self._outputs("valid", (words,), np.uint64)
            check(lib.krk_digest_parse_hex_dev(text, off, n, d.ptr, None, v.ptr, None))
            check(lib.krk_stream_sync(None))
            digests, vbits = d.a.copy(), v.a.copy()
        valid = np.unpackbits(vbits.view(np.uint8), bitorder="little")[:n].astype(bool)
        return digests, valid, self._errors(valid)

    def force_cleanup_plan(self, now_ns, ttl_ns, ring, addr, placement="host"):
        """force_cleanup_plan over the listing itself: (delete_idx int64 ascending -- positions in
        the listing of the names with expired || !owns --, errors).  One call of krk_cleanup_plan
        (or krk_cleanup_plan_dev) with Ring.ShardMaskOwns(addr) inverted: no digest array, no
        expired bitset and no mapping back from a compacted sublisting."""
        import ctypes as C

        import numpy as np

        from ._capi import check, lib
        self._check_placement(placement)
        assert self.mtime_ns is not None, "force_cleanup_plan needs the mtime column"
        n = len(self)
        words = (n + 63) // 64
        u64p = C.POINTER(C.c_uint64)
        mask = np.ascontiguousarray(ring.ShardMaskOwns(addr), dtype=np.uint64)
        if placement == "host":
            bits, vbits = np.zeros(words, dtype=np.uint64), np.zeros(words, dtype=np.uint64)
            idx = np.zeros(n, dtype=np.uint64)
            count = C.c_uint64()
            check(lib.krk_cleanup_plan(self.text.ctypes.data, self.off.ctypes.data_as(u64p), n,
                                       self.mtime_ns.ctypes.data_as(C.POINTER(C.c_int64)), int(now_ns), int(ttl_ns),
                                       mask.ctypes.data_as(u64p), 1, bits.ctypes.data_as(u64p), vbits.ctypes.data_as(u64p),
                                       idx.ctypes.data_as(u64p) if n else None, n, C.byref(count)))
            idx = idx[:count.value]
        else:
            text, off, mtime = self._device_inputs(True)
            b = self._outputs("bits", (words,), np.uint64)
            v = self._outputs("valid", (words,), np.uint64)
            ix = self._outputs("idx", (n,), np.uint64)
            c = self._outputs("count", (1,), np.uint64)
            check(lib.krk_cleanup_plan_dev(text, off, n, mtime, int(now_ns), int(ttl_ns), mask.ctypes.data_as(u64p), 1,
                                           b.ptr if n else None, v.ptr if n else None, ix.ptr if n else None, n, c.ptr,
                                           None))
            check(lib.krk_stream_sync(None))
            idx, vbits = ix.a[:int(c.a[0])].copy(), v.a.copy()
        valid = np.unpackbits(vbits.view(np.uint8), bitorder="little")[:n].astype(bool)
        return idx.astype(np.int64), self._errors(valid)

    def cleanup_scan_plan(self, now_ns, tti_ns, ttl_ns):
        """cleanupManager.scan (lib/store/cleanup.go:112-155) as a plan: (delete_idx int64 ascending,
        usage).  A file is ready for deletion when ttl > 0 and now - mtime > ttl, or when it has a
        last access time and now - atime > tti; usage is the sum of all sizes, the deleted files'
        included, as the reference counts it.  Host only (krk_expiry_bits)."""
        import ctypes as C

        import numpy as np

        from ._capi import check, lib
        n = len(self)
        i64p = C.POINTER(C.c_int64)
        mt = self.mtime_ns if int(ttl_ns) > 0 else None
        bits = np.zeros((n + 63) // 64, dtype=np.uint64)
        check(lib.krk_expiry_bits(mt.ctypes.data_as(i64p) if mt is not None else None,
                                  self.atime_ns.ctypes.data_as(i64p) if self.atime_ns is not None else None, n,
                                  int(now_ns), int(ttl_ns), int(tti_ns),
                                  bits.ctypes.data_as(C.POINTER(C.c_uint64)) if n else None))
        idx = np.flatnonzero(np.unpackbits(bits.view(np.uint8), bitorder="little")[:n]).astype(np.int64)
        usage = int(self.size.sum()) if self.size is not None else 0
        return idx, usage
