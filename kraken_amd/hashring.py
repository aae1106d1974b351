"""Host-side mirror of lib/hashring's owner-list computation over the C ABI.

``Ring.Locations`` follows lib/hashring/ring.go:91-118: the HRW order of the
digest's ShardID (core/digest.go:148-150) over every member (weight 100,
ring.go:28,150-153), then the healthy filter: no healthy node -> [order[0]];
else walk the order while (no location yet or i < MaxReplica), keeping healthy
nodes.  Membership/health monitoring (Monitor, the health filters) is out of scope:
the caller passes the member list and the healthy set.

Locations depends on the digest only through its 2-byte ShardID, so Refresh (the
reference rebuilds its hrw object there, ring.go:141-165) computes all 65,536 owner
lists on the GPU in one call (krk_ring_owner_table) and Locations is a host lookup
-- the binding INTEGRATION.md gives the Go ring.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._capi import check, lib
from .hrw import _NodeTable, RendezvousHash

DEFAULT_WEIGHT = 100  # ring.go:28
DEFAULT_MAX_REPLICA = 3  # lib/hashring/config.go:30-37


class Ring:
    def __init__(self, addrs, healthy=None, max_replica: int = DEFAULT_MAX_REPLICA):
        self.addrs = list(addrs)
        if not self.addrs:
            raise ValueError("ring must be non-empty")
        self.hash = RendezvousHash()
        for a in self.addrs:
            self.hash.AddNode(a, DEFAULT_WEIGHT)
        self.max_replica = int(max_replica)
        self.set_healthy(self.addrs if healthy is None else healthy)

    def set_healthy(self, healthy) -> None:
        hs = set(healthy)
        self._healthy = np.array([1 if a in hs else 0 for a in self.addrs], dtype=np.uint8)
        self._table = None  # rebuilt by the next Refresh / Locations

    def Refresh(self) -> None:
        """The 65,536-row owner table for the current members and healthy set."""
        row = max(1, self.max_replica)
        locs = np.full((65536, row), -1, dtype=np.int32)
        counts = np.zeros(65536, dtype=np.uint8)
        nt = _NodeTable(self.hash.Nodes)
        check(lib.krk_ring_owner_table(C.byref(nt.s), self._healthy.ctypes.data_as(C.POINTER(C.c_uint8)),
                                       self.max_replica, locs.ctypes.data_as(C.POINTER(C.c_int32)),
                                       counts.ctypes.data_as(C.POINTER(C.c_uint8))))
        self._table = (locs, counts)

    def Contains(self, addr: str) -> bool:
        return addr in self.addrs

    def _raw(self, digests32: np.ndarray):
        d = np.ascontiguousarray(digests32, dtype=np.uint8).reshape(-1, 32)
        n = d.shape[0]
        row = max(1, self.max_replica)
        locs = np.full((n, row), -1, dtype=np.int32)
        counts = np.zeros(n, dtype=np.uint8)
        nt = _NodeTable(self.hash.Nodes)
        check(lib.krk_ring_locations(d.ctypes.data_as(C.POINTER(C.c_uint8)), n, C.byref(nt.s),
                                     self._healthy.ctypes.data_as(C.POINTER(C.c_uint8)), self.max_replica,
                                     locs.ctypes.data_as(C.POINTER(C.c_int32)),
                                     counts.ctypes.data_as(C.POINTER(C.c_uint8))))
        return locs, counts

    def Locations(self, d) -> list[str]:
        """ring.Locations (lib/hashring/ring.go:91-118): a lookup of the ShardID's row."""
        if self._table is None:
            self.Refresh()
        locs, counts = self._table
        shard = int(d.ShardID(), 16)
        return [self.addrs[int(j)] for j in locs[shard, : counts[shard]]]

    def LocationsBatch(self, digests32: np.ndarray):
        """Raw 32-byte digests -> (int32 [n, max(1,MaxReplica)] node indices, uint8 [n] counts)."""
        return self._raw(digests32)

    # ------------------------------------------------------------ ownership as bitsets
    # maybeDelete's `owns` (origin/blobserver/server.go:686-759) and applyToReplicas' replica set
    # (426-454) for a whole listing: a 65,536-bit shard mask (uint64 [1024], shard s = bit s & 63 of
    # word s >> 6) built on the host from the owner table, applied to digests by Select.
    def _owner_table(self):
        if self._table is None:
            self.Refresh()
        locs, counts = self._table
        return np.ascontiguousarray(locs, dtype=np.int32), np.ascontiguousarray(counts, dtype=np.uint8)

    def ShardMaskOwns(self, addr: str) -> np.ndarray:
        """mask[s] = addr in Locations(s); all zero for an address the ring does not have."""
        locs, counts = self._owner_table()
        node = self.addrs.index(addr) if addr in self.addrs else -2  # -1 is the rows' padding
        mask = np.zeros(MASK_WORDS, dtype=np.uint64)
        check(lib.krk_ring_mask_owns(locs.ctypes.data_as(_i32p), counts.ctypes.data_as(_u8p), locs.shape[1], node,
                                     mask.ctypes.data_as(_u64p)))
        return mask

    def ShardMaskMoved(self, other: "Ring") -> np.ndarray:
        """mask[s] = set(self.Locations(s)) != set(other.Locations(s)): the shards whose owner set
        changes when the ring goes from self to other (members, health or MaxReplica)."""
        la, ca = self._owner_table()
        lb, cb = other._owner_table()
        at = {a: i for i, a in enumerate(self.addrs)}
        b_to_a = np.array([at.get(a, -1) for a in other.addrs], dtype=np.int32)
        mask = np.zeros(MASK_WORDS, dtype=np.uint64)
        check(lib.krk_ring_mask_moved(la.ctypes.data_as(_i32p), ca.ctypes.data_as(_u8p), la.shape[1],
                                      lb.ctypes.data_as(_i32p), cb.ctypes.data_as(_u8p), lb.shape[1],
                                      b_to_a.ctypes.data_as(_i32p), len(other.addrs), mask.ctypes.data_as(_u64p)))
        return mask

    def OwnsBatch(self, addr: str, digests32) -> np.ndarray:
        """Bit i = addr in Locations(digest i), as uint64 words (bit i & 63 of word i >> 6)."""
        return self.Select(digests32, self.ShardMaskOwns(addr), indices=False)[0]

    @staticmethod
    def Select(digests32, mask, invert=False, or_bits=None, indices=True):
        """sel(i) = (mask[ShardID(d_i)] ^ invert) | or_bits[i] over raw 32-byte digests ->
        (bits: uint64 words, idx: the selected i ascending, or None without `indices`).  The
        device form when a gfx950 device is present, the host form otherwise: the same bits
        either way."""
        from . import device as D
        if D.device_count() > 0:
            return select_dev(digests32, mask, invert, or_bits, indices)
        return select_host(digests32, mask, invert, or_bits, indices)


MASK_WORDS = 1024
_i32p, _u8p, _u64p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)


def select_host(digests32, mask, invert=False, or_bits=None, indices=True):
    """krk_ring_select: the host form (no device), the reference of the kernel."""
    d = np.ascontiguousarray(digests32, dtype=np.uint8).reshape(-1, 32)
    n = d.shape[0]
    mask = np.ascontiguousarray(mask, dtype=np.uint64)
    assert mask.size == MASK_WORDS
    words = int(lib.krk_bitfield_words(n))
    ob = None
    if or_bits is not None:
        ob = np.ascontiguousarray(or_bits, dtype=np.uint64)
        assert ob.size == words
    bits = np.zeros(words, dtype=np.uint64)
    idx = np.empty(n if indices else 0, dtype=np.uint64)
    count = C.c_uint64()
    check(lib.krk_ring_select(d.ctypes.data_as(_u8p) if n else None, n, mask.ctypes.data_as(_u64p), int(bool(invert)),
                              ob.ctypes.data_as(_u64p) if ob is not None and words else None,
                              bits.ctypes.data_as(_u64p) if words else None,
                              idx.ctypes.data_as(_u64p) if idx.size else None, idx.size, C.byref(count)))
    return bits, (idx[:count.value].copy() if indices else None)


def select_dev(digests32, mask, invert=False, or_bits=None, indices=True, n=None):
    """krk_ring_select_dev: digests32 is a host array (uploaded here) or a device.DeviceBuffer
    holding n digests.  The index list is sized by a first call that asks for the count alone."""
    from . import device as D
    if isinstance(digests32, D.DeviceBuffer):
        dev = digests32
        n = dev.nbytes // 32 if n is None else int(n)
    else:
        d = np.ascontiguousarray(digests32, dtype=np.uint8).reshape(-1, 32)
        n = d.shape[0]
        dev = D.DeviceBuffer(32 * n)
        dev.from_host(d)
    mask = np.ascontiguousarray(mask, dtype=np.uint64)
    assert mask.size == MASK_WORDS
    words = int(lib.krk_bitfield_words(n))
    ob = None
    if or_bits is not None and words:
        ob = D.DeviceBuffer(8 * words)
        h = np.ascontiguousarray(or_bits, dtype=np.uint64)
        assert h.size == words
        ob.from_host(h)
    bits = D.PinnedArray((words,), np.uint64)
    count = D.PinnedArray((1,), np.uint64)

    def call(idx_ptr, cap):
        check(lib.krk_ring_select_dev(dev.ptr, n, mask.ctypes.data_as(_u64p), int(bool(invert)),
                                      ob.ptr if ob is not None else None, bits.ptr if words else None, idx_ptr, cap,
                                      count.ptr, None))
        D.synchronize()
        return int(count.a[0])

    c = call(None, 0)
    idx = None
    if indices:
        idx = np.empty(0, dtype=np.uint64)
        if c:
            out = D.PinnedArray((c,), np.uint64)
            call(out.ptr, c)
            idx = out.a.copy()
    return bits.a.copy(), idx

