"""Device-resident batch helpers over the C ABI (used by bench.py and the GPU
parity tests): an HBM arena of synthetic blobs and the batch calls on it."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._capi import (check, krk_blob, krk_file_blob, krk_chunk, krk_launch_rec, krk_nodes, krk_planner_rates,
                    krk_request_torrent, krk_resend_torrent, krk_failed_request, krk_announce_torrent, krk_announce, krk_conn_torrent,
                    krk_conn_lists, krk_conn_transition, krk_conn_incoming, lib)

ALIGN = 256  # every blob starts 256-byte aligned in the arena


class DeviceBuffer:
    def __init__(self, nbytes: int):
        p = C.c_void_p()
        check(lib.krk_dev_alloc(max(int(nbytes), 1), C.byref(p)))
        self.ptr = p.value
        self.nbytes = int(nbytes)

    def free(self):
        if self.ptr:
            lib.krk_dev_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def to_host(self, dtype=np.uint8, count: int | None = None, offset: int = 0) -> np.ndarray:
        it = np.dtype(dtype).itemsize
        n = (self.nbytes - offset) // it if count is None else count
        out = np.empty(n, dtype=dtype)
        if n:
            check(lib.krk_memcpy_d2h(out.ctypes.data, self.ptr + offset, n * it))
        return out

    def zero(self):
        self.from_host(np.zeros(self.nbytes, dtype=np.uint8))

    def from_host(self, a: np.ndarray, offset: int = 0):
        a = np.ascontiguousarray(a)
        if a.nbytes:
            check(lib.krk_memcpy_h2d(self.ptr + offset, a.ctypes.data, a.nbytes))


class PinnedArray:
    """A numpy view of library-allocated pinned host memory (krk_host_alloc):
    device results land here at PCIe rate instead of through a pageable bounce."""

    def __init__(self, shape, dtype, dma_target=False):
        """dma_target: the HIP runtime's allocator (krk_host_alloc_dma: the device's NUMA
        node) for buffers the device copies into."""
        self.array_nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        check((lib.krk_host_alloc_dma if dma_target else lib.krk_host_alloc)(max(self.array_nbytes, 1), C.byref(p)))
        self.ptr = p.value
        buf = (C.c_uint8 * max(self.array_nbytes, 1)).from_address(self.ptr)
        self.a = np.frombuffer(buf, dtype=np.uint8, count=self.array_nbytes).view(dtype).reshape(shape)

    def fill_from(self, dev: "DeviceBuffer", offset: int = 0):
        if self.array_nbytes:
            check(lib.krk_memcpy_d2h(self.ptr, dev.ptr + offset, self.array_nbytes))
        return self.a

    def fill_from_async(self, dev: "DeviceBuffer", stream, offset: int = 0):
        """Queue the copy on `stream`; self.a is valid once that stream is synchronised."""
        if self.array_nbytes:
            check(lib.krk_memcpy_d2h_async(self.ptr, dev.ptr + offset, self.array_nbytes, stream))

    def __del__(self):
        try:
            if self.ptr:
                lib.krk_host_free(self.ptr)
                self.ptr = None
        except Exception:
            pass


def device_count() -> int:
    n = C.c_int()
    check(lib.krk_device_count(C.byref(n)))
    return n.value


def set_device(d: int):
    check(lib.krk_set_device(d))


def init(dev_mask: int = 0):
    """Create device contexts eagerly (krk_init): bit i = device i, 0 = current."""
    check(lib.krk_init(dev_mask))


def shutdown():
    """Free every device context and the pinned staging windows (krk_shutdown).
    No library call may be in flight; later calls re-create contexts lazily."""
    check(lib.krk_shutdown())


def synchronize():
    check(lib.krk_synchronize())


def sha_lanes_per_stream(n_streams: int) -> int:
    """Lanes per SHA-256 stream the library uses for a batch of n_streams (1, 2 or 8)."""
    v = C.c_int(0)
    check(lib.krk_sha_lanes_per_stream(n_streams, C.byref(v)))
    return v.value


SHA_PLAN_NAMES = {1: "1lane", 2: "2lane", 3: "1lane_2pair", 4: "2lane_2pair", 5: "8lane", 6: "8lane_2pair"}


def sha_plan_for(n_streams: int) -> int:
    """KRK_SHA_PLAN_* id the library launches for a batch of n_streams (SHA_PLAN_NAMES)."""
    v = C.c_int(0)
    check(lib.krk_sha_plan_for(n_streams, C.byref(v)))
    return v.value


KRK_BLOB_DTYPE = np.dtype([("data", "<u8"), ("length", "<u8"), ("piece_length", "<i8"), ("sums_offset", "<u8")])
assert KRK_BLOB_DTYPE.itemsize == C.sizeof(krk_blob)


class BlobArena:
    """Blobs laid out back to back in one HBM allocation (each 256 B aligned)."""

    def __init__(self, lengths, piece_length, blob_ids=None, variant: int = 0, fill: bool = True,
                 misalign: int = 0):
        self.lengths = np.asarray(lengths, dtype=np.uint64)
        n = len(self.lengths)
        pls = np.broadcast_to(np.asarray(piece_length, dtype=np.int64), (n,))
        self.piece_lengths = np.array(pls, dtype=np.int64)
        self.blob_ids = np.arange(n, dtype=np.uint64) if blob_ids is None else np.asarray(blob_ids, np.uint64)
        self.offsets = np.zeros(n, dtype=np.uint64)
        o = 0
        for i, L in enumerate(self.lengths):
            self.offsets[i] = o + misalign  # misalign > 0 exercises the unaligned path
            o += (int(L) + misalign + ALIGN - 1) // ALIGN * ALIGN
        self.nbytes = max(o, 1)
        self.buf = DeviceBuffer(self.nbytes)
        self.n_pieces = np.array([lib.krk_num_pieces(int(L), int(p)) for L, p in
                                  zip(self.lengths, self.piece_lengths)], dtype=np.uint64)
        self.sums_off = np.zeros(n, dtype=np.uint64)
        if n:
            self.sums_off[1:] = np.cumsum(self.n_pieces)[:-1]
        self.total_pieces = int(self.n_pieces.sum())
        if fill:
            for i in range(n):
                self.fill(i, variant)
            synchronize()

    def fill(self, i: int, variant: int = 0):
        check(lib.krk_synth_fill_dev(self.buf.ptr + int(self.offsets[i]), int(self.blob_ids[i]), 0,
                                     int(self.lengths[i]), variant, None))

    def put(self, i: int, data: np.ndarray):
        self.buf.from_host(np.asarray(data, dtype=np.uint8), int(self.offsets[i]))

    def blob_structs(self):
        """krk_blob[] of the arena, built once (column-wise) and cached: the layout
        never changes after construction."""
        arr = getattr(self, "_structs", None)
        if arr is None:
            n = len(self.lengths)
            a = np.zeros(max(n, 1), dtype=KRK_BLOB_DTYPE)
            a["data"][:n] = np.uint64(self.buf.ptr) + self.offsets
            a["length"][:n], a["piece_length"][:n], a["sums_offset"][:n] = \
                self.lengths, self.piece_lengths, self.sums_off
            arr = (krk_blob * max(n, 1)).from_buffer_copy(a.tobytes())
            self._structs = arr
        return arr

    def data_ptrs(self):
        n = len(self.lengths)
        ptrs = (C.c_void_p * max(n, 1))(*[self.buf.ptr + int(o) for o in self.offsets])
        lens = np.ascontiguousarray(self.lengths, dtype=np.uint64)
        return ptrs, lens


class BatchOutputs:
    def __init__(self, arena: BlobArena):
        self.sums = DeviceBuffer(max(arena.total_pieces, 1) * 4)
        self.digests = DeviceBuffer(max(len(arena.lengths), 1) * 32)


def piece_sums(arena: BlobArena, out: BatchOutputs, stream=None):
    check(lib.krk_piece_sums_dev(arena.blob_structs(), len(arena.lengths), out.sums.ptr, stream))


def pack_names(names):
    """The (bytes, offsets) layout krk_metainfo_batch_dev takes for the blobs' names."""
    enc = [x.encode() for x in names]
    noff = np.zeros(len(enc) + 1, dtype=np.uint64)
    noff[1:] = np.cumsum([len(e) for e in enc]) if enc else []
    return b"".join(enc), noff


def metainfo_batch(arena: BlobArena, out: BatchOutputs, names, sums_host: np.ndarray, stream=None) -> np.ndarray:
    """Generator.Generate over the arena's blobs (krk_metainfo_batch_dev): piece sums into
    out.sums and sums_host (uint32, arena layout) and the InfoHashes, returned as an
    (n, 20) uint8 array; the host hashes each group while later groups' kernels run, or the
    device kernel does under set_info_hash_placement(KRK_PLACE_GPU).
    names: the blobs' names (str), or pack_names() of them."""
    n = len(arena.lengths)
    buf, noff = names if isinstance(names, tuple) else pack_names(names)
    if noff.size != n + 1:
        raise ValueError(f"metainfo_batch: {noff.size - 1} names for {n} blobs")
    ih = np.zeros((max(n, 1), 20), dtype=np.uint8)
    assert sums_host.dtype == np.uint32 and sums_host.size >= arena.total_pieces
    check(lib.krk_metainfo_batch_dev(arena.blob_structs(), n, buf or None,
                                     noff.ctypes.data_as(C.POINTER(C.c_uint64)), out.sums.ptr,
                                     sums_host.ctypes.data_as(C.POINTER(C.c_uint32)),
                                     ih.ctypes.data_as(C.POINTER(C.c_uint8)), stream))
    return ih[:n]


def info_hash_batch_dev(piece_lengths, sums: DeviceBuffer, sums_off, n_sums, names, lengths, out=None, stream=None):
    """krk_info_hash_batch_dev: the InfoHashes of n blobs from piece sums in device memory
    (`sums`, uint32; blob i's at sums_off[i] .. + n_sums[i]), computed by the device kernel.
    names: the blobs' names (str), pack_names() of them, or None when every name is empty.
    out: a DeviceBuffer or PinnedArray of 20 n bytes to fill, asynchronously on `stream` (it is
    returned); None: an (n, 20) uint8 array, returned once the stream has run the call."""
    pl = np.ascontiguousarray(piece_lengths, dtype=np.int64)
    n = pl.size
    so = np.ascontiguousarray(sums_off, dtype=np.uint64)
    ns = np.ascontiguousarray(n_sums, dtype=np.uint64)
    ln = np.ascontiguousarray(lengths, dtype=np.int64)
    if not (so.size == ns.size == ln.size == n):
        raise ValueError("info_hash_batch_dev: the per-blob arrays differ in length")
    if names is None:
        buf, noff = b"", np.zeros(n + 1, dtype=np.uint64)
    else:
        buf, noff = names if isinstance(names, tuple) else pack_names(names)
    if noff.size != n + 1:
        raise ValueError(f"info_hash_batch_dev: {noff.size - 1} names for {n} blobs")
    dst = PinnedArray((max(n, 1), 20), np.uint8) if out is None else out
    i64p, u64p = C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
    check(lib.krk_info_hash_batch_dev(pl.ctypes.data_as(i64p), sums.ptr, so.ctypes.data_as(u64p),
                                      ns.ctypes.data_as(u64p), buf or None, noff.ctypes.data_as(u64p),
                                      ln.ctypes.data_as(i64p), n, dst.ptr, stream))
    if out is not None:
        return out
    check(lib.krk_stream_sync(stream))
    return dst.a[:n].copy()


def set_info_hash_placement(placement: int):
    """krk_set_info_hash_placement: where metainfo_batch computes its InfoHashes, process-wide
    (KRK_PLACE_AUTO = HOST for now, KRK_PLACE_HOST, KRK_PLACE_GPU)."""
    check(lib.krk_set_info_hash_placement(int(placement)))


def info_hash_placement() -> int:
    v = C.c_int(-1)
    check(lib.krk_info_hash_placement(C.byref(v)))
    return v.value


def metainfo_batch_last_placement() -> int:
    """Where this thread's last metainfo_batch computed its InfoHashes (KRK_PLACE_HOST / _GPU)."""
    v = C.c_int(-1)
    check(lib.krk_metainfo_batch_last_placement(C.byref(v)))
    return v.value


def sha256(arena: BlobArena, out: BatchOutputs, stream=None):
    ptrs, lens = arena.data_ptrs()
    check(lib.krk_sha256_dev(ptrs, lens.ctypes.data_as(C.POINTER(C.c_uint64)), len(arena.lengths),
                             out.digests.ptr, stream))


def sha256_dev_on_host(ptrs, lens, threads: int = 0, stream=None) -> np.ndarray:
    """krk_sha256_dev_on_host: device blobs (numpy device addresses + lengths) hashed by
    up to `threads` host threads after `stream`'s queued work; (n, 32) uint8 digests."""
    n = len(ptrs)
    p = np.ascontiguousarray(ptrs, dtype=np.uint64)
    ln = np.ascontiguousarray(lens, dtype=np.uint64)
    out = np.zeros((max(n, 1), 32), dtype=np.uint8)
    check(lib.krk_sha256_dev_on_host(p.ctypes.data_as(C.POINTER(C.c_void_p)), ln.ctypes.data_as(C.POINTER(C.c_uint64)),
                                     n, int(threads), stream, out.ctypes.data_as(C.POINTER(C.c_uint8))))
    return out[:n]


def piece_sums_dev_arrays(ptrs, lens, piece_lengths, sums_offsets, sums_dev_ptr: int, stream=None):
    """krk_piece_sums_dev over blobs given column-wise (device addresses, lengths, piece
    lengths, offsets of their sums in the sums buffer at sums_dev_ptr)."""
    n = len(ptrs)
    a = np.zeros(max(n, 1), dtype=KRK_BLOB_DTYPE)
    a["data"][:n], a["length"][:n] = ptrs, lens
    a["piece_length"][:n], a["sums_offset"][:n] = piece_lengths, sums_offsets
    check(lib.krk_piece_sums_dev(a.ctypes.data_as(C.POINTER(krk_blob)), n, sums_dev_ptr, stream))


def metainfo_digest(arena: BlobArena, out: BatchOutputs, stream=None):
    check(lib.krk_metainfo_digest_dev(arena.blob_structs(), len(arena.lengths), out.sums.ptr,
                                      out.digests.ptr, stream))


def set_sha_host_offload(threads: int):
    """krk_set_sha_host_offload: up to `threads` host threads take the longest SHA-256
    chains of sha256 / metainfo_digest batches (0 = off; -1 = AUTO, the default: the
    planner-gated offload on the process's CPU budget)."""
    check(lib.krk_set_sha_host_offload(int(threads)))


OFFLOAD_DEVICE, OFFLOAD_HOST_SHA, OFFLOAD_HOST_WHOLE, OFFLOAD_HOST_FILES = 0, 1, 2, 3


def piece_sums_host(datas, piece_length: int):
    """krk_piece_sums_host over host buffers (numpy uint8 arrays or bytes): each one's
    piece sums (calcPieceSums), split between host threads and the GPU by the planner."""
    arrs = [np.frombuffer(d, dtype=np.uint8) if isinstance(d, (bytes, bytearray)) else d for d in datas]
    n = len(arrs)
    blobs = (krk_blob * max(n, 1))()
    off = 0
    counts = []
    for i, a in enumerate(arrs):
        cnt = int(lib.krk_num_pieces(int(a.size), int(piece_length)))
        blobs[i] = krk_blob(a.ctypes.data if a.size else None, int(a.size), int(piece_length), off)
        counts.append(cnt)
        off += cnt
    sums = np.zeros(max(off, 1), dtype=np.uint32)
    check(lib.krk_piece_sums_host(blobs, n, sums.ctypes.data_as(C.POINTER(C.c_uint32))))
    out, o = [], 0
    for c in counts:
        out.append(sums[o:o + c].copy())
        o += c
    return out


def crc_host_split():
    """(GPU bytes, host bytes) of this thread's last krk_piece_sums_host / verify call and
    the GPU share the next pinned batch will use (-1 until learned)."""
    g, h, f = C.c_uint64(), C.c_uint64(), C.c_double()
    check(lib.krk_crc_host_split(C.byref(g), C.byref(h), C.byref(f)))
    return g.value, h.value, f.value


RATES_SOURCE = {0: "nominal", 1: "measured", 2: "set"}


def planner_rates() -> dict:
    """krk_planner_rates_get: the rates the planners use on this thread's device
    (measured there at first use; nominal without a device; or what was set)."""
    r = krk_planner_rates()
    check(lib.krk_planner_rates_get(C.byref(r)))
    return {"sha_stream_bps": list(r.sha_stream_bps), "d2h_bps": r.d2h_bps, "h2d_bps": r.h2d_bps,
            "host_sha_bps": r.host_sha_bps, "host_crc_bps": r.host_crc_bps, "host_copy_bps": r.host_copy_bps,
            "cus": r.cus,
            "source": RATES_SOURCE.get(r.source, r.source)}


def set_planner_rates(rates: dict | None):
    """krk_planner_rates_set (None: back to the measured / nominal rates)."""
    if rates is None:
        check(lib.krk_planner_rates_set(None))
        return
    r = krk_planner_rates()
    for k, v in enumerate(rates["sha_stream_bps"]):
        r.sha_stream_bps[k] = v
    r.d2h_bps, r.h2d_bps = rates["d2h_bps"], rates["h2d_bps"]
    r.host_sha_bps, r.host_crc_bps = rates["host_sha_bps"], rates["host_crc_bps"]
    r.host_copy_bps = rates["host_copy_bps"]
    r.cus = rates["cus"]
    check(lib.krk_planner_rates_set(C.byref(r)))


def sha_tail_plan(lengths, threads: int):
    """krk_sha_tail_plan: (chain indices whose tails host threads finish, the GPU's prefix
    bytes of each, planned end seconds, GPU-alone seconds) -- planner_rates(), no device."""
    L = np.ascontiguousarray(lengths, dtype=np.uint64)
    idx = np.zeros(max(L.size, 1), dtype=np.uint32)
    st = np.zeros(max(L.size, 1), dtype=np.uint64)
    k, e, g = C.c_uint64(0), C.c_double(0), C.c_double(0)
    check(lib.krk_sha_tail_plan(L.ctypes.data_as(C.POINTER(C.c_uint64)), L.size, int(threads),
                                idx.ctypes.data_as(C.POINTER(C.c_uint32)), st.ctypes.data_as(C.POINTER(C.c_uint64)),
                                C.byref(k), C.byref(e), C.byref(g)))
    return idx[:k.value].copy(), st[:k.value].copy(), e.value, g.value


def sha_last_tail() -> dict:
    """krk_sha_last_tail: the calling thread's last device-resident SHA-256 batch's tail
    handoff (chains finished on host threads from the GPU's midstate, the GPU's prefix bytes)."""
    c, b = C.c_uint64(0), C.c_uint64(0)
    check(lib.krk_sha_last_tail(C.byref(c), C.byref(b)))
    return {"chains": c.value, "gpu_prefix_bytes": b.value}


def sha_offload_plan(lengths, threads: int, cus: int = 0, mode: int = OFFLOAD_DEVICE):
    """krk_host_offload_plan: (indices of the blobs the host would take, longest first,
    modelled GPU seconds, modelled host seconds) -- no device work (planner_rates(); cus
    > 0 overrides their CU count).  mode: a batch in
    HBM (OFFLOAD_DEVICE), host blobs hashed only (OFFLOAD_HOST_SHA, sha256_host) or hashed
    and piece-summed on the host (OFFLOAD_HOST_WHOLE, metainfo_digest_host)."""
    L = np.ascontiguousarray(lengths, dtype=np.uint64)
    idx = np.zeros(max(L.size, 1), dtype=np.uint32)
    k, g, h = C.c_uint64(0), C.c_double(0), C.c_double(0)
    check(lib.krk_host_offload_plan(L.ctypes.data_as(C.POINTER(C.c_uint64)), L.size, int(threads), int(cus),
                                    int(mode), idx.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(k), C.byref(g),
                                    C.byref(h)))
    return idx[:k.value].copy(), g.value, h.value


def set_devices(devs):
    """The process's device set (krk_set_devices): where the *_multi calls run and new
    Digesters / piece streams are placed; repeats allowed; [] = the calling thread's device."""
    arr = (C.c_int * max(len(devs), 1))(*devs)
    check(lib.krk_set_devices(arr, len(devs)))


def get_devices():
    n = C.c_uint32()
    check(lib.krk_get_devices(None, 0, C.byref(n)))
    arr = (C.c_int * max(n.value, 1))()
    check(lib.krk_get_devices(arr, n.value, C.byref(n)))
    return list(arr[:n.value])


def metainfo_digest_host(datas, piece_lengths, multi: bool = False):
    """End-to-end batch over HOST buffers (numpy uint8 arrays, pageable or
    pinned): one PCIe pass feeds both kernels.  Returns (sums per blob, digests).
    multi: krk_metainfo_digest_host_multi (LPT over the device set)."""
    n = len(datas)
    pls = np.broadcast_to(np.asarray(piece_lengths, dtype=np.int64), (n,))
    counts = [int(lib.krk_num_pieces(int(d.size), int(p))) for d, p in zip(datas, pls)]
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(counts) if n else []
    arr = (krk_blob * max(n, 1))()
    for i, d in enumerate(datas):
        arr[i] = krk_blob(d.ctypes.data if d.size else None, int(d.size), int(pls[i]), int(offs[i]))
    sums = np.zeros(max(int(offs[-1]), 1), dtype=np.uint32)
    dg = np.zeros((max(n, 1), 32), dtype=np.uint8)
    fn = lib.krk_metainfo_digest_host_multi if multi else lib.krk_metainfo_digest_host
    check(fn(arr, n, sums.ctypes.data_as(C.POINTER(C.c_uint32)), dg.ctypes.data_as(C.POINTER(C.c_uint8))))
    return [sums[int(offs[i]):int(offs[i + 1])] for i in range(n)], dg[:n]


def metainfo_digest_files(paths, lengths, piece_lengths, multi: bool = False):
    """krk_metainfo_digest_files: the digests and piece sums of CAS files, each read once
    (pinned windows -> both kernels; the planner's files on host threads).  lengths: the
    sizes the caller stat-ed.  Returns (sums per file, digests).  multi: the _multi form
    (LPT over the device set)."""
    n = len(paths)
    L = np.asarray(lengths, dtype=np.uint64)
    pls = np.broadcast_to(np.asarray(piece_lengths, dtype=np.int64), (n,))
    counts = [int(lib.krk_num_pieces(int(l), int(p))) for l, p in zip(L, pls)]
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(counts) if n else []
    enc = [p.encode() if isinstance(p, str) else bytes(p) for p in paths]
    arr = (krk_file_blob * max(n, 1))()
    for i in range(n):
        arr[i] = krk_file_blob(enc[i], int(L[i]), int(pls[i]), int(offs[i]))
    sums = np.zeros(max(int(offs[-1]), 1), dtype=np.uint32)
    dg = np.zeros((max(n, 1), 32), dtype=np.uint8)
    fn = lib.krk_metainfo_digest_files_multi if multi else lib.krk_metainfo_digest_files
    check(fn(arr, n, sums.ctypes.data_as(C.POINTER(C.c_uint32)), dg.ctypes.data_as(C.POINTER(C.c_uint8))))
    return [sums[int(offs[i]):int(offs[i + 1])] for i in range(n)], dg[:n]


def piece_sums_files(paths, lengths, piece_lengths, multi: bool = False):
    """krk_piece_sums_files: the piece sums of CAS files (Generate over cache files), on the
    CRC placement (krk_set_crc_placement; AUTO = the measured crossover).  Returns the sums
    per file as one array (offsets from the counts) and the per-file views."""
    n = len(paths)
    L = np.asarray(lengths, dtype=np.uint64)
    pls = np.broadcast_to(np.asarray(piece_lengths, dtype=np.int64), (n,))
    counts = [int(lib.krk_num_pieces(int(l), int(p))) for l, p in zip(L, pls)]
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(counts) if n else []
    enc = [p.encode() if isinstance(p, str) else bytes(p) for p in paths]
    arr = (krk_file_blob * max(n, 1))()
    for i in range(n):
        arr[i] = krk_file_blob(enc[i], int(L[i]), int(pls[i]), int(offs[i]))
    sums = np.zeros(max(int(offs[-1]), 1), dtype=np.uint32)
    fn = lib.krk_piece_sums_files_multi if multi else lib.krk_piece_sums_files
    check(fn(arr, n, sums.ctypes.data_as(C.POINTER(C.c_uint32))))
    return sums, offs


def bitfield_offsets(n_pieces) -> np.ndarray:
    """First bitfield word of each blob of a verify batch, and the total as the last entry:
    blob i's krk_bitfield_words(n_pieces[i]) words follow blob i-1's."""
    words = (np.asarray(n_pieces, dtype=np.uint64) + np.uint64(63)) // np.uint64(64)
    offs = np.zeros(words.size + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(words)
    return offs


def bitfield_bools(words: np.ndarray, n_pieces: int) -> np.ndarray:
    """A blob's bitfield words (willf/bitset: piece i = bit i & 63 of word i >> 6) as bools."""
    w = np.ascontiguousarray(words, dtype="<u8")
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:int(n_pieces)].astype(bool)


def piece_bitfield(sums, expected):
    """krk_piece_bitfield: (bitfield words, mismatching pieces) of one blob from sums on the
    host -- pure host code, the same bits the device kernel gives."""
    s = np.ascontiguousarray(sums, dtype=np.uint32)
    e = np.ascontiguousarray(expected, dtype=np.uint32)
    if s.size != e.size:
        raise ValueError(f"piece_bitfield: {s.size} sums against {e.size} expected")
    bits = np.zeros(int(lib.krk_bitfield_words(s.size)), dtype=np.uint64)
    bad = C.c_uint32()
    u32p = C.POINTER(C.c_uint32)
    check(lib.krk_piece_bitfield(s.ctypes.data_as(u32p) if s.size else None, e.ctypes.data_as(u32p) if s.size else None,
                                 s.size, bits.ctypes.data_as(C.POINTER(C.c_uint64)) if bits.size else None,
                                 C.byref(bad)))
    return bits, bad.value


class VerifyOutputs:
    """The outputs of verify_batch over an arena, in device memory or (pinned=True) in
    page-locked host memory the kernels write over PCIe: .bits (uint64, bitfield_offsets
    layout), .n_bad (uint32 a blob), .digest_ok (uint8 a blob; only with digests)."""

    def __init__(self, arena: BlobArena, digests: bool = False, pinned: bool = False):
        n = len(arena.lengths)
        self.word_off = bitfield_offsets(arena.n_pieces)
        self.n, self.words, self.pinned = n, int(self.word_off[-1]), pinned
        if pinned:
            self.bits = PinnedArray((max(self.words, 1),), np.uint64)
            self.n_bad = PinnedArray((max(n, 1),), np.uint32)
            self.digest_ok = PinnedArray((max(n, 1),), np.uint8) if digests else None
        else:
            self.bits = DeviceBuffer(max(self.words, 1) * 8)
            self.n_bad = DeviceBuffer(max(n, 1) * 4)
            self.digest_ok = DeviceBuffer(max(n, 1)) if digests else None

    def fill(self, byte: int):
        """Every output byte set to `byte` (tests: the call must overwrite all of it)."""
        for b, dt in ((self.bits, np.uint64), (self.n_bad, np.uint32), (self.digest_ok, np.uint8)):
            if b is None:
                continue
            if self.pinned:
                b.a.view(np.uint8)[:] = byte
            else:
                b.from_host(np.full(b.nbytes, byte, dtype=np.uint8))

    def to_host(self):
        """(bits, n_bad, digest_ok or None) as numpy arrays, once the call's stream has run."""
        def get(b, dt, k):
            if b is None:
                return None
            return b.a[:k].copy() if self.pinned else b.to_host(dt, k)
        ok = get(self.digest_ok, np.uint8, self.n)
        return get(self.bits, np.uint64, self.words), get(self.n_bad, np.uint32, self.n), \
            (None if ok is None else ok.astype(bool))


def verify_batch(arena: BlobArena, expected, digests=None, out: VerifyOutputs | None = None, stream=None):
    """krk_verify_batch_dev: the arena's blobs against the piece sums their metainfo stores
    (`expected`, uint32, arena layout: blob i's at arena.sums_off[i]) and, with `digests`
    ((n, 32) uint8: the blobs' names), their SHA-256.  One wave ballots 64 pieces of a blob into
    one willf/bitset word.  out: VerifyOutputs to fill asynchronously on `stream` (returned);
    None: (bits, n_bad, digest_ok or None), returned once the stream has run the call."""
    n = len(arena.lengths)
    exp = np.ascontiguousarray(expected, dtype=np.uint32)
    if exp.size < arena.total_pieces:
        raise ValueError(f"verify_batch: {exp.size} expected sums for {arena.total_pieces} pieces")
    dg = None
    if digests is not None:
        dg = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1)
        if dg.size != 32 * n:
            raise ValueError(f"verify_batch: {dg.size} digest bytes for {n} blobs")
    dst = VerifyOutputs(arena, digests=dg is not None, pinned=True) if out is None else out
    check(lib.krk_verify_batch_dev(arena.blob_structs(), n, exp.ctypes.data_as(C.POINTER(C.c_uint32)) if exp.size else None,
                                   dg.ctypes.data_as(C.POINTER(C.c_uint8)) if dg is not None else None,
                                   dst.bits.ptr, dst.n_bad.ptr, dst.digest_ok.ptr if dst.digest_ok is not None else None,
                                   stream))
    if out is not None:
        return out
    check(lib.krk_stream_sync(stream))
    return dst.to_host()


def verify_files(paths, lengths, piece_lengths, expected, digests=None):
    """krk_verify_files: cache or download files against the piece sums their metainfo stores
    (`expected`: uint32, file i's sums after file i-1's) and, with `digests` ((n, 32) uint8),
    their SHA-256 -- krk_piece_sums_files underneath (the CRC placement rule; HOST needs no
    device), or krk_metainfo_digest_files with digests (one read a byte feeds both).  lengths:
    the sizes the caller stat-ed.  Returns (bits, word offsets (bitfield_offsets), n_bad,
    digest_ok or None)."""
    n = len(paths)
    L = np.asarray(lengths, dtype=np.uint64)
    pls = np.broadcast_to(np.asarray(piece_lengths, dtype=np.int64), (n,))
    counts = [int(lib.krk_num_pieces(int(l), int(p))) if p > 0 else 0 for l, p in zip(L, pls)]
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(counts) if n else []
    exp = np.ascontiguousarray(expected, dtype=np.uint32)
    if exp.size < int(offs[-1]):
        raise ValueError(f"verify_files: {exp.size} expected sums for {int(offs[-1])} pieces")
    dg = None
    if digests is not None:
        dg = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1)
        if dg.size != 32 * n:
            raise ValueError(f"verify_files: {dg.size} digest bytes for {n} files")
    enc = [os.fsencode(p) for p in paths]
    arr = (krk_file_blob * max(n, 1))()
    for i in range(n):
        arr[i] = krk_file_blob(enc[i], int(L[i]), int(pls[i]), int(offs[i]))
    woff = bitfield_offsets(counts)
    bits = np.zeros(max(int(woff[-1]), 1), dtype=np.uint64)
    bad = np.zeros(max(n, 1), dtype=np.uint32)
    ok = np.zeros(max(n, 1), dtype=np.uint8) if dg is not None else None
    u8p = C.POINTER(C.c_uint8)
    check(lib.krk_verify_files(arr, n, exp.ctypes.data_as(C.POINTER(C.c_uint32)) if exp.size else None,
                               dg.ctypes.data_as(u8p) if dg is not None else None,
                               bits.ctypes.data_as(C.POINTER(C.c_uint64)), bad.ctypes.data_as(C.POINTER(C.c_uint32)),
                               ok.ctypes.data_as(u8p) if ok is not None else None))
    return bits[:int(woff[-1])], woff, bad[:n], (ok[:n].astype(bool) if ok is not None else None)


PLACE_AUTO, PLACE_HOST, PLACE_GPU = 0, 1, 2


def set_crc_placement(placement: int):
    """krk_set_crc_placement: the process-wide placement of CRC-only host calls."""
    check(lib.krk_set_crc_placement(int(placement)))


def windows_last_call() -> dict:
    """The calling thread's last krk_metainfo_digest_host / _files call: the most live blobs
    in a window, the windows, the blobs the host offload took (krk_windows_last_call)."""
    m, w, h, d = C.c_uint64(), C.c_int(), C.c_uint64(), C.c_int()
    g, rb, rs = C.c_int(), C.c_uint64(), C.c_double()
    check(lib.krk_windows_last_call(C.byref(m), C.byref(w), C.byref(h)))
    check(lib.krk_windows_last_direct(C.byref(d)))
    check(lib.krk_windows_last_gather(C.byref(g), C.byref(rb), C.byref(rs)))
    ph = [C.c_double() for _ in range(5)]
    dr = C.c_int()
    check(lib.krk_windows_last_phases(*[C.byref(x) for x in ph], C.byref(dr)))
    lc = C.c_uint64()
    check(lib.krk_windows_last_copyout(C.byref(lc)))
    return {"live_registered_at_copyout": lc.value, "max_live": m.value, "windows": w.value, "host_blobs": h.value, "direct_windows": d.value,
            "gather_windows": g.value, "registered_bytes": rb.value, "register_s": rs.value,
            "phases_s": dict(zip(("loop", "acquire", "fill", "enqueue"), (round(x.value, 4) for x in ph[:4]))),
            "resident_sample": round(ph[4].value, 4), "direct_reads": bool(dr.value)}


def set_host_gather(mode: int):
    """krk_set_host_gather: -1 AUTO (default), 0 stage every window, 1 gather any size."""
    check(lib.krk_set_host_gather(int(mode)))


def device_pci_bus_id() -> str:
    b = C.create_string_buffer(64)
    check(lib.krk_device_pci_bus_id(b, 64))
    return b.value.decode()


def device_cus() -> int:
    v = C.c_int(0)
    check(lib.krk_device_cus(C.byref(v)))
    return v.value


def window_stream_cap() -> int:
    v = C.c_uint64(0)
    check(lib.krk_window_stream_cap(C.byref(v)))
    return v.value


class ChunkedBatch:
    """Window-by-window metainfo+digest over device chunks (krk_metainfo_digest_chunks_dev):
    per-blob SHA midstates and XOR-accumulated piece sums live on the device between steps."""

    def __init__(self, lengths, piece_lengths):
        self.lengths = np.asarray(lengths, dtype=np.uint64)
        n = len(self.lengths)
        self.piece_lengths = np.array(np.broadcast_to(np.asarray(piece_lengths, dtype=np.int64), (n,)))
        self.n_pieces = np.array([lib.krk_num_pieces(int(L), int(p)) for L, p in
                                  zip(self.lengths, self.piece_lengths)], dtype=np.uint64)
        self.sums_off = np.zeros(n, dtype=np.uint64)
        if n:
            self.sums_off[1:] = np.cumsum(self.n_pieces)[:-1]
        self.total_pieces = int(self.n_pieces.sum())
        self.state = DeviceBuffer(max(n, 1) * 32)
        self.sums = DeviceBuffer(max(self.total_pieces, 1) * 4)
        self.sums.zero()
        self.digests = DeviceBuffer(max(n, 1) * 32)

    def step_arrays(self, blob_idx, ptrs, offsets, lengths, stream=None, sha_stream=None, crc_after_sha=False):
        """step() from numpy arrays (one window of thousands of chunks, no Python loop);
        sha_stream: the SHA-256 launch's stream (krk_metainfo_digest_chunks_dev_on);
        crc_after_sha: the CRCs on `stream` once that launch has ended (_after)."""
        arr = chunk_array(ptrs, offsets, lengths, self.lengths[blob_idx], self.piece_lengths[blob_idx],
                          self.sums_off[blob_idx], blob_idx)
        fn = lib.krk_metainfo_digest_chunks_dev_after if crc_after_sha else lib.krk_metainfo_digest_chunks_dev_on
        check(fn(arr.ctypes.data_as(C.POINTER(krk_chunk)), len(arr), self.state.ptr, self.sums.ptr, self.digests.ptr,
                 stream, sha_stream))

    def step(self, items, stream=None):
        """items: [(blob index, device address of the chunk, offset, length)]."""
        arr = (krk_chunk * max(len(items), 1))()
        for k, (i, ptr, off, ln) in enumerate(items):
            arr[k] = krk_chunk(ptr, int(off), int(ln), int(self.lengths[i]), int(self.piece_lengths[i]),
                               int(self.sums_off[i]), int(i))
        check(lib.krk_metainfo_digest_chunks_dev(arr, len(items), self.state.ptr, self.sums.ptr,
                                                 self.digests.ptr, stream))


KRK_CHUNK_DTYPE = np.dtype([("data", "<u8"), ("offset", "<u8"), ("length", "<u8"), ("blob_length", "<u8"),
                            ("piece_length", "<i8"), ("sums_offset", "<u8"), ("blob", "<u8")])
assert KRK_CHUNK_DTYPE.itemsize == C.sizeof(krk_chunk)


def chunk_array(ptrs, offsets, lengths, blob_lengths, piece_lengths, sums_offsets, blobs) -> np.ndarray:
    """A krk_chunk[] built column-wise with numpy."""
    n = len(ptrs)
    arr = np.zeros(max(n, 1), dtype=KRK_CHUNK_DTYPE)[:n]
    arr["data"], arr["offset"], arr["length"] = ptrs, offsets, lengths
    arr["blob_length"], arr["piece_length"] = blob_lengths, piece_lengths
    arr["sums_offset"], arr["blob"] = sums_offsets, blobs
    return arr


def synth_fill_chunk_arrays(blob_ids, ptrs, offsets, lengths, variant: int = 0, stream=None):
    """synth_fill_chunks from numpy arrays."""
    n = len(ptrs)
    arr = chunk_array(ptrs, offsets, lengths, 0, 1, 0, blob_ids)
    check(lib.krk_synth_fill_chunks_dev(arr.ctypes.data_as(C.POINTER(krk_chunk)), n, variant, stream))


def synth_fill_chunks(items, variant: int = 0, stream=None):
    """items: [(blob id, device address, offset, length)] -> bytes [offset, offset+length)
    of each synthetic blob written at its address, one launch."""
    arr = (krk_chunk * max(len(items), 1))()
    for k, (b, ptr, off, ln) in enumerate(items):
        arr[k] = krk_chunk(ptr, int(off), int(ln), 0, 1, 0, int(b))
    check(lib.krk_synth_fill_chunks_dev(arr, len(items), variant, stream))


_NODES_CACHE: dict = {}


def nodes_struct(labels, weights):
    """krk_nodes for (labels, weights), kept per membership (the last 16) so a placement
    call per batch does not re-encode the ring."""
    key = (tuple(labels), tuple(int(w) for w in weights))
    hit = _NODES_CACHE.get(key)
    if hit is not None:
        return hit
    if len(_NODES_CACHE) >= 16:
        _NODES_CACHE.pop(next(iter(_NODES_CACHE)))
    _NODES_CACHE[key] = hit = _nodes_struct(labels, weights)
    return hit


def _nodes_struct(labels, weights):
    enc = [s.encode() for s in labels]
    blob = b"".join(enc)
    off = np.zeros(len(enc) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(e) for e in enc])
    w = np.ascontiguousarray(weights, dtype=np.int64)
    s = krk_nodes(blob, off.ctypes.data_as(C.POINTER(C.c_uint64)), w.ctypes.data_as(C.POINTER(C.c_int64)),
                  len(labels))
    return s, (blob, off, w)  # keep the backing arrays alive


def ring_locations_dev(digests_dev: DeviceBuffer, n: int, labels, healthy, max_replica: int,
                       locs_dev: DeviceBuffer, counts_dev: DeviceBuffer, stream=None, weights=None):
    """ring.Locations for n device-resident digests; weights default to the ring's 100
    (lib/hashring/ring.go:28)."""
    s, keep = nodes_struct(labels, [100] * len(labels) if weights is None else weights)
    h = np.ascontiguousarray(healthy, dtype=np.uint8)
    check(lib.krk_ring_locations_dev(digests_dev.ptr, n, C.byref(s), h.ctypes.data_as(C.POINTER(C.c_uint8)),
                                      max_replica, locs_dev.ptr, counts_dev.ptr, stream))
    del keep


def ring_locations_u8_dev(digests_dev: DeviceBuffer, n: int, labels, healthy, max_replica: int,
                          locs_dev: DeviceBuffer, counts_dev: DeviceBuffer, stream=None, weights=None):
    """ring_locations_dev with uint8 owner indices (0xFF padded) for rings of <= 255 nodes:
    a quarter of the owner-list bytes to copy back (krk_ring_locations_u8_dev)."""
    s, keep = nodes_struct(labels, [100] * len(labels) if weights is None else weights)
    h = np.ascontiguousarray(healthy, dtype=np.uint8)
    check(lib.krk_ring_locations_u8_dev(digests_dev.ptr, n, C.byref(s), h.ctypes.data_as(C.POINTER(C.c_uint8)),
                                         max_replica, locs_dev.ptr, counts_dev.ptr, stream))
    del keep


# ------------------------------------------------------------------ piece request rounds
PR_MAX_LIMIT, PR_RAREST_FIRST, PR_SAMPLE, PR_ALLOW_DUPLICATES, PR_NONE = 16, 0, 1, 0x100, 0xFFFFFFFF


class RequestBatch:
    """The layout of one request round over a batch of torrents, packed back to back: torrent t's
    rows (have, then (bits_p, blocked_p) a peer, krk_bitfield_words(n_pieces) words each) start at
    word .bits_off[t], its peers at .peer_off[t], its counts at .piece_off[t]; .structs is the
    krk_request_torrent array the round calls take."""

    def __init__(self, n_pieces, n_peers, flags=PR_RAREST_FIRST, seeds=0):
        n = np.asarray(n_pieces, dtype=np.uint64).reshape(-1)
        k = n.size
        self.n_pieces = n
        self.n_peers = np.broadcast_to(np.asarray(n_peers, dtype=np.uint32), (k,)).copy()
        self.flags = np.broadcast_to(np.asarray(flags, dtype=np.uint32), (k,)).copy()
        self.seeds = np.broadcast_to(np.asarray(seeds, dtype=np.uint64), (k,)).copy()
        self.words = (n + np.uint64(63)) // np.uint64(64)
        rows = self.words * (np.uint64(1) + np.uint64(2) * self.n_peers.astype(np.uint64))
        self.bits_off, self.peer_off, self.piece_off = (np.zeros(k + 1, dtype=np.uint64) for _ in range(3))
        self.bits_off[1:], self.peer_off[1:], self.piece_off[1:] = np.cumsum(rows), np.cumsum(self.n_peers), np.cumsum(n)
        self.total_words, self.total_peers, self.total_pieces = (int(o[-1]) for o in
                                                                 (self.bits_off, self.peer_off, self.piece_off))
        self.structs = (krk_request_torrent * max(k, 1))()
        for t in range(k):
            self.structs[t] = krk_request_torrent(int(n[t]), int(self.n_peers[t]), int(self.flags[t]), int(self.seeds[t]),
                                                  int(self.bits_off[t]), int(self.peer_off[t]), int(self.piece_off[t]))

    def __len__(self):
        return int(self.n_pieces.size)

    def rows(self, bits: np.ndarray, t: int) -> np.ndarray:
        """Torrent t's rows as a (1 + 2 n_peers, words) view of the batch's `bits` array."""
        a, b = int(self.bits_off[t]), int(self.bits_off[t + 1])
        return bits[a:b].reshape(1 + 2 * int(self.n_peers[t]), int(self.words[t]))


class RequestOutputs:
    """The outputs of piece_request_round_dev over a RequestBatch, in device memory or
    (pinned=True) in page-locked host memory the kernels write over PCIe: .counts (uint32 a piece;
    only with counts), .picks (uint32, `limit` a peer), .n_picked (uint32 a peer)."""

    def __init__(self, batch: RequestBatch, limit: int, counts: bool = False, pinned: bool = False):
        self.pieces, self.peers, self.limit, self.pinned = batch.total_pieces, batch.total_peers, int(limit), pinned
        sizes = (self.pieces if counts else None, self.peers * self.limit, self.peers)
        make = (lambda k: PinnedArray((max(k, 1),), np.uint32)) if pinned else (lambda k: DeviceBuffer(max(k, 1) * 4))
        self.counts, self.picks, self.n_picked = (None if k is None else make(k) for k in sizes)

    def fill(self, byte: int):
        """Every output byte set to `byte` (tests: the call must overwrite all of it)."""
        for b in (self.counts, self.picks, self.n_picked):
            if b is None:
                continue
            if self.pinned:
                b.a.view(np.uint8)[:] = byte
            else:
                b.from_host(np.full(b.nbytes, byte, dtype=np.uint8))

    def to_host(self):
        """(counts or None, picks (peers, limit), n_picked) as numpy arrays, once the call's stream has run."""
        def get(b, k):
            if b is None:
                return None
            return b.a[:k].copy() if self.pinned else b.to_host(np.uint32, k)
        return get(self.counts, self.pieces), get(self.picks, self.peers * self.limit).reshape(self.peers, self.limit), \
            get(self.n_picked, self.peers)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None and a.size else None


def piece_availability(peer_bits, n_pieces: int) -> np.ndarray:
    """krk_piece_availability: numPeersByPiece as the column sum of the peers' bitfield rows
    ((n_peers, words) uint64).  Pure host code."""
    words = int(lib.krk_bitfield_words(int(n_pieces)))
    b = np.ascontiguousarray(peer_bits, dtype=np.uint64).reshape(-1, words) if words else np.zeros((len(peer_bits), 0), np.uint64)
    counts = np.zeros(int(n_pieces), dtype=np.uint32)
    check(lib.krk_piece_availability(_p(b, C.c_uint64), b.shape[0], int(n_pieces), _p(counts, C.c_uint32)))
    return counts


def piece_select(cand, blocked, counts, n_pieces: int, q: int, flags: int = PR_RAREST_FIRST, seed: int = 0,
                 peer: int = 0) -> np.ndarray:
    """krk_piece_select: the min(q, candidates) pieces of cand & ~blocked with the smallest
    (key, index), in that order.  Pure host code."""
    c = np.ascontiguousarray(cand, dtype=np.uint64)
    b = None if blocked is None else np.ascontiguousarray(blocked, dtype=np.uint64)
    k = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint32)
    picks = np.zeros(max(int(q), 0), dtype=np.uint32)
    m = C.c_uint32()
    check(lib.krk_piece_select(_p(c, C.c_uint64), _p(b, C.c_uint64), _p(k, C.c_uint32), int(n_pieces), int(q), int(flags),
                               int(seed), int(peer), _p(picks, C.c_uint32), C.byref(m)))
    return picks[:m.value]


def piece_request_round(batch: RequestBatch, bits, quota, limit: int, counts: bool = False):
    """krk_piece_request_round: the whole round on the host.  bits: uint64, the batch's layout;
    quota: int32 a peer.  Returns (counts or None, picks (peers, limit), n_picked)."""
    b = np.ascontiguousarray(bits, dtype=np.uint64)
    q = np.ascontiguousarray(quota, dtype=np.int32)
    if b.size < batch.total_words or q.size < batch.total_peers:
        raise ValueError(f"piece_request_round: {b.size} words and {q.size} quotas for a batch of "
                         f"{batch.total_words} and {batch.total_peers}")
    cnt = np.zeros(batch.total_pieces, dtype=np.uint32) if counts else None
    picks = np.zeros((batch.total_peers, int(limit)), dtype=np.uint32)
    n_picked = np.zeros(batch.total_peers, dtype=np.uint32)
    check(lib.krk_piece_request_round(batch.structs, len(batch), _p(b, C.c_uint64), _p(q, C.c_int32), int(limit),
                                      _p(cnt, C.c_uint32) if counts else None, _p(picks, C.c_uint32),
                                      _p(n_picked, C.c_uint32)))
    return cnt, picks, n_picked


def piece_request_round_dev(batch: RequestBatch, bits_dev, quota_dev, limit: int, out: RequestOutputs | None = None,
                            counts: bool = False, stream=None):
    """krk_piece_request_round_dev: the round in one call on the device.  bits_dev / quota_dev:
    DeviceBuffer or PinnedArray in the batch's layout.  out: RequestOutputs to fill asynchronously
    on `stream` (returned); None: (counts or None, picks, n_picked), returned once the stream has
    run the call."""
    dst = RequestOutputs(batch, limit, counts=counts, pinned=True) if out is None else out
    check(lib.krk_piece_request_round_dev(batch.structs, len(batch), bits_dev.ptr, quota_dev.ptr, int(limit),
                                          dst.counts.ptr if dst.counts is not None else None, dst.picks.ptr,
                                          dst.n_picked.ptr, stream))
    if out is not None:
        return out
    check(lib.krk_stream_sync(stream))
    return dst.to_host()


def piece_request_geometry():
    """(pieces one workgroup pass of the selection scan covers, the thread stride inside it, count
    workgroups a launch has at the most)."""
    g, t, m = C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(lib.krk_piece_request_geometry(C.byref(g), C.byref(t), C.byref(m)))
    return int(g.value), int(t.value), int(m.value)


PR_EXPIRED, PR_UNSENT, PR_INVALID = 1, 2, 3


class ResendBatch:
    """The failed requests of a resend round over a RequestBatch: one list of (piece, peer index or
    PR_NONE, status) a torrent, ascending by piece, packed back to back.  Torrent t's entries (and
    its targets) start at .failed_off[t]; .structs is the krk_resend_torrent array parallel to the
    batch's, .failed the krk_failed_request array."""

    def __init__(self, batch: RequestBatch, lists):
        lists = [list(l) for l in lists]
        if len(lists) != len(batch):
            raise ValueError(f"ResendBatch: {len(lists)} lists for a batch of {len(batch)} torrents")
        k = len(lists)
        self.failed_off = np.zeros(k + 1, dtype=np.uint64)
        self.failed_off[1:] = np.cumsum([len(l) for l in lists])
        self.total_failed = int(self.failed_off[-1])
        self.structs = (krk_resend_torrent * max(k, 1))()
        self.failed = (krk_failed_request * max(self.total_failed, 1))()
        j = 0
        for t, l in enumerate(lists):
            self.structs[t] = krk_resend_torrent(int(self.failed_off[t]), len(l))
            for piece, peer, status in l:
                self.failed[j] = krk_failed_request(int(piece), int(peer), int(status))
                j += 1

    def split(self, a: np.ndarray, t: int) -> np.ndarray:
        """Torrent t's slice of an array with one element a failed request (the targets)."""
        return a[int(self.failed_off[t]):int(self.failed_off[t + 1])]


class ResendOutputs:
    """The outputs of piece_resend_round_dev, in device memory or (pinned=True) in page-locked host
    memory the kernel writes over PCIe: .target (uint32 a failed request), .quota_left (int32 a
    peer; only with quota_left), .n_resent (uint32 a torrent)."""

    def __init__(self, batch: RequestBatch, resend: ResendBatch, quota_left: bool = True, pinned: bool = False):
        self.failed, self.peers, self.torrents, self.pinned = resend.total_failed, batch.total_peers, len(batch), pinned
        make = (lambda k, t: PinnedArray((max(k, 1),), t)) if pinned else (lambda k, t: DeviceBuffer(max(k, 1) * 4))
        self.target = make(self.failed, np.uint32)
        self.quota_left = make(self.peers, np.int32) if quota_left else None
        self.n_resent = make(self.torrents, np.uint32)

    def fill(self, byte: int):
        """Every output byte set to `byte` (tests: the call must overwrite all of it)."""
        for b in (self.target, self.quota_left, self.n_resent):
            if b is None:
                continue
            if self.pinned:
                b.a.view(np.uint8)[:] = byte
            else:
                b.from_host(np.full(b.nbytes, byte, dtype=np.uint8))

    def to_host(self):
        """(target, quota_left or None, n_resent) as numpy arrays, once the call's stream has run."""
        def get(b, k, t):
            if b is None:
                return None
            return b.a[:k].copy() if self.pinned else b.to_host(t, k)
        return get(self.target, self.failed, np.uint32), get(self.quota_left, self.peers, np.int32), \
            get(self.n_resent, self.torrents, np.uint32)


def piece_resend_round(batch: RequestBatch, resend: ResendBatch, bits, quota, quota_left: bool = True):
    """krk_piece_resend_round: the whole resend round on the host.  bits: uint64, the batch's
    layout; quota: int32 a peer.  Returns (target a failed request, quota_left a peer or None,
    n_resent a torrent)."""
    b = np.ascontiguousarray(bits, dtype=np.uint64)
    q = np.ascontiguousarray(quota, dtype=np.int32)
    if b.size < batch.total_words or q.size < batch.total_peers:
        raise ValueError(f"piece_resend_round: {b.size} words and {q.size} quotas for a batch of "
                         f"{batch.total_words} and {batch.total_peers}")
    target = np.zeros(resend.total_failed, dtype=np.uint32)
    left = np.zeros(batch.total_peers, dtype=np.int32) if quota_left else None
    n_resent = np.zeros(len(batch), dtype=np.uint32)
    check(lib.krk_piece_resend_round(batch.structs, resend.structs, len(batch), _p(b, C.c_uint64), _p(q, C.c_int32),
                                     resend.failed, _p(target, C.c_uint32),
                                     _p(left, C.c_int32) if quota_left else None, _p(n_resent, C.c_uint32)))
    return target, left, n_resent


def piece_resend_round_dev(batch: RequestBatch, resend: ResendBatch, bits_dev, quota_dev,
                           out: ResendOutputs | None = None, quota_left: bool = True, stream=None):
    """krk_piece_resend_round_dev: the resend round in one call on the device.  bits_dev /
    quota_dev: DeviceBuffer or PinnedArray in the batch's layout (the rows a reserve round
    uploaded serve as they are).  out: ResendOutputs to fill asynchronously on `stream` (returned);
    None: (target, quota_left or None, n_resent), returned once the stream has run the call."""
    dst = ResendOutputs(batch, resend, quota_left=quota_left, pinned=True) if out is None else out
    check(lib.krk_piece_resend_round_dev(batch.structs, resend.structs, len(batch), bits_dev.ptr, quota_dev.ptr,
                                         resend.failed, dst.target.ptr,
                                         dst.quota_left.ptr if dst.quota_left is not None else None, dst.n_resent.ptr,
                                         stream))
    if out is not None:
        return out
    check(lib.krk_stream_sync(stream))
    return dst.to_host()


def piece_resend_geometry() -> int:
    """The peers one workgroup pass over a failed request's peers covers (one peer a thread)."""
    s = C.c_uint64()
    check(lib.krk_piece_resend_geometry(C.byref(s)))
    return int(s.value)


AN_MAX_WINDOWS, AN_MAX_ORIGINS, AN_MAX_LIMIT = 8, 8, 64
AN_DEFAULT, AN_COMPLETENESS, AN_COMPLETE = 0, 1, 1
AN_NONE, AN_ORIGIN, AN_COMPLETE_BIT = 0xFFFFFFFF, 0x80000000, 0x40000000


class AnnounceBatch:
    """The torrents and announces of an announce round.  torrents: (n_peers, n_windows, cur_row,
    n_origins) each; their peer stores -- 2 * n_windows rows of krk_bitfield_words(n_peers) words,
    (member, complete) a ring row -- are packed back to back, torrent t's from word .bits_off[t].
    announces: (torrent, peer, flags, source, seed) each.  .structs / .announces are the
    krk_announce_torrent / krk_announce arrays."""

    def __init__(self, torrents, announces):
        torrents, announces = [tuple(int(x) for x in t) for t in torrents], [tuple(int(x) for x in a) for a in announces]
        k = len(torrents)
        words = [2 * w * ((p + 63) // 64) for p, w, _, _ in torrents]
        self.bits_off = np.zeros(k + 1, dtype=np.uint64)
        self.bits_off[1:] = np.cumsum(words)
        self.total_words = int(self.bits_off[-1])
        self.structs = (krk_announce_torrent * max(k, 1))()
        for t, (p, w, cur, o) in enumerate(torrents):
            self.structs[t] = krk_announce_torrent(p, w, cur, o, 0, int(self.bits_off[t]))
        self.n_torrents, self.n_announces = k, len(announces)
        self.announces = (krk_announce * max(len(announces), 1))()
        for j, a in enumerate(announces):
            self.announces[j] = krk_announce(*a)

    def __len__(self):
        return self.n_torrents


class AnnounceOutputs:
    """The outputs of announce_round_dev, in device memory or (pinned=True) in page-locked host
    memory the kernel writes over PCIe: .handout (uint32, limit + AN_MAX_ORIGINS an announce),
    .n_out (uint32 an announce), .labels (uint32, three an announce)."""

    def __init__(self, batch: AnnounceBatch, limit: int, pinned: bool = False):
        self.n, self.cap, self.pinned = batch.n_announces, int(limit) + AN_MAX_ORIGINS, pinned
        make = (lambda k: PinnedArray((max(k, 1),), np.uint32)) if pinned else (lambda k: DeviceBuffer(max(k, 1) * 4))
        self.handout, self.n_out, self.labels = make(self.n * self.cap), make(self.n), make(self.n * 3)

    def fill(self, byte: int):
        """Every output byte set to `byte` (tests: the call must overwrite all of it)."""
        for b in (self.handout, self.n_out, self.labels):
            if self.pinned:
                b.a.view(np.uint8)[:] = byte
            else:
                b.from_host(np.full(b.nbytes, byte, dtype=np.uint8))

    def to_host(self):
        """(handout (A, cap), n_out (A,), labels (A, 3)), once the call's stream has run."""
        def get(b, k):
            return b.a[:k].copy() if self.pinned else b.to_host(np.uint32, k)
        return get(self.handout, self.n * self.cap).reshape(self.n, self.cap), get(self.n_out, self.n), \
            get(self.labels, self.n * 3).reshape(self.n, 3)


def _announce_bits(batch: AnnounceBatch, bits, who: str):
    if not (isinstance(bits, np.ndarray) and bits.dtype == np.uint64 and bits.flags.c_contiguous):
        raise ValueError(f"{who}: bits must be a contiguous uint64 array")
    if bits.size < batch.total_words:
        raise ValueError(f"{who}: {bits.size} words for a batch of {batch.total_words}")
    return bits


def announce_handout(batch: AnnounceBatch, bits, k: int, limit: int, policy: int = AN_DEFAULT):
    """krk_announce_handout: announce k's handout over the rows as they are (no update).  Returns
    (handout with limit + AN_MAX_ORIGINS entries, n_out, the three label counts)."""
    b = _announce_bits(batch, bits, "announce_handout")
    if not 0 <= k < batch.n_announces:
        raise IndexError(f"announce_handout: announce {k} of {batch.n_announces}")
    handout = np.zeros(max(int(limit), 0) + AN_MAX_ORIGINS, dtype=np.uint32)
    labels, n = np.zeros(3, dtype=np.uint32), C.c_uint32()
    check(lib.krk_announce_handout(batch.structs, len(batch), _p(b, C.c_uint64), C.byref(batch.announces[k]), limit, policy,
                                   _p(handout, C.c_uint32), C.byref(n), _p(labels, C.c_uint32)))
    return handout, int(n.value), labels


def announce_round(batch: AnnounceBatch, bits, limit: int, policy: int = AN_DEFAULT):
    """krk_announce_round: the whole announce round on the host.  bits: a contiguous uint64 array
    in the batch's layout, UPDATED IN PLACE.  Returns (handout (A, limit + AN_MAX_ORIGINS), n_out
    (A,), labels (A, 3))."""
    b = _announce_bits(batch, bits, "announce_round")
    n, cap = batch.n_announces, max(int(limit), 0) + AN_MAX_ORIGINS
    handout, n_out, labels = np.zeros((n, cap), np.uint32), np.zeros(n, np.uint32), np.zeros((n, 3), np.uint32)
    check(lib.krk_announce_round(batch.structs, len(batch), _p(b, C.c_uint64), batch.announces, n, limit, policy,
                                 _p(handout, C.c_uint32), _p(n_out, C.c_uint32), _p(labels, C.c_uint32)))
    return handout, n_out, labels


def announce_round_dev(batch: AnnounceBatch, bits_dev, limit: int, policy: int = AN_DEFAULT,
                       out: AnnounceOutputs | None = None, stream=None):
    """krk_announce_round_dev: the announce round on the device.  bits_dev: DeviceBuffer or
    PinnedArray in the batch's layout, updated in place.  out: AnnounceOutputs to fill
    asynchronously on `stream` (returned); None: (handout, n_out, labels), returned once the stream
    has run the call."""
    dst = AnnounceOutputs(batch, limit, pinned=True) if out is None else out
    check(lib.krk_announce_round_dev(batch.structs, len(batch), bits_dev.ptr, batch.announces, batch.n_announces, limit,
                                     policy, dst.handout.ptr, dst.n_out.ptr, dst.labels.ptr, stream))
    if out is not None:
        return out
    check(lib.krk_stream_sync(stream))
    return dst.to_host()


CN_NONE, CN_NO_ROW, CN_TORRENT_COMPLETE, CN_DISABLE_BLACKLIST = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 1, 1
CN_ESTABLISHED, CN_FAILED_IN, CN_FAILED_OUT, CN_CLOSED = 0, 1, 2, 3
(CN_OK, CN_FREED, CN_NOOP, CN_NOT_PENDING, CN_BLACKLISTED_NOW, CN_STILL_BLACKLISTED, CN_AT_CAPACITY, CN_ALREADY_PENDING,
 CN_ALREADY_ACTIVE, CN_TOO_MANY_MUTUAL, CN_SELF, CN_BLACKLISTED, CN_TORRENT_IS_COMPLETE) = (1 << k for k in range(13))


class ConnBatch:
    """The torrents and lists of a connection round (or the torrents of a preemption sweep).
    torrents: (n_peers, self_peer, flags) each; their states are packed back to back: torrent t's
    active and pending rows from word .bits_off[t] of `bits`, its expiries (and a sweep's times) from
    .peer_off[t], its close row from word .close_off[t].  lists: per torrent (transitions
    [(peer, kind)], incoming [(peer, neighbour row or None)], dials [peer]), a neighbour row being
    krk_bitfield_words(n_peers) uint64 words; None: no lists (a sweep).  .structs / .lists /
    .transitions / .incoming are the C arrays, .dials and .neighbors numpy arrays."""

    def __init__(self, torrents, lists=None):
        torrents = [tuple(int(x) for x in t) for t in torrents]
        k = len(torrents)
        lists = [((), (), ())] * k if lists is None else [tuple(list(x) for x in l) for l in lists]
        if len(lists) != k:
            raise ValueError(f"ConnBatch: {len(lists)} lists for {k} torrents")
        wp = [(p + 63) // 64 for p, _, _ in torrents]
        self.bits_off, self.peer_off, self.close_off = (np.zeros(k + 1, dtype=np.uint64) for _ in range(3))
        self.bits_off[1:] = np.cumsum([2 * w for w in wp])
        self.peer_off[1:] = np.cumsum([p for p, _, _ in torrents])
        self.close_off[1:] = np.cumsum(wp)
        self.total_words, self.total_peers, self.close_words = int(self.bits_off[-1]), int(self.peer_off[-1]), int(self.close_off[-1])
        self.n_torrents = k
        self.structs = (krk_conn_torrent * max(k, 1))()
        self.lists = (krk_conn_lists * max(k, 1))()
        nt, ni, nd = (sum(len(l[j]) for l in lists) for j in range(3))
        self.n_trans, self.n_in, self.n_dial = nt, ni, nd
        self.transitions = (krk_conn_transition * max(nt, 1))()
        self.incoming = (krk_conn_incoming * max(ni, 1))()
        self.dials = np.zeros(max(nd, 1), dtype=np.uint32)
        self.list_off = np.zeros((k + 1, 3), dtype=np.uint64)
        rows, at, a = [], 0, [0, 0, 0]
        for t, ((p, me, flags), (tr, inc, dial)) in enumerate(zip(torrents, lists)):
            self.structs[t] = krk_conn_torrent(p, me, flags, 0, int(self.bits_off[t]), int(self.peer_off[t]),
                                               int(self.close_off[t]))
            self.lists[t] = krk_conn_lists(a[0], len(tr), a[1], len(inc), a[2], len(dial))
            for peer, kind in tr:
                self.transitions[a[0]] = krk_conn_transition(int(peer), int(kind))
                a[0] += 1
            for peer, row in inc:
                if row is None:
                    self.incoming[a[1]] = krk_conn_incoming(int(peer), 0, CN_NO_ROW)
                else:
                    row = np.ascontiguousarray(row, dtype=np.uint64)
                    if row.size != wp[t]:
                        raise ValueError(f"ConnBatch: a neighbour row of {row.size} words for {p} peers")
                    self.incoming[a[1]] = krk_conn_incoming(int(peer), 0, at)
                    rows.append(row)
                    at += wp[t]
                a[1] += 1
            for peer in dial:
                self.dials[a[2]] = int(peer)
                a[2] += 1
            self.list_off[t + 1] = a
        self.neighbors = np.concatenate(rows) if rows else np.zeros(1, dtype=np.uint64)
        self.n_neighbor_words = at

    def __len__(self):
        return self.n_torrents

    def split(self, a: np.ndarray, t: int, which: int) -> np.ndarray:
        """Torrent t's slice of a status array: which = 0 transitions, 1 incoming, 2 dials."""
        return a[int(self.list_off[t, which]):int(self.list_off[t + 1, which])]


class ConnOutputs:
    """The outputs of conn_round_dev, in device memory or (pinned=True) in page-locked host memory:
    .trans, .incoming, .dial (uint32 statuses an entry), .n_admitted (uint32, two a torrent),
    .n_freed (uint32 a torrent)."""

    def __init__(self, batch: ConnBatch, pinned: bool = False):
        self.sizes = (batch.n_trans, batch.n_in, batch.n_dial, 2 * len(batch), len(batch))
        self.pinned = pinned
        make = (lambda k: PinnedArray((max(k, 1),), np.uint32)) if pinned else (lambda k: DeviceBuffer(max(k, 1) * 4))
        self.trans, self.incoming, self.dial, self.n_admitted, self.n_freed = (make(k) for k in self.sizes)

    def buffers(self):
        return self.trans, self.incoming, self.dial, self.n_admitted, self.n_freed

    def fill(self, byte: int):
        """Every output byte set to `byte` (tests: the call must overwrite all of it)."""
        for b in self.buffers():
            if self.pinned:
                b.a.view(np.uint8)[:] = byte
            else:
                b.from_host(np.full(b.nbytes, byte, dtype=np.uint8))

    def to_host(self):
        """(trans, incoming, dial, n_admitted (T, 2), n_freed) as numpy arrays, once the stream has run."""
        got = [b.a[:k].copy() if self.pinned else b.to_host(np.uint32, k) for b, k in zip(self.buffers(), self.sizes)]
        got[3] = got[3].reshape(-1, 2)
        return tuple(got)


def conn_round(batch: ConnBatch, bits, expiry, capacity, now: int, blacklist_duration: int, max_mutual: int, flags: int = 0):
    """krk_conn_round: the whole connection round on the host.  bits (uint64), expiry (int64) and
    capacity (uint32) are contiguous arrays in the batch's layout, UPDATED IN PLACE.  Returns
    (transition, incoming and dial statuses, n_admitted (T, 2), n_freed)."""
    for a, t, n, what in ((bits, np.uint64, batch.total_words, "bits"), (expiry, np.int64, batch.total_peers, "expiry"),
                          (capacity, np.uint32, len(batch), "capacity")):
        if not (isinstance(a, np.ndarray) and a.dtype == t and a.flags.c_contiguous and a.size >= n):
            raise ValueError(f"conn_round: {what} must be a contiguous {np.dtype(t).name} array of at least {n}")
    outs = [np.zeros(max(k, 1), dtype=np.uint32) for k in (batch.n_trans, batch.n_in, batch.n_dial, 2 * len(batch), len(batch))]
    check(lib.krk_conn_round(batch.structs, batch.lists, len(batch), bits.ctypes.data, expiry.ctypes.data,
                             capacity.ctypes.data, batch.transitions, batch.incoming, batch.dials.ctypes.data,
                             batch.neighbors.ctypes.data, batch.n_neighbor_words, now, blacklist_duration, max_mutual, flags,
                             *(o.ctypes.data for o in outs)))
    return (outs[0][:batch.n_trans], outs[1][:batch.n_in], outs[2][:batch.n_dial],
            outs[3][:2 * len(batch)].reshape(-1, 2), outs[4][:len(batch)])


def conn_round_dev(batch: ConnBatch, bits_dev, expiry_dev, capacity_dev, neighbors_dev, now: int, blacklist_duration: int,
                   max_mutual: int, flags: int = 0, out: ConnOutputs | None = None, stream=None):
    """krk_conn_round_dev: the round in one launch on the device.  bits_dev / expiry_dev /
    capacity_dev: DeviceBuffer or PinnedArray in the batch's layout, updated in place;
    neighbors_dev: the batch's .neighbors in device or page-locked memory (None: uploaded here).
    out: ConnOutputs to fill asynchronously on `stream` (returned); None: the host form's tuple,
    returned once the stream has run the call."""
    if neighbors_dev is None and batch.n_neighbor_words:
        neighbors_dev = DeviceBuffer(batch.neighbors.nbytes)
        neighbors_dev.from_host(batch.neighbors)
    dst = ConnOutputs(batch, pinned=True) if out is None else out
    check(lib.krk_conn_round_dev(batch.structs, batch.lists, len(batch), bits_dev.ptr, expiry_dev.ptr, capacity_dev.ptr,
                                 batch.transitions, batch.incoming, batch.dials.ctypes.data,
                                 neighbors_dev.ptr if neighbors_dev is not None else None, batch.n_neighbor_words, now,
                                 blacklist_duration, max_mutual, flags, *(b.ptr for b in dst.buffers()), stream))
    if out is not None:
        return out
    check(lib.krk_stream_sync(stream))
    return dst.to_host()


def conn_preempt(batch: ConnBatch, bits, created, received, sent, now: int, conn_tti: int, conn_ttl: int):
    """krk_conn_preempt on the host: (close rows packed at .close_off, n_close a torrent)."""
    b = np.ascontiguousarray(bits, dtype=np.uint64)
    times = [np.ascontiguousarray(a, dtype=np.int64) for a in (created, received, sent)]
    if b.size < batch.total_words or any(a.size < batch.total_peers for a in times):
        raise ValueError("conn_preempt: bits or times shorter than the batch's layout")
    close = np.zeros(max(batch.close_words, 1), dtype=np.uint64)
    n_close = np.zeros(max(len(batch), 1), dtype=np.uint32)
    check(lib.krk_conn_preempt(batch.structs, len(batch), b.ctypes.data, *(a.ctypes.data for a in times), now, conn_tti,
                               conn_ttl, close.ctypes.data, n_close.ctypes.data))
    return close[:batch.close_words], n_close[:len(batch)]


def conn_preempt_dev(batch: ConnBatch, bits_dev, created_dev, received_dev, sent_dev, now: int, conn_tti: int,
                     conn_ttl: int, stream=None):
    """krk_conn_preempt_dev: the sweep on the device over arrays in device or page-locked memory;
    returns the host form's tuple once the stream has run the call."""
    close = PinnedArray((max(batch.close_words, 1),), np.uint64)
    n_close = PinnedArray((max(len(batch), 1),), np.uint32)
    check(lib.krk_conn_preempt_dev(batch.structs, len(batch), bits_dev.ptr, created_dev.ptr, received_dev.ptr, sent_dev.ptr,
                                   now, conn_tti, conn_ttl, close.ptr, n_close.ptr, stream))
    check(lib.krk_stream_sync(stream))
    return close.a[:batch.close_words].copy(), n_close.a[:len(batch)].copy()


class KernelTimer:
    """hipEvent-based per-kernel device time (recorded on each kernel's stream)."""

    def __enter__(self):
        check(lib.krk_set_timing(1))
        check(lib.krk_reset_kernel_stats())
        return self

    def __exit__(self, *a):
        check(lib.krk_set_timing(0))

    @staticmethod
    def timeline(kernel: str):
        """[(plan, units, start_ms, end_ms)] of every timed launch of `kernel` since the
        timer was entered (krk_kernel_timeline)."""
        n = C.c_uint64()
        check(lib.krk_kernel_timeline(kernel.encode(), None, 0, C.byref(n)))
        recs = (krk_launch_rec * max(1, n.value))()
        check(lib.krk_kernel_timeline(kernel.encode(), recs, n.value, C.byref(n)))
        return [(r.plan, r.units, r.start_ms, r.end_ms) for r in recs[:n.value]]

    @staticmethod
    def stats(kernel: str):
        n = C.c_uint64()
        ms = C.c_double()
        check(lib.krk_kernel_stats(kernel.encode(), C.byref(n), C.byref(ms)))
        return n.value, ms.value
