"""Host-side mirror of lib/metainfogen over the C ABI.

* ``newPieceLengthConfig`` / ``pieceLengthConfig.get``: lib/metainfogen/config.go:48-80
* ``Generator.Generate``: lib/metainfogen/generator.go:40-58 (stat -> piece length
  -> NewMetaInfo over the cache file -> persist the _torrentmeta sidecar)
* ``Generator.GenerateBatch``: the batch form used for whole-CAS regeneration
  (SURVEY.md §8(f) row 2): one pass over many cache files (krk_piece_sums_files).
* ``Generator.VerifyAndGenerateBatch`` / ``VerifyAndGenerateUploads``: upload verification
  fused with Generate, over upload bytes or the upload files.
* ``Generator.VerifyAll``: the read-only scrub -- every cached blob against the _torrentmeta
  stored for it (krk_verify_files: piece bitfields, and the SHA-256 against the name).
* ``Generator.OverwriteMetaInfo`` / ``RepieceAll``: a stored _torrentmeta brought to a coarser
  piece length from its stored sums alone (krk_repiece_sums / krk_repiece_batch[_dev]) --
  Server.overwriteMetaInfo (origin/blobserver/server.go:347-360) and a piece-length table change
  without rereading the cache.

The CAS store itself (lib/store) is out of scope; ``DirCAS`` is a minimal
stand-in exposing the three calls Generate makes.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import core
from ._capi import (KRK_EIO, check, krk_blob, krk_file_blob, krk_metainfo_json_blob, krk_metainfo_json_span,
                    krk_repiece_blob, lib)


class pieceLengthConfig:
    def __init__(self, ranges):
        self.ranges = ranges  # sorted [(fileSize, pieceLength)]

    def get(self, file_size: int) -> int:
        t = np.ascontiguousarray([a for a, _ in self.ranges], dtype=np.int64)
        l = np.ascontiguousarray([b for _, b in self.ranges], dtype=np.int64)
        return lib.krk_piece_length_for_size(t.ctypes.data_as(C.POINTER(C.c_int64)),
                                              l.ctypes.data_as(C.POINTER(C.c_int64)), len(t), file_size)


def newPieceLengthConfig(piece_length_by_file_size: dict) -> pieceLengthConfig:
    if not piece_length_by_file_size:
        raise ValueError("no piece lengths configured")
    return pieceLengthConfig(sorted((int(a), int(b)) for a, b in piece_length_by_file_size.items()))


DefaultShardIDLength = 2  # lib/store/base/const.go:16-18


class DirCAS:
    """Minimal content-addressed cache directory in the reference's layout:
    <root>/<hex[0:2]>/<hex[2:4]>/<hex>/data with the _torrentmeta sidecar beside it
    (casFileEntryFactory.GetRelativePath, lib/store/base/file_entry.go:176-189;
    getMetadataPath :468-469)."""

    def __init__(self, root: str):
        self.root = root

    def _dir(self, hex_: str) -> str:
        shards = [hex_[2 * i:2 * i + 2] for i in range(min(DefaultShardIDLength, len(hex_) // 2))]
        return os.path.join(self.root, *shards, hex_)

    def ListNames(self) -> list[str]:
        """Every cached blob name, walking the shard directories (file_entry.go ListNames)."""
        out = []
        for dirpath, dirnames, filenames in os.walk(self.root):
            rel = os.path.relpath(dirpath, self.root)
            depth = 0 if rel == "." else rel.count(os.sep) + 1
            if depth == DefaultShardIDLength + 1 and "data" in filenames:
                out.append(os.path.basename(dirpath))
                dirnames[:] = []
        return sorted(out)

    def Listing(self):
        """The cache as a castore.Listing: ListNames() with the columns cleanup needs -- mtime and
        size from stat, the last access time from the _last_access_time sidecar beside `data`
        (metadata.LastAccessTime; KRK_NO_TIME where there is none)."""
        from . import castore
        names = self.ListNames()
        mtime, size, atime = [], [], []
        for name in names:
            st = self.GetCacheFileStat(name)
            mtime.append(st.st_mtime_ns)
            size.append(st.st_size)
            try:
                with open(os.path.join(self._dir(name), castore.LastAccessTime.Suffix), "rb") as f:
                    lat = castore.LastAccessTime()
                    lat.Deserialize(f.read())
                atime.append(lat.Time * 1_000_000_000)
            except FileNotFoundError:
                atime.append(castore.KRK_NO_TIME)
        return castore.Listing(names, mtime_ns=mtime, size=size, atime_ns=atime)

    def GetCacheFileStat(self, hex_: str) -> os.stat_result:
        return os.stat(os.path.join(self._dir(hex_), "data"))

    def GetCacheFileReader(self, hex_: str):
        return open(os.path.join(self._dir(hex_), "data"), "rb")

    def GetCacheFilePath(self, hex_: str) -> str:
        """The cache file's path (base FileOp.GetFilePath): lets GenerateBatch read
        the file natively into pinned staging instead of through a reader."""
        return os.path.join(self._dir(hex_), "data")

    def GetCacheFileMetadata(self, hex_: str) -> bytes:
        """The _torrentmeta sidecar's bytes (base FileOp.GetFileMetadata); FileNotFoundError
        when the blob has none."""
        with open(os.path.join(self._dir(hex_), "_torrentmeta"), "rb") as f:
            return f.read()

    def SetCacheFileMetadata(self, hex_: str, mi: core.MetaInfo) -> bool:
        return self.SetCacheFileMetadataBytes(hex_, mi.Serialize())

    def SetCacheFileMetadataBytes(self, hex_: str, b: bytes) -> bool:
        """SetCacheFileMetadata for a sidecar that is serialised already (the device codec's
        documents): the same compare-then-write, the same `changed` return."""
        p = os.path.join(self._dir(hex_), "_torrentmeta")
        if os.path.exists(p) and open(p, "rb").read() == b:
            return False
        with open(p, "wb") as f:
            f.write(b)
        return True

    def WriteCacheFileAs(self, d: core.Digest, data) -> core.Digest:
        """Commit already-verified bytes under their digest."""
        os.makedirs(self._dir(d.Hex()), exist_ok=True)
        with open(os.path.join(self._dir(d.Hex()), "data"), "wb") as f:
            f.write(memoryview(data))
        return d

    def MoveUploadFileToCache(self, upload_path: str, hex_: str) -> None:
        """CAStore.MoveUploadFileToCache (origin/blobserver/uploader.go:98 commit): the
        verified upload file renamed into the cache; FileExistsError when the blob is
        already cached (the uploader's 409).  The upload file is deleted either way
        (lib/store/ca_store.go:79-86: `defer s.DeleteUploadFile(uploadName)`)."""
        dst = os.path.join(self._dir(hex_), "data")
        os.makedirs(self._dir(hex_), exist_ok=True)
        try:
            if os.path.exists(dst):
                raise FileExistsError(dst)
            os.replace(upload_path, dst)
        finally:
            if os.path.exists(upload_path):
                os.remove(upload_path)

    def WriteCacheFile(self, data: bytes) -> core.Digest:
        d = core.NewDigester().FromBytes(data)
        os.makedirs(self._dir(d.Hex()), exist_ok=True)
        with open(os.path.join(self._dir(d.Hex()), "data"), "wb") as f:
            f.write(data)
        return d


def repiece_sidecars_dev(entries) -> dict:
    """{name: the new sidecar's bytes} for entries' [(name, blob size, target piece length, stored
    sidecar bytes)]: sidecar bytes in, sidecar bytes out, no per-sum host work.  Per stored sidecar
    the host reads the envelope (krk_metainfo_json_envelope, O(1)) and makes
    Generator._stored_metainfo's no-read checks on it -- the Name is the blob's, the Length its
    size, the piece length positive -- and RepieceAll's: the piece length divides the target and is
    not the target.  Then one upload of the spans between the brackets, and on one stream
    krk_metainfo_parse_sums_batch_dev -> krk_repiece_batch_dev -> krk_info_hash_batch_dev ->
    krk_metainfo_serialize_batch_dev, one copy back of [documents][lengths][statuses].  (The
    InfoHashes stay on the device: the sidecar does not hold them.)  A blob whose envelope is
    refused, whose span is not canonical or does not hold the blob's number of sums (a nonzero
    device status) or that fails a check is not in the result: it belongs to the general path."""
    from . import device as D
    cand, texts = [], []
    pl, ln, a0, a1, null = C.c_int64(), C.c_int64(), C.c_uint64(), C.c_uint64(), C.c_int()
    nm = C.create_string_buffer(64)
    for name, size, target, raw in entries:
        if lib.krk_metainfo_json_envelope(raw, len(raw), C.byref(pl), C.byref(a0), C.byref(a1), C.byref(null), nm,
                                          C.byref(ln)) != 0:
            continue
        p = pl.value
        if nm.raw.decode() != name or ln.value != size or p <= 0 or target <= 0 or target == p or target % p:
            continue
        cand.append((name, size, p, target))
        texts.append(raw[a0.value:a1.value])
    n = len(cand)
    if not n:
        return {}
    spans = (krk_metainfo_json_span * n)()
    rp = (krk_repiece_blob * n)()
    ser = (krk_metainfo_json_blob * n)()
    t = a = b = o = 0
    for i, ((name, size, p, target), text) in enumerate(zip(cand, texts)):
        n_old, n_new = int(lib.krk_num_pieces(size, p)), int(lib.krk_num_pieces(size, target))
        spans[i] = krk_metainfo_json_span(t, len(text), a, n_old)
        rp[i] = krk_repiece_blob(size, p, target, a, b)
        ser[i] = krk_metainfo_json_blob(b, n_new, target, size, o, n_new == 0, 0, name.encode())
        t, a, b = t + len(text), a + n_old, b + n_new
        o += int(lib.krk_metainfo_json_bound(n_new))
    # one device buffer: [spans' text][stored sums][new sums][InfoHashes] then the part that
    # comes back, [documents][lengths][statuses]
    up = lambda x, to: (x + to - 1) // to * to
    at_old = up(t, 4)
    at_new = at_old + 4 * a
    at_ih = at_new + 4 * b
    at_doc = up(at_ih + 20 * n, 8)
    at_len = up(at_doc + o, 8)
    at_st = at_len + 8 * n
    end = at_st + 4 * n
    dev = D.DeviceBuffer(end)
    back = D.PinnedArray((end - at_doc,), np.uint8)
    try:
        dev.from_host(np.frombuffer(b"".join(texts), dtype=np.uint8))
        check(lib.krk_metainfo_parse_sums_batch_dev(spans, n, dev.ptr, dev.ptr + at_old, dev.ptr + at_st, None))
        check(lib.krk_repiece_batch_dev(rp, n, dev.ptr + at_old, dev.ptr + at_new, None))
        buf, noff = D.pack_names([c[0] for c in cand])
        i64p, u64p = C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
        col = lambda v, dt: np.ascontiguousarray(v, dtype=dt)
        pl_, ln_ = col([c[3] for c in cand], np.int64), col([c[1] for c in cand], np.int64)
        so_, ns_ = col([x.sums_off for x in ser], np.uint64), col([x.n_sums for x in ser], np.uint64)
        check(lib.krk_info_hash_batch_dev(pl_.ctypes.data_as(i64p), dev.ptr + at_new, so_.ctypes.data_as(u64p),
                                          ns_.ctypes.data_as(u64p), buf or None, noff.ctypes.data_as(u64p),
                                          ln_.ctypes.data_as(i64p), n, dev.ptr + at_ih, None))
        check(lib.krk_metainfo_serialize_batch_dev(ser, n, dev.ptr + at_new, dev.ptr + at_doc, dev.ptr + at_len,
                                                   None))
        back.fill_from_async(dev, None, at_doc)
        check(lib.krk_stream_sync(None))
        lens = back.a[at_len - at_doc:at_st - at_doc].view(np.uint64)
        status = back.a[at_st - at_doc:].view(np.uint32)
        return {c[0]: back.a[int(x.out_off):int(x.out_off) + int(lens[i])].tobytes()
                for i, (c, x) in enumerate(zip(cand, ser)) if status[i] == 0}
    finally:
        dev.free()


class Generator:
    def __init__(self, config: dict, cas):
        try:
            self.pieceLengthConfig = newPieceLengthConfig(config)
        except ValueError as e:
            raise ValueError(f"piece length config: {e}") from None
        self.cas = cas

    def Generate(self, d: core.Digest) -> None:
        try:
            info = self.cas.GetCacheFileStat(d.Hex())
        except OSError as e:
            raise IOError(f"cache stat: {e}") from None
        try:
            f = self.cas.GetCacheFileReader(d.Hex())
        except OSError as e:
            raise IOError(f"get cache file: {e}") from None
        with f:
            pl = self.pieceLengthConfig.get(info.st_size)
            try:
                mi = core.NewMetaInfo(d, f, pl)
            except (ValueError, IOError) as e:
                raise IOError(f"create metainfo: {e}") from None
        try:
            self.cas.SetCacheFileMetadata(d.Hex(), mi)
        except OSError as e:
            raise IOError(f"set metainfo: {e}") from None

    def RegenerateAll(self, batch_bytes: int = 8 << 30) -> dict:
        """Whole-CAS regeneration: every cached blob's
        _torrentmeta rewritten from GPU piece sums in batches of ~batch_bytes
        (each batch one pinned, pipelined pass), byte-identical to what
        Generate writes.  Returns counts of blobs seen / sidecars changed."""
        names = self.cas.ListNames()
        seen = changed = 0
        batch, size = [], 0
        for i, name in enumerate(names):
            batch.append(core.NewSHA256DigestFromHex(name))
            size += self.cas.GetCacheFileStat(name).st_size
            if size >= batch_bytes or i == len(names) - 1:
                self.GenerateBatch(batch)
                changed += self._last_changed
                seen += len(batch)
                batch, size = [], 0
        return {"blobs": seen, "changed": changed}

    def _stored_metainfo(self, name: str, st_size: int):
        """The blob's stored MetaInfo if it passes VerifyAll's no-read checks -- it parses, its
        Name is the directory's, its Length the stat size, its piece length positive and its sum
        count right -- else None."""
        try:
            mi = core.DeserializeMetaInfo(self.cas.GetCacheFileMetadata(name))
        except (OSError, ValueError):
            return None
        if mi.Digest().Hex() != name or mi.Length() != st_size or mi.PieceLength() <= 0:
            return None
        if mi.NumPieces() != int(lib.krk_num_pieces(st_size, mi.PieceLength())):
            return None
        return mi

    def OverwriteMetaInfo(self, d: core.Digest, piece_length: int) -> None:
        """Server.overwriteMetaInfo (origin/blobserver/server.go:347-360): d's metainfo at
        piece_length written over any existing one.  With a usable stored sidecar
        (_stored_metainfo) whose piece length divides piece_length the new sums come from the
        stored ones (MetaInfo.Repiece) and the blob is not read; otherwise the blob is read, as
        the reference does.  The reference's error prefixes."""
        mi = None
        if piece_length > 0:
            try:
                stored = self._stored_metainfo(d.Hex(), self.cas.GetCacheFileStat(d.Hex()).st_size)
            except OSError:
                stored = None  # the reader below reports it
            if stored is not None and piece_length % stored.PieceLength() == 0:
                mi = stored.Repiece(piece_length)
        if mi is None:
            try:
                f = self.cas.GetCacheFileReader(d.Hex())
            except OSError as e:
                raise IOError(f"get cache file: {e}") from None
            with f:
                try:
                    mi = core.NewMetaInfo(d, f, piece_length)
                except (ValueError, IOError) as e:
                    raise IOError(f"create metainfo: {e}") from None
        try:
            self.cas.SetCacheFileMetadata(d.Hex(), mi)
        except OSError as e:
            raise IOError(f"set metainfo: {e}") from None

    def RepieceAll(self, placement: str = "host", batch_bytes: int = 8 << 30) -> dict:
        """Every cached blob's _torrentmeta brought to the piece length the config gives its
        size -- what RegenerateAll writes after a piece-length table change, byte for byte --
        reading only the blobs whose stored sums cannot serve.  Per blob, with its usable stored
        sidecar (_stored_metainfo): the target equals the stored piece length: ``unchanged``; the
        stored one divides it: ``repieced`` from the stored sums -- all of them in ONE
        krk_repiece_batch call (placement "host"), or (placement "gpu") one device chain from the
        stored sidecars' bytes to the new sidecars' bytes (_repiece_chain_dev); everything else, a
        missing or unusable sidecar included: ``reread`` through GenerateBatch in batches of
        ~batch_bytes.  Returns {"blobs", "unchanged", "repieced", "reread", "changed" (sidecars
        whose bytes changed), "bytes_not_read" (the sizes of the unchanged and repieced blobs)}."""
        if placement not in ("host", "gpu"):
            raise ValueError(f"unknown placement {placement!r}")
        names = self.cas.ListNames()
        sizes = [self.cas.GetCacheFileStat(name).st_size for name in names]
        targets = [self.pieceLengthConfig.get(size) for size in sizes]
        docs = self._repiece_chain_dev(names, sizes, targets) if placement == "gpu" else {}
        unchanged = changed = bytes_not_read = repieced = 0
        todo, reread = [], []
        for name, size, target in zip(names, sizes, targets):
            if name in docs:
                repieced += 1
                bytes_not_read += size
                try:
                    changed += bool(self.cas.SetCacheFileMetadataBytes(name, docs[name]))
                except OSError as e:
                    raise IOError(f"set metainfo: {e}") from None
                continue
            mi = self._stored_metainfo(name, size)
            if mi is not None and target == mi.PieceLength():
                unchanged += 1
                bytes_not_read += size
            elif mi is not None and target > 0 and target % mi.PieceLength() == 0:
                todo.append((name, mi, target))
                bytes_not_read += size
            else:
                reread.append((name, size))
        if todo:
            for (name, mi, target), (sums, ih) in zip(todo, self._repiece_batch(todo)):
                new = core.MetaInfo(target, sums, name, mi.Length(), mi.Digest(), ih)
                try:
                    changed += bool(self.cas.SetCacheFileMetadata(name, new))
                except OSError as e:
                    raise IOError(f"set metainfo: {e}") from None
        batch, size = [], 0
        for i, (name, n) in enumerate(reread):
            batch.append(core.NewSHA256DigestFromHex(name))
            size += n
            if size >= batch_bytes or i == len(reread) - 1:
                self.GenerateBatch(batch)
                changed += self._last_changed
                batch, size = [], 0
        return {"blobs": len(names), "unchanged": unchanged, "repieced": repieced + len(todo), "reread": len(reread),
                "changed": changed, "bytes_not_read": bytes_not_read}

    def _repiece_batch(self, todo):
        """[(new sums or None, InfoHash)] of todo's [(name, stored MetaInfo, new piece length)]:
        ONE krk_repiece_batch and one krk_info_hash_batch, on the host."""
        n = len(todo)
        arr = (krk_repiece_blob * n)()
        a = b = 0
        for i, (_, mi, target) in enumerate(todo):
            arr[i] = krk_repiece_blob(mi.Length(), mi.PieceLength(), target, a, b)
            a += mi.NumPieces()
            b += int(lib.krk_num_pieces(mi.Length(), target))
        old = np.concatenate([mi.PieceSums() for _, mi, _ in todo] + [np.zeros(0, np.uint32)]).astype(np.uint32)
        offs = [int(x.out_offset) for x in arr]
        counts = [int(lib.krk_num_pieces(mi.Length(), target)) for _, mi, target in todo]
        pls, lens, hexes = [t for *_, t in todo], [mi.Length() for _, mi, _ in todo], [name for name, *_ in todo]
        u32p = C.POINTER(C.c_uint32)
        out = np.zeros(max(b, 1), dtype=np.uint32)
        check(lib.krk_repiece_batch(arr, n, old.ctypes.data_as(u32p) if old.size else None, out.ctypes.data_as(u32p)))
        ihs = core._info_hash_batch(pls, out, offs, counts, hexes, lens)
        return [(out[o:o + c].copy() if c else None, ih) for o, c, ih in zip(offs, counts, ihs)]

    def _repiece_chain_dev(self, names, sizes, targets) -> dict:
        """{name: the new sidecar's bytes} of the blobs repiece_sidecars_dev re-pieces from the
        stored sidecars' bytes; a blob without a readable sidecar is not among them."""
        entries = []
        for name, size, target in zip(names, sizes, targets):
            try:
                entries.append((name, size, target, self.cas.GetCacheFileMetadata(name)))
            except OSError:
                continue
        return repiece_sidecars_dev(entries)

    def VerifyAll(self, batch_bytes: int = 8 << 30, check_digest: bool = True) -> dict:
        """The read-only counterpart of RegenerateAll: every cached blob against the
        _torrentmeta already stored for it.  Nothing is written, renamed or deleted.

        Each sidecar is loaded with DeserializeMetaInfo; found without reading data: no sidecar
        (reason ``missing_meta``), one that does not parse or cannot describe the file
        (``bad_meta``, with the ``error`` text), a stored Name that is not the directory's
        (``name``), a stored Length that is not the stat size (``length``).  The rest go through
        krk_verify_files in batches of ~batch_bytes, with the STORED piece length and sums (not
        the config's) and, with check_digest, the blob's name as its SHA-256: reason ``pieces``
        with the mismatching piece indices, or ``digest`` when every piece sum agrees and the
        digest does not -- a sidecar regenerated over rotten bytes.  Returns {"blobs": n,
        "ok": k, "corrupt": [{"name", "reason", "bad_pieces", "digest_ok"}]} sorted by name."""
        from . import device as D
        from ._capi import KrakenError
        names = self.cas.ListNames()
        corrupt, batch, size = [], [], 0

        def entry(name, reason, bad_pieces=(), digest_ok=None, **more):
            corrupt.append({"name": name, "reason": reason, "bad_pieces": [int(x) for x in bad_pieces],
                            "digest_ok": digest_ok, **more})

        def flush():
            nonlocal batch, size
            if not batch:
                return
            exp = np.concatenate([mi.PieceSums() for _, mi in batch] + [np.zeros(0, np.uint32)])
            dg = (np.frombuffer(b"".join(bytes.fromhex(name) for name, _ in batch), dtype=np.uint8)
                  if check_digest else None)
            try:
                bits, woff, bad, ok = D.verify_files([self.cas.GetCacheFilePath(name) for name, _ in batch],
                                                     [mi.Length() for _, mi in batch],
                                                     [mi.PieceLength() for _, mi in batch], exp, dg)
            except KrakenError as e:
                if e.code == KRK_EIO:
                    raise IOError(f"verify: {e}") from None
                raise
            for k, (name, mi) in enumerate(batch):
                dig_ok = bool(ok[k]) if ok is not None else None
                if bad[k]:
                    good = D.bitfield_bools(bits[int(woff[k]):int(woff[k + 1])], mi.NumPieces())
                    entry(name, "pieces", np.flatnonzero(~good), dig_ok)
                elif dig_ok is False:
                    entry(name, "digest", (), False)
            batch, size = [], 0

        for name in names:
            try:
                raw = self.cas.GetCacheFileMetadata(name)
            except FileNotFoundError:
                entry(name, "missing_meta")
                continue
            try:
                mi = core.DeserializeMetaInfo(raw)
            except ValueError as e:
                entry(name, "bad_meta", error=str(e))
                continue
            if mi.Digest().Hex() != name:
                entry(name, "name")
                continue
            st_size = self.cas.GetCacheFileStat(name).st_size
            if mi.Length() != st_size:
                entry(name, "length")
                continue
            if mi.PieceLength() <= 0:
                entry(name, "bad_meta", error="piece length must be positive")
                continue
            want = int(lib.krk_num_pieces(st_size, mi.PieceLength()))
            if mi.NumPieces() != want:
                entry(name, "bad_meta", error=f"{mi.NumPieces()} piece sums for {want} pieces")
                continue
            batch.append((name, mi))
            size += st_size
            if size >= batch_bytes:
                flush()
        flush()
        corrupt.sort(key=lambda c: c["name"])
        return {"blobs": len(names), "ok": len(names) - len(corrupt), "corrupt": corrupt}

    def GenerateBatch(self, digests) -> list[core.MetaInfo]:
        """Generate for many cache files in one pipelined GPU pass.  When the CAS
        exposes file paths (DirCAS.GetCacheFilePath) the files are read by the
        library's host threads straight into pinned staging windows
        (krk_piece_sums_files); otherwise through GetCacheFileReader into host
        memory (krk_piece_sums_host).  Errors carry Generate's prefixes
        (generator.go:41-58)."""
        if hasattr(self.cas, "GetCacheFilePath"):
            metas, off = [], 0
            for d in digests:
                try:
                    size = self.cas.GetCacheFileStat(d.Hex()).st_size
                except OSError as e:
                    raise IOError(f"cache stat: {e}") from None
                pl = self.pieceLengthConfig.get(size)
                metas.append((d, size, pl, off))
                off += int(lib.krk_num_pieces(size, pl))
            paths = [os.fsencode(self.cas.GetCacheFilePath(d.Hex())) for d, *_ in metas]
            arr = (krk_file_blob * max(len(metas), 1))()
            for i, ((d, size, pl, o), path) in enumerate(zip(metas, paths)):
                arr[i] = krk_file_blob(path, size, pl, o)
            sums = np.zeros(max(off, 1), dtype=np.uint32)
            rc = lib.krk_piece_sums_files(arr, len(metas), sums.ctypes.data_as(C.POINTER(C.c_uint32)))
            if rc == KRK_EIO:
                raise IOError(f"create metainfo: {lib.krk_last_error().decode()}")
            check(rc)
        else:
            datas, metas, off = [], [], 0
            for d in digests:
                try:
                    f = self.cas.GetCacheFileReader(d.Hex())
                except OSError as e:
                    raise IOError(f"get cache file: {e}") from None
                with f:
                    b = np.frombuffer(f.read(), dtype=np.uint8)
                pl = self.pieceLengthConfig.get(b.size)
                datas.append(b)
                metas.append((d, b.size, pl, off))
                off += int(lib.krk_num_pieces(b.size, pl))
            arr = (krk_blob * max(len(metas), 1))()
            for i, (b, (d, size, pl, o)) in enumerate(zip(datas, metas)):
                arr[i] = krk_blob(b.ctypes.data if b.size else None, size, pl, o)
            sums = np.zeros(max(off, 1), dtype=np.uint32)
            check(lib.krk_piece_sums_host(arr, len(metas), sums.ctypes.data_as(C.POINTER(C.c_uint32))))
        out = []
        self._last_changed = 0
        counts = [int(lib.krk_num_pieces(size, pl)) for _, size, pl, _ in metas]
        ihs = core._info_hash_batch([pl for _, _, pl, _ in metas], sums, [o for *_, o in metas], counts,
                                    [d.Hex() for d, *_ in metas], [size for _, size, _, _ in metas])
        for (d, size, pl, o), n, ih in zip(metas, counts, ihs):
            s_ = sums[o:o + n].copy() if n else None
            mi = core.MetaInfo(pl, s_, d.Hex(), size, d, ih)
            try:
                self._last_changed += bool(self.cas.SetCacheFileMetadata(d.Hex(), mi))
            except OSError as e:
                raise IOError(f"set metainfo: {e}") from None
            out.append(mi)
        return out

    def VerifyAndGenerateBatch(self, uploads):
        """Fused upload verification + metainfo generation.

        The reference reads every uploaded blob twice: uploader.verify digests it
        (origin/blobserver/uploader.go:74-94, error "computed digest %s doesn't
        match parameter %s") and Generate later re-reads the committed cache file
        for the piece sums (generator.go:41-58).  Here one host->device pass over
        each blob (krk_metainfo_digest_host) yields both.  uploads: [(core.Digest
        expected, bytes-like data)].  Verified blobs are committed to the CAS with
        their _torrentmeta; returns [MetaInfo | ValueError] in input order."""
        from . import device as D
        datas = [np.frombuffer(memoryview(b), dtype=np.uint8) for _, b in uploads]
        pls = [self.pieceLengthConfig.get(int(x.size)) for x in datas]
        sums, dg = D.metainfo_digest_host(datas, pls)
        out = []
        for (want, _), x, pl, s, g in zip(uploads, datas, pls, sums, dg):
            got = core.NewSHA256DigestFromHex(bytes(g).hex())
            if got != want:
                out.append(ValueError(f"computed digest {got.String()} doesn't match parameter {want.String()}"))
                continue
            d = self.cas.WriteCacheFileAs(want, x)
            out.append((d, pl, s.copy() if s.size else None, int(x.size)))
        return self._commit_metainfo(out)

    def VerifyAndGenerateUploads(self, uploads):
        """The same from the upload FILES, as the origin holds them (uploader.verify reads
        the upload file, origin/blobserver/uploader.go:74-94; commit moves it into the
        cache, :96-105; Generate re-reads the cache file, generator.go:41-58): each file is
        read once by krk_metainfo_digest_files and that read yields the digest AND the piece
        sums.  uploads: [(core.Digest expected, upload file path)].  A file that cannot be
        read fails the batch with uploader.verify's prefixes ("get upload file: ...",
        "calculate digest: read blob: <path>: ..."); a digest mismatch is that upload's
        ValueError; verified files are moved into the CAS with their _torrentmeta.  A verified
        upload whose blob is already cached -- or an earlier upload of the same batch put it
        there -- is that upload's FileExistsError (uploader.commit's 409, uploader.go:96-104),
        its upload file deleted as the reference does, and the batch goes on.  Returns
        [MetaInfo | ValueError | FileExistsError] in input order."""
        from . import device as D
        from ._capi import KrakenError
        paths, sizes = [], []
        for _, p in uploads:
            try:
                sizes.append(os.stat(p).st_size)
            except OSError as e:
                raise IOError(f"get upload file: {e}") from None
            paths.append(p)
        pls = [self.pieceLengthConfig.get(n) for n in sizes]
        try:
            sums, dg = D.metainfo_digest_files(paths, sizes, pls)
        except KrakenError as e:
            raise IOError(f"calculate digest: {e}") from None
        out = []
        for (want, p), n, pl, s, g in zip(uploads, sizes, pls, sums, dg):
            got = core.NewSHA256DigestFromHex(bytes(g).hex())
            if got != want:
                out.append(ValueError(f"computed digest {got.String()} doesn't match parameter {want.String()}"))
                continue
            try:
                self.cas.MoveUploadFileToCache(p, want.Hex())
            except FileExistsError as e:
                out.append(e)  # 409 Conflict for this upload only
                continue
            out.append((want, pl, s.copy() if s.size else None, int(n)))
        return self._commit_metainfo(out)

    def _commit_metainfo(self, out):
        """The committed uploads' InfoHashes in one batched call and their sidecars (entries
        that are errors -- digest mismatch, conflict -- pass through)."""
        ok = [k for k, o in enumerate(out) if isinstance(o, tuple)]
        if ok:
            flat = [out[k][2] for k in ok if out[k][2] is not None]
            allsums = np.concatenate(flat) if flat else np.zeros(0, np.uint32)
            counts = [0 if out[k][2] is None else out[k][2].size for k in ok]
            offs = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
            ihs = core._info_hash_batch([out[k][1] for k in ok], allsums, offs, counts,
                                        [out[k][0].Hex() for k in ok], [out[k][3] for k in ok])
            for k, ih in zip(ok, ihs):
                d, pl, s, size = out[k]
                mi = core.MetaInfo(pl, s, d.Hex(), size, d, ih)
                self.cas.SetCacheFileMetadata(d.Hex(), mi)
                out[k] = mi
        return out


def New(config: dict, cas) -> Generator:
    return Generator(config, cas)


def _parse_config(text: str) -> dict:
    """"0:4194304,2147483648:8388608" -> {0: 4194304, 2147483648: 8388608}."""
    out = {}
    for part in text.split(","):
        a, b = part.split(":")
        out[int(a)] = int(b)
    return out


def main(argv=None) -> int:
    """python -m kraken_amd.metainfogen <cache dir> [--piece-lengths 0:4194304]:
    regenerate every _torrentmeta of a CAS cache directory on the GPU.  With --verify
    [--no-digest] nothing is written: every blob is checked against its stored _torrentmeta
    (and its name, unless --no-digest), the report is printed and the exit code is 1 when
    anything is corrupt.  With --repiece [--repiece-placement gpu] the sidecars are brought to
    --piece-lengths from their stored sums wherever the stored piece length divides the new one
    (no blob byte read), the other blobs are reread, and the report is printed."""
    import argparse
    import json
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("cache_dir")
    ap.add_argument("--piece-lengths", default="0:4194304",
                    help="size:pieceLength ranges (config/origin/base.yaml:24-26 default: 0:4MB)")
    ap.add_argument("--batch-gib", type=int, default=8)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--verify", action="store_true",
                    help="read-only: check every blob against its stored _torrentmeta (Generator.VerifyAll)")
    ap.add_argument("--no-digest", action="store_true", help="with --verify: piece sums only, no SHA-256 pass")
    ap.add_argument("--repiece", action="store_true",
                    help="bring every _torrentmeta to --piece-lengths from the stored sums where the stored piece "
                         "length divides the new one, reading only the other blobs (Generator.RepieceAll)")
    ap.add_argument("--repiece-placement", choices=("host", "gpu"), default="host",
                    help="with --repiece: where the stored sums are re-pieced")
    a = ap.parse_args(argv)
    from . import device
    from ._capi import KRK_ENODEV, KrakenError
    try:
        device.set_device(a.device)
    except KrakenError as e:
        # the piece-sum scrub and the host re-piece run on the host CRC placement where there is
        # no device
        if not (e.code == KRK_ENODEV and ((a.verify and a.no_digest) or
                                          (a.repiece and a.repiece_placement == "host"))):
            raise
    g = New(_parse_config(a.piece_lengths), DirCAS(a.cache_dir))
    if a.repiece:
        print(json.dumps(g.RepieceAll(a.repiece_placement, a.batch_gib << 30)))
        return 0
    if a.verify:
        report = g.VerifyAll(a.batch_gib << 30, check_digest=not a.no_digest)
        print(json.dumps(report))
        return 1 if report["corrupt"] else 0
    print(json.dumps(g.RegenerateAll(a.batch_gib << 30)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
