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
