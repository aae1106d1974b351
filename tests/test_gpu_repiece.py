"""Stored MetaInfo re-pieced on the device: Generator.RepieceAll(placement="gpu")
(krk_repiece_batch_dev then krk_info_hash_batch_dev on one stream, one copy back) against the
host placement and against RegenerateAll, and one C4-sized blob's stored sums re-pieced and
InfoHashed on the device against the host path."""
import ctypes as C
import shutil

import numpy as np
import pytest

from kraken_amd import _capi, core, device as D, metainfogen
from kraken_amd._capi import check, lib
from tests import repiece_cache as RC

pytestmark = pytest.mark.gpu


def test_repiece_all_gpu_placement_matches_host_and_regenerate_all(gpu, tmp_path):
    roots = {k: str(tmp_path / k) for k in ("gpu", "host", "regen")}
    cas, names = RC.build_cache(roots["gpu"])
    shutil.copytree(roots["gpu"], roots["host"])
    shutil.copytree(roots["gpu"], roots["regen"])
    for n in names:  # no blob byte may be read: zeros of the same size
        RC.zero_data(cas, n)
    with D.KernelTimer():
        report = metainfogen.New(RC.NEW, cas).RepieceAll(placement="gpu")
        D.synchronize()
        assert D.KernelTimer.stats("piece_repiece")[0] == 1 and D.KernelTimer.stats("info_hash")[0] == 1
        assert D.KernelTimer.stats("crc32_pieces")[0] == 0
    assert report == {"blobs": 12, "unchanged": 0, "repieced": 12, "reread": 0, "changed": 12,
                      "bytes_not_read": sum(RC.SIZES)}
    host = metainfogen.DirCAS(roots["host"])
    assert metainfogen.New(RC.NEW, host).RepieceAll(placement="host") == report
    regen = metainfogen.DirCAS(roots["regen"])
    assert metainfogen.New(RC.NEW, regen).RegenerateAll() == {"blobs": 12, "changed": 12}
    want = RC.sidecars(regen)
    assert RC.sidecars(cas) == want and RC.sidecars(host) == want
    # the command line on the GPU placement: everything is at its target already
    assert metainfogen.main([roots["gpu"], "--repiece", "--repiece-placement", "gpu", "--piece-lengths",
                             "0:262144,524288:1048576"]) == 0


def test_c4_sized_blob_repieced_and_info_hashed_on_the_device(gpu):
    """81,920 stored sums at 256 KiB (a 20 GiB blob; synthetic sums, no bytes) to 4 MiB: 5,120 sums
    and their InfoHash from the device, against krk_repiece_sums and the host InfoHash."""
    po, pn, n_old = 256 << 10, 4 << 20, 81_920
    length = n_old * po - 12_345
    old = np.random.default_rng(20261022).integers(0, 1 << 32, size=n_old, dtype=np.uint64).astype(np.uint32)
    name = "c4" * 32
    stored = core.MetaInfo(po, old, name, length, core.NewSHA256DigestFromHex(name), core._info_hash(po, old, name, length))
    want = stored.Repiece(pn)
    assert want.NumPieces() == 5_120
    d_old, d_out = D.DeviceBuffer(old.nbytes), D.DeviceBuffer(4 * 5_120)
    d_old.from_host(old)
    d_out.from_host(np.full(5_120, 0xFFFFFFFF, dtype=np.uint32))
    blob = _capi.krk_repiece_blob(length, po, pn, 0, 0)
    check(lib.krk_repiece_batch_dev(C.byref(blob), 1, d_old.ptr, d_out.ptr, None))
    ih = D.info_hash_batch_dev([pn], d_out, [0], [5_120], [name], [length])
    assert np.array_equal(d_out.to_host(np.uint32, 5_120), want.PieceSums())
    assert bytes(ih[0]) == want.InfoHash().Bytes()
