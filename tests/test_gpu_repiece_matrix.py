"""GPU parity: the re-piece kernel (piece_repiece.hip) at its segment, stride-pass, owner-search,
wave-stride, sums-layout and 64-bit distance edges through krk_repiece_batch_dev, every output
word against zlib.crc32 (group F: the plain-Python GF(2) reference) and against the host form's
bytes (the cases and the comparison live in tests/repiece_matrix.py; tests/test_repiece_matrix_cpu.py
proves them on the host forms)."""
import ctypes as C

import numpy as np
import pytest

from kraken_amd import _capi, device as D
from kraken_amd._capi import lib
from tests import repiece_matrix as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device(gpu):
    return M.DeviceBackend()


@pytest.mark.parametrize("group", M.GROUPS)
def test_repiece_matrix_group(device, group):
    n, bad = M.run_group_counted(group, device)
    assert n > 0
    assert bad == [], f"group {group}: {len(bad)} sums or stray words of {n} blobs differ, first {bad[:5]}"


@pytest.mark.parametrize("group", M.GROUPS)
def test_repiece_matrix_group_into_page_locked_outputs(device, group):
    n, bad = M.run_group_counted(group, device, pinned=True)
    assert n > 0
    assert bad == [], f"group {group}: {len(bad)} sums or stray words of {n} blobs differ, first {bad[:5]}"


@pytest.mark.parametrize("group", M.GROUPS)
def test_device_bytes_equal_the_host_form(device, group):
    host = M.HostBackend()
    for b in M.batches(group, device.host):
        dev_out, host_out = device.outputs(b), host.outputs(b)
        assert np.array_equal(device.call(b, dev_out), host.call(b, host_out)), b.label


def test_one_launch_a_call_and_the_wave_stride(device):
    """Group D is ONE launch of more units than the grid has waves."""
    b = M.batch_d(device.host)
    out = device.outputs(b)
    with D.KernelTimer():
        got = device.call(b, out)
        launches = D.KernelTimer.stats("piece_repiece")[0]
        units = [u for _, u, _, _ in D.KernelTimer.timeline("piece_repiece")]
    assert launches == 1 and units == [b.units] and units[0] > M.STRIDE_UNITS
    assert M.compare("D", b, got) == []


def test_refusals_launch_nothing_and_write_nothing(device):
    old = D.DeviceBuffer(4 * 64)
    old.from_host(np.arange(64, dtype=np.uint32))
    out = D.DeviceBuffer(4 * 64)
    canary = np.full(64, M.CANARY, dtype=np.uint32)
    out.from_host(canary)
    pageable = np.full(64, M.CANARY, dtype=np.uint32)
    pinned = D.PinnedArray((64,), np.uint32)
    pinned.a[:] = np.arange(64, dtype=np.uint32)
    good = M.refusal_batch((100, 16, 32))

    def call(blobs, sums, dst):
        return lib.krk_repiece_batch_dev(blobs.ctypes.data_as(M.blobp), blobs.size, sums, dst, None)

    with D.KernelTimer():
        for what, row, code, text in M.refusals():
            assert call(M.refusal_batch(row), old.ptr, out.ptr) == code, what
            assert text is None or lib.krk_last_error().decode() == text, what
        # a pageable output, a pageable input: KRK_EINVAL by the pointer check, before a launch
        assert call(good, old.ptr, pageable.ctypes.data) == _capi.KRK_EINVAL
        assert b"repiece_batch_dev" in lib.krk_last_error()
        assert call(good, pageable.ctypes.data, out.ptr) == _capi.KRK_EINVAL
        assert call(good, None, out.ptr) == _capi.KRK_EINVAL
        D.synchronize()
        assert D.KernelTimer.stats("piece_repiece")[0] == 0
        assert np.array_equal(out.to_host(np.uint32, 64), canary) and (pageable == M.CANARY).all()
        # the accepted neighbours: page-locked sums in, an empty batch, a batch of empty blobs (no launch)
        assert call(good, pinned.ptr, out.ptr) == _capi.KRK_OK
        assert lib.krk_repiece_batch_dev(None, 0, None, None, None) == _capi.KRK_OK
        empty = M.refusal_batch((0, 16, 32))[1:2]
        assert call(empty, None, None) == _capi.KRK_OK
        D.synchronize()
        assert D.KernelTimer.stats("piece_repiece")[0] == 1
    want = canary.copy()
    host_out = canary.copy()
    _capi.check(lib.krk_repiece_batch(good.ctypes.data_as(M.blobp), 3, pinned.a.ctypes.data_as(M.u32p),
                                      host_out.ctypes.data_as(M.u32p)))
    assert (host_out != want).sum() == 2 + 4 + 1
    assert np.array_equal(out.to_host(np.uint32, 64), host_out)
