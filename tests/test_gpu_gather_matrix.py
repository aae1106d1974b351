"""GPU parity: the host gather kernel (gather.hip) at its funnel, lane, unroll, stride and tile
edges through krk_gather_spans_dev, byte for byte against the page-locked source and with every
byte beside the gathered ones still canary (the cases, the expected image and the comparison
live in tests/gather_matrix.py), and the hook's refusals: nothing launched, nothing written."""
import ctypes as C

import numpy as np
import pytest

from kraken_amd import _capi
from kraken_amd import device as D
from kraken_amd._capi import lib
from tests import gather_matrix as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device(gpu):
    b = M.DeviceBackend()
    yield b
    b.close()


@pytest.mark.parametrize("group", M.GROUPS)
def test_gather_matrix_group(device, group):
    n, bad = M.run_group_counted(group, device)
    assert n > 0
    assert bad == [], f"group {group}: {len(bad)} spans or stray bytes of {n} spans differ, first {bad[:5]}"


def test_one_launch_a_call_and_the_tile_stride(device):
    """Group A is ONE launch of more tiles than the grid has workgroups."""
    spans, size, calls, image, mask = device.want("A")
    with D.KernelTimer():
        got = device.run("A")
        launches = D.KernelTimer.stats("host_gather")[0]
        units = [u for _, u, _, _ in D.KernelTimer.timeline("host_gather")]
    assert launches == 1 and units == [M.n_tiles(spans)] and units[0] > max(64, D.device_cus())
    assert M.compare("A", spans, got, image, mask) == []


def test_refusals_launch_nothing_and_write_nothing(device):
    size = 4096 + 48  # no multiple of a page: the bytes after it belong to no allocation
    buf = D.DeviceBuffer(size)
    canary = np.full(size, M.CANARY, dtype=np.uint8)
    buf.from_host(canary)
    good = M.Span(5, 100, 0)
    pageable = np.arange(256, dtype=np.uint8)
    vpp, u64p = C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)

    def call(src, dst, n):
        a, b, c = (np.array(x, dtype=np.uint64) for x in (src, dst, n))
        return lib.krk_gather_spans_dev(a.ctypes.data_as(vpp), b.ctypes.data_as(vpp), c.ctypes.data_as(u64p), a.size,
                                        None)

    ok_src, ok_dst = device.arena.ptr + good.src, buf.ptr
    refused = {
        "a pageable source": ([ok_src, pageable.ctypes.data], [ok_dst, ok_dst + 256], [good.n, 100]),
        "a dst at +8": ([ok_src, ok_src], [ok_dst, ok_dst + 256 + 8], [good.n, 100]),
        "a dst whose rounded end lies past its allocation": ([ok_src, ok_src], [ok_dst, ok_dst + size - 16],
                                                             [good.n, 17]),
    }
    try:
        with D.KernelTimer():
            for what, (src, dst, n) in refused.items():
                assert call(src, dst, n) == _capi.KRK_EINVAL, what
                assert b"gather_spans_dev" in lib.krk_last_error(), what
                D.synchronize()
                assert D.KernelTimer.stats("host_gather")[0] == 0, what  # the good span before it did not run either
                assert np.array_equal(buf.to_host(np.uint8, size), canary), what
            # the same calls' good halves are accepted: the refusals above were about the bad span
            assert call([ok_src], [ok_dst], [good.n]) == _capi.KRK_OK
            assert call([0, ok_src], [ok_dst + 256, ok_dst + 256], [0, 17]) == _capi.KRK_OK  # n == 0: src NULL
            assert call([], [], []) == _capi.KRK_OK
            D.synchronize()
            assert D.KernelTimer.stats("host_gather")[0] == 2
        got = buf.to_host(np.uint8, size)
        want = canary.copy()
        want[:good.n] = device.host[good.src:good.src + good.n]
        want[256:256 + 17] = device.host[good.src:good.src + 17]
        keep = np.ones(size, dtype=bool)
        keep[good.n:M.roundup16(good.n)] = False
        keep[256 + 17:256 + 32] = False
        assert np.array_equal(got[keep], want[keep])
    finally:
        buf.free()
