"""GPU parity: the verify kernels (piece_bitfield.hip) at their word, count-loop, stride,
owner-search, sums-layout and digest-dword edges through krk_verify_batch_dev, every word, count
and flag against numpy.packbits, zlib and hashlib (the cases and the comparison live in
tests/verify_matrix.py; tests/test_verify_matrix_cpu.py proves them on the host packer)."""
import pytest

from tests import verify_matrix as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device(gpu):
    b = M.DeviceBackend()
    yield b
    b.close()


@pytest.mark.parametrize("group", M.GROUPS)
def test_verify_matrix_group(device, group):
    n, bad = M.run_group_counted(group, device)
    assert n > 0
    assert bad == [], f"group {group}: {len(bad)} words, counts or flags of {n} blobs differ, first {bad[:5]}"
