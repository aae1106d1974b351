"""krk_info_hash_batch_dev past one job a workgroup: 2^20 + 65 jobs in one call, so 65
workgroups of info_hash.hip run a second job over the ring, pos, done and h of their first;
the whole (n, 20) output, written to page-locked memory, against hashlib.sha1 over a bencode
written in tests/info_hash_stride.py (tests/test_info_hash_stride_cpu.py proves the cases)."""
import time

import numpy as np
import pytest

from kraken_amd import device as D
from tests import info_hash_stride as S

pytestmark = pytest.mark.gpu


def test_second_job_of_a_workgroup(gpu):
    n = S.N_JOBS
    t0 = time.perf_counter()
    want = S.expected(n)
    ln, pl = S.fields(n)
    sums = D.DeviceBuffer(4 * len(S.SUMS))
    sums.from_host(np.array(S.SUMS, dtype=np.uint32))
    out = D.PinnedArray((n, 20), np.uint8)
    out.a[:] = 0xFF
    zeros, three = np.zeros(n, dtype=np.uint64), np.full(n, len(S.SUMS), dtype=np.uint64)
    t1 = time.perf_counter()
    with D.KernelTimer():
        assert D.info_hash_batch_dev(pl, sums, zeros, three, None, ln, out=out) is out
        t2 = time.perf_counter()
        D.synchronize()
        t3 = time.perf_counter()
        launches, ms = D.KernelTimer.stats("info_hash")
        units = [u for _, u, _, _ in D.KernelTimer.timeline("info_hash")]
    print(f"info_hash stride: reference {t1 - t0:.3f} s, call {t2 - t1:.3f} s, wait {t3 - t2:.3f} s, kernel {ms:.3f} ms")
    assert launches == 1 and units == [n]
    sums.free()
    same = np.array_equal(out.a, want)
    rows = [] if same else np.nonzero((out.a != want).any(axis=1))[0]
    assert same, f"{len(rows)} of {n} digests differ, first rows {rows[:8].tolist()} (a second job starts at row {S.MAX_GRID})"
