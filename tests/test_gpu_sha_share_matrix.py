"""GPU parity: the SHA-256 host share and the tail handoff of krk_sha256_dev and
krk_metainfo_digest_dev (offload.cpp, batch_dev.cpp) at their edges, bit for bit against hashlib
and zlib.  The cases, their injected planner rates and their required plans are
tests/sha_share_matrix.py's; tests/test_sha_share_plan_cpu.py proves without a device that the
planner gives each case its plan and that every named edge is among them.  Here each case runs,
krk_sha_last_tail is compared with the plan, and the whole digest and sums buffers -- canary rows
included -- with the expectations.

No call in this file waits for the whole device: the copies of a run's output buffers into pinned
host memory are queued on the stream the run was queued on and that stream alone is awaited
(krk_stream_sync), so an output that some other stream of the library still has to write shows."""
import ctypes as C
import os
import subprocess
import sys
import threading
import time

import pytest

from kraken_amd import device as D
from kraken_amd._capi import check, lib
from tests import sha_share_matrix as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built(gpu):
    """build(case), once a module for every distinct data layout (the whole-blob cases share one)."""
    cache = {}

    def get(case):
        key = (tuple(case.lens), case.aligns, case.piece_lengths)
        if key not in cache:
            cache[key] = M.build(case)
        return cache[key]._replace(case=case)

    yield get
    for b in cache.values():
        b.buf.free()


def run_case(b, stream=None, sha_plan=0):
    """Both entry points over the built case on `stream` (metainfo_digest at each piece length),
    each awaited on that stream alone and compared in full."""
    case = b.case
    with M.settings(case, sha_plan=sha_plan):
        for fn, P in [(M.sha256_call, None)] + [(M.metainfo_digest_call, P) for P in case.piece_lengths]:
            out = M.Outputs(b, P)
            try:
                fn(b, out, stream)
                out.read_back(stream)
                check(lib.krk_stream_sync(stream))
                assert D.sha_last_tail() == M.last_tail_of(case), (case.name, fn.__name__, D.sha_last_tail())
                out.check((fn.__name__, P, sha_plan))
            finally:
                out.free()


@pytest.mark.parametrize("case", M.TAIL_CASES, ids=lambda c: c.name)
def test_tail_handoff_case(built, case):
    """Block edges (prefixes of one block and more; tails of 1, 55, 56, 63, 64, 65 bytes), chunk
    edges (tails of C - 64 .. 3 C + 1, the last wrapping the two-buffer ring), takeovers queued in
    another order than their note slots with more of them than threads, every ptr % 16."""
    run_case(built(case))


@pytest.mark.parametrize("case", M.FALLBACK_CASES, ids=lambda c: c.name)
def test_threads_at_or_above_the_takeovers(built, case):
    """With a thread for every chain a plan would take, no chain is handed over mid-way: whole
    blobs, or no share at all; krk_sha_last_tail reports 0 chains."""
    assert M.last_tail_of(case)["chains"] == 0
    run_case(built(case))


@pytest.mark.parametrize("sha_plan", [1, 2, 3, 4, 5, 6])
def test_midstate_note_under_every_launch_plan(built, sha_plan):
    """The smallest block-edge case under each production launch plan: every kernel body writes
    the midstate of a non-final stream to the note."""
    run_case(built(M.BY_NAME[M.SMALLEST_BLOCK_EDGE]), sha_plan=sha_plan)


@pytest.mark.parametrize("case", M.WHOLE_CASES, ids=lambda c: c.name)
def test_whole_blob_share(built, case):
    """Whole blobs of C - 1 .. 4 C + 13 bytes (1, 2, 3 and more copy chunks: the ring filled once
    and wrapped) on 1, 3 and more threads than host blobs, beside 204 chains the GPU keeps."""
    run_case(built(case))


@pytest.fixture
def stream(gpu):
    s = C.c_void_p()
    check(lib.krk_stream_create(C.byref(s)))
    yield s
    check(lib.krk_stream_sync(s))
    check(lib.krk_stream_destroy(s))


STREAM_CASES = [M.BY_NAME["q-t2"], M.BY_NAME["c-C-1-C-64"], M.BY_NAME["w-t3"], M.GPU_LONG_CASE]


@pytest.mark.parametrize("case", STREAM_CASES, ids=lambda c: c.name)
def test_callers_stream_alone_orders_the_outputs(built, stream, case):
    """Tail cases and whole-blob cases on a stream of the caller's, awaited with krk_stream_sync
    of that stream only: the host share's scatter, the GPU part on the library's streams and the
    piece CRCs have all been joined into it.  In w-gpu-long the host share ends tens of ms before
    the GPU's chains, so the call returns with the library's streams still running."""
    run_case(built(case), stream=stream)


@pytest.mark.parametrize("case", STREAM_CASES, ids=lambda c: c.name)
def test_two_calls_back_to_back_on_one_stream(built, stream, case):
    """Two calls queued one after the other on the caller's stream into different output buffers,
    one krk_stream_sync after both."""
    b = built(case)
    P = case.piece_lengths[0]
    with M.settings(case):
        for fns in ((M.sha256_call, M.metainfo_digest_call), (M.metainfo_digest_call, M.metainfo_digest_call)):
            outs = [M.Outputs(b, None if fn is M.sha256_call else P) for fn in fns]
            try:
                for fn, out in zip(fns, outs):
                    fn(b, out, stream)
                    assert D.sha_last_tail() == M.last_tail_of(case)
                for out in outs:
                    out.read_back(stream)
                check(lib.krk_stream_sync(stream))
                for fn, out in zip(fns, outs):
                    out.check(("back to back", fn.__name__))
            finally:
                for out in outs:
                    out.free()


def test_concurrent_callers(built):
    """Two threads with a stream each run a tail batch (two host threads a call) while a third
    runs a whole-blob batch, two rounds: every output equals the serial expectation, and each
    thread's krk_sha_last_tail is its own call's."""
    cases = [M.BY_NAME["q-t2"], M.BY_NAME["c-C-1-C-64"], M.BY_NAME["f-t2"]]
    assert all(c.threads == 2 and c.rates == cases[0].rates for c in cases)  # the knobs are process-wide
    assert cases[0].tails and cases[1].tails and cases[2].whole
    bs = [built(c) for c in cases]
    errors = []
    gate = threading.Barrier(len(cases))

    def worker(b):
        try:
            D.set_device(0)
            s = C.c_void_p()
            check(lib.krk_stream_create(C.byref(s)))
            try:
                for rnd in range(2):
                    gate.wait(timeout=60)
                    for fn, P in ((M.sha256_call, None), (M.metainfo_digest_call, b.case.piece_lengths[0])):
                        out = M.Outputs(b, P)
                        try:
                            fn(b, out, s)
                            out.read_back(s)
                            check(lib.krk_stream_sync(s))
                            assert D.sha_last_tail() == M.last_tail_of(b.case), (b.case.name, D.sha_last_tail())
                            out.check(("concurrent", rnd, fn.__name__))
                        finally:
                            out.free()
            finally:
                check(lib.krk_stream_sync(s))
                check(lib.krk_stream_destroy(s))
        except BaseException as e:  # noqa: BLE001 -- reported by the test's thread
            errors.append((b.case.name, repr(e)))
            gate.abort()

    with M.settings(cases[0]):
        threads = [threading.Thread(target=worker, args=(b,)) for b in bs]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    assert not errors, errors


def test_pooled_worker_sets_grow_and_shrink(built):
    """Consecutive calls of one thread on 2, then 4, then 1 host threads: the pooled worker set is
    taken, grown, and used in part; each call is correct."""
    assert [c.threads for c in M.POOL_CASES] == [2, 4, 1]
    for case in M.POOL_CASES:
        run_case(built(case))


def _child(which, limit):
    t0 = time.monotonic()
    p = subprocess.run([sys.executable, "-m", "tests.sha_share_child", which], cwd=ROOT, timeout=limit,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    wall = time.monotonic() - t0
    assert p.returncode == 0 and ("ok " + which) in p.stdout, (which, p.returncode, p.stdout[-2000:])
    return wall


def test_sentinel_collision_takes_the_gpu_done_branch():
    """A true midstate word equal to the note's fill (tests/golden/sha_sentinel_block.json): the
    host cannot see the midstate as written and waits for the launch's end instead
    (offload_hash, `gpu_done`).  tests/sha_share_child.py runs the block-edge batch with that
    block as the handed-over chain's GPU prefix in a process of its own; digests and sums equal
    hashlib's and zlib's.  Its time limit is 20 x the wall time of the same child with the control
    block (no fill word in its midstate), so a wait that never ends fails here.

    Measured on an MI355X: the control child 0.29 s wall (process start, library load, both
    calls), so a limit of 5.9 s; the collision child 0.53 s.  A build that refuses a midstate
    still holding a fill word after the launch's end fails the collision child and no other test
    of this file: the input does take that branch."""
    control = _child("control", 120)
    limit = 20 * control
    collision = _child("collision", limit)
    print(f"sentinel child: control {control:.2f} s, limit {limit:.1f} s, collision {collision:.2f} s")
