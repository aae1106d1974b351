"""The O_DIRECT window reads of the file batches (direct_read.hpp, par_read and AioReader of staging.hpp, FileSource of
window_pass.cpp) on both of their paths, whichever of the two this machine takes by itself.

Where the pinned windows accept the disk's DMA nothing is ever refused, and the bounce loop, the AIO reaper's re-read
and the hand-over of later windows to the read threads never run; where they refuse it (a GPU passed through to a
virtual machine) the zero-copy path and the AIO path beyond its first window never run.  So every refused case runs in
a fresh child process under the diag library with KRK_DIRECT_REFUSE=N: from the N-th O_DIRECT read aimed at a window
each one is refused as the real refusal is -- EFAULT, no byte of the file in the window (an AIO request's range is
overwritten with a filler, so a re-read that is skipped or lands elsewhere gives a wrong digest).  The switch to the
bounce buffer is process-wide and permanent, hence the children (tests/window_matrix.py, `reads`).  Expected values are
hashlib's, zlib's and the oracle's; krk_windows_last_reads says which way the bytes came, and every case accounts for
every byte: window + bounce + page-cache bytes == the files' lengths.

The files lie under the repository's build tree (tests/window_matrix.py direct_dir): a tmpfs opens nothing O_DIRECT,
and FileSource then reads buffered without a word."""
import json
import os
import re
import subprocess
import sys

import pytest

from tests import window_matrix as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 120
_died = []  # a child that ended by a signal or at its timeout: no further child is started


def _child(scenario, refuse=None, **env):
    """One scenario in a fresh process: under the diag library with KRK_DIRECT_REFUSE=refuse, or (refuse None) under
    the production library with nothing refused.  Its JSON line; a child that exits non-zero fails the test."""
    from tests.conftest import diag_lib
    assert not _died, f"the child of {_died[0]} ended by a signal or at its timeout: no further child is started"
    e = {k: v for k, v in os.environ.items() if k not in ("KRK_DIRECT_REFUSE", "KRK_LIB_PATH", "KRK_LIVE_CAP")}
    e.update(KRK_WINDOW_MB="1", KRK_FILE_DIRECT="1", **env)
    if refuse is not None:
        e.update(KRK_LIB_PATH=diag_lib(), KRK_DIRECT_REFUSE=str(refuse))
    with M.direct_tmp() as d:
        if d is None:
            pytest.skip(M.NO_DIRECT)
        try:
            r = subprocess.run([sys.executable, "-m", "tests.window_matrix", "reads", scenario, d], capture_output=True,
                               text=True, cwd=ROOT, env=e, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired as x:
            _died.append(scenario)
            pytest.fail(f"{scenario}: the child did not end within {CHILD_TIMEOUT_S} s; output so far: {x.stdout!r}")
    if r.returncode < 0:
        _died.append(scenario)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    print(json.dumps(out))
    assert out["n_mismatches"] == 0 and out["refused"] == refuse, out
    return out


AIO = {"aio": "1", "sync": "0"}


@pytest.mark.parametrize("P", [M.MiB, 3])
@pytest.mark.parametrize("how", ["aio", "sync"])
def test_edge_lengths_every_read_refused(gpu, how, P):
    """Case 1: the EDGE lengths at piece lengths 1 MiB and 3, every read refused: every digest and piece sum right,
    every byte through the bounce buffer, none straight into a window, the switch on.  A child a piece length: only
    the first direct call of a process reaches the AIO reaper, which must see every file's first chunk refused."""
    out = _child("edge:%d" % P, 1, KRK_FILE_AIO=AIO[how])
    rd = out["reads"]
    assert rd["bounce_bytes"] == out["total"] and rd["window_bytes"] == 0 and rd["bounce_on"], rd
    if how == "aio":
        assert rd["aio_reaped"] == rd["aio_rereads"] == out["tasks"], (rd, out["tasks"])


def test_first_window_deeper_than_the_aio_queue(gpu):
    """Case 2: 300 read tasks in the first window against 256 AIO requests in flight: the refusals arrive while
    requests are in flight and more are to be submitted.  Every refused task is re-read, and from the second window on
    the read threads have the windows: no AIO request is reaped for them."""
    out = _child("files_aio:many", 1, KRK_FILE_AIO="1")
    rd, tasks = out["reads"], out["tasks"]
    assert tasks[0] == M.R_FILES > 256 and len(tasks) >= 3, tasks
    assert rd["aio_rereads"] >= tasks[0], (rd, tasks)
    assert 1 <= rd["aio_reaped"] <= tasks[0], (rd, tasks)
    assert rd["bounce_bytes"] == out["total"] and rd["window_bytes"] == 0 and rd["bounce_on"], rd


@pytest.mark.parametrize("how,n", [("aio", 100), ("sync", 5)])
def test_switch_flips_in_mid_batch(gpu, how, n):
    """Case 3: the N-th read is the first refused: bytes of both kinds, and together all of them.  Where this
    machine's windows refuse the reads themselves (asked of the machine by one os.preadv into a page-locked page,
    M.machine_refuses) the first read is refused whatever N says and no byte can go straight into a window: the
    counters are then case 1's."""
    out = _child("files_%s:many" % how, n, KRK_FILE_AIO=AIO[how])
    rd = out["reads"]
    assert rd["window_bytes"] + rd["bounce_bytes"] + rd["cached_bytes"] == out["total"] and rd["bounce_on"], rd
    if out["machine_refuses"]:
        assert rd["window_bytes"] == 0 and rd["bounce_bytes"] == out["total"], rd
    else:
        assert rd["window_bytes"] > 0 and rd["bounce_bytes"] > 0, rd


def test_requests_larger_than_the_bounce_buffer(gpu):
    """Case 4: requests of 3 MiB + 4 KiB and 2 MiB through the 1 MiB bounce buffer: more preads than tasks."""
    out = _child("files_sync:big", 1, KRK_FILE_AIO="0")
    rd = out["reads"]
    assert out["tasks"] == [2] and rd["bounce_preads"] > 2, (rd, out["tasks"])
    assert rd["bounce_bytes"] == out["total"] == 5 * M.MiB + 5, rd


@pytest.mark.parametrize("how", ["aio", "sync"])
def test_threaded_fill_every_thread_its_own_buffer(gpu, how):
    """Case 5: windows of at least kSplitMinBytes (window_math.hpp), which par_read cuts into spans for the pool's
    threads, each bouncing through a buffer of its own."""
    text = open(os.path.join(ROOT, "kraken_amd", "csrc", "window_math.hpp")).read()
    m = re.search(r"kSplitMinBytes = size_t\((\d+)\) << (\d+);", text)
    split_min = int(m.group(1)) << int(m.group(2))
    case = M.case_d()
    first = sum((ln + 4095) // 4096 * 4096 for _, _, ln in case.replay(4096)[0][0])
    assert first >= split_min == M.SPLIT_MIN, (first, split_min)
    out = _child("files_%s:split" % how, 1, KRK_FILE_AIO=AIO[how])
    assert out["reads"]["bounce_bytes"] == out["total"] == sum(case.lens), out["reads"]


@pytest.mark.parametrize("what", list(M.SHORT) + ["missing"])
@pytest.mark.parametrize("how", ["aio", "sync"])
def test_short_and_missing_files_keep_their_texts(gpu, how, what):
    """Case 6: a file shorter than declared -- by one byte, to a 4 KiB edge, to exactly 1 MiB inside a 3 MiB request --
    is KRK_EIO with `read blob: <path>: unexpected EOF`, the text of the unrefused reads; a missing file keeps
    `open ...: No such file or directory`.  Each shortfall is the first direct call of a child of its own: on the AIO
    leg the request is reaped, refused and re-read by the reaper (one request reaped, one re-read, asserted in the
    child), and that re-read -- for the 3 MiB request, block-rounded and larger than the bounce buffer -- meets the end
    of the file; in one shared process every shortfall after the first would have gone to the read threads."""
    _child("short:" + what, 1, KRK_FILE_AIO=AIO[how])


def test_piece_sums_files_every_read_refused(gpu):
    """Case 7: krk_piece_sums_files on the GPU placement (the FileSource without AIO): sums right, every byte bounced."""
    out = _child("sums", 1)
    rd = out["reads"]
    assert rd["bounce_bytes"] == out["total"] and rd["window_bytes"] == 0 and rd["aio_reaped"] == 0, rd


def test_two_threads_flip_the_switch_between_them(gpu):
    """Case 8: two threads of one process, a 40-file direct batch each at the same time, the third read refused."""
    out = _child("threads", 3)
    assert all(rd["bounce_on"] for rd in out["reads"]), out["reads"]


@pytest.mark.parametrize("how", ["aio", "sync"])
def test_unrefused_control_accounts_for_every_byte(gpu, how):
    """Case 9: the 300 files under the production library with nothing simulated.  Windows that accept the disk's DMA
    leave the switch off: no byte bounced, all of them straight into the windows, one AIO request a task.  Windows
    that refuse it turn the switch on by themselves, and the counters are those of case 1."""
    out = _child("files_%s:many" % how, None, KRK_FILE_AIO=AIO[how])
    rd, total, tasks = out["reads"], out["total"], sum(out["tasks"])
    print("the windows of this machine %s O_DIRECT reads" % ("refuse" if rd["bounce_on"] else "accept"))
    assert rd["bounce_on"] == out["machine_refuses"], out
    if not rd["bounce_on"]:
        assert rd["bounce_bytes"] == 0 and rd["bounce_preads"] == 0 and rd["window_bytes"] == total, rd
        if how == "aio":
            assert rd["aio_reaped"] == tasks, (rd, tasks)
    else:
        assert rd["bounce_bytes"] == total and rd["window_bytes"] == 0, rd
