"""The InfoHash kernel (info_hash.hip) past one job a workgroup: the launch has at most 2^20
workgroups, so a batch of 2^20 + 65 jobs makes 65 workgroups run a second job over the ring,
pos, done and h their first job left behind.  The cases and their expectation, shared by
tests/test_gpu_info_hash_stride.py (one krk_info_hash_batch_dev call) and
tests/test_info_hash_stride_cpu.py (the distinct shapes through krk_info_hash_math_host).  A
helper module, not a test file.

Every job reads the SAME three sums at the same offset and has no name, so all sort keys of
info_hash_dev.cpp's stable sort are equal and job j is blob j.  Blob i has Length i % 251 and
PieceLength 1 + i % 7: 1,757 distinct digests, from hashlib.sha1 over a bencode written here,
expanded to the batch by numpy indexing.  251 and 7 are coprime to 2^20, so blob i and blob
i + 2^20 (one workgroup's two jobs) differ in both fields, and so do neighbouring rows of the
output: a job landing in another job's row, or a second job starting from the first job's state,
cannot give the expected array."""
import hashlib

import numpy as np

MAX_GRID = 1 << 20  # restated from launch_info_hash: beyond it the workgroups take a second job
N_JOBS = MAX_GRID + 65
SUMS = (0, 4294967295, 1000000000)
N_LENGTHS, N_PIECE_LENGTHS = 251, 7


def bencode(piece_length, sums, name, length):
    """jackpal/bencode-go's encoding of core.info: a dict, keys sorted."""
    return (b"d6:Lengthi%de4:Name%d:%s11:PieceLengthi%de9:PieceSumsl%see"
            % (length, len(name), name, piece_length, b"".join(b"i%de" % s for s in sums)))


def fields(n=N_JOBS):
    """(lengths, piece_lengths) of the batch's blobs."""
    i = np.arange(n, dtype=np.int64)
    return i % N_LENGTHS, 1 + i % N_PIECE_LENGTHS


def table():
    """The (251, 7, 20) digests: [Length, PieceLength - 1]."""
    t = np.zeros((N_LENGTHS, N_PIECE_LENGTHS, 20), dtype=np.uint8)
    for L in range(N_LENGTHS):
        for p in range(N_PIECE_LENGTHS):
            t[L, p] = np.frombuffer(hashlib.sha1(bencode(p + 1, SUMS, b"", L)).digest(), dtype=np.uint8)
    return t


def expected(n=N_JOBS):
    """The (n, 20) digests of the batch."""
    assert n > MAX_GRID, "the batch no longer gives a workgroup a second job"
    ln, pl = fields(n)
    return table()[ln, pl - 1]
