"""The sentinel-collision run of tests/test_gpu_sha_share_matrix.py, in a process of its own so that
a stalled wait ends at the parent's time limit:  python -m tests.sha_share_child collision|control

The block-edge batch whose blob 1 is handed over at 64 bytes gets the fixture's block as that
chain's first block.  With "collision" the midstate the GPU writes into the note holds the note's
fill in one word, so the host cannot tell it from an unwritten one and takes the branch that waits
for the launch to end; "control" is the same run with a block whose midstate holds no such word.
Digests and piece sums are compared with hashlib and zlib; prints "ok <name>"."""
import sys

from kraken_amd import device as D
from tests import sha256_ref as R
from tests import sha_share_matrix as M


def main(which):
    fx, fill = M.sentinel_fixture()
    block, word, mid, _ = fx[which]
    case = M.BY_NAME[M.SENTINEL_CASE]
    assert (1, 64) in [tuple(p) for p in case.tails]
    assert R.compress(R.IV, block) == mid and (fill in mid) == (which == "collision")
    D.set_device(0)
    b = M.build(case, first_block={1: block})
    assert bytes(b.host[b.offs[1]:b.offs[1] + 64]) == block
    try:
        with M.settings(case):
            for fn, P in ((M.sha256_call, None), (M.metainfo_digest_call, case.piece_lengths[0])):
                out = M.Outputs(b, P)
                fn(b, out)
                out.read_back(None)
                D.check(D.lib.krk_stream_sync(None))
                assert D.sha_last_tail() == M.last_tail_of(case), D.sha_last_tail()
                out.check((which, fn.__name__))
                out.free()
    finally:
        b.buf.free()
    print("ok", which, flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
