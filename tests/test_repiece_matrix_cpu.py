"""The re-piece matrix (tests/repiece_matrix.py) where no GPU is: its builders give the counts the
module states, groups A - F pass through krk_repiece_batch and (D apart) blob by blob through
krk_repiece_sums -- the host forms piece_repiece.hip is documented to equal -- and every row of
the refusals table comes back with its code, its text and the outputs' canaries intact."""
import ctypes as C
import zlib

import numpy as np
import pytest

from kraken_amd import _capi
from kraken_amd._capi import lib
from tests import repiece_matrix as M

u32p = M.u32p


@pytest.fixture(scope="module")
def host():
    return M.HostBackend()


def test_group_a_and_b_builders(host):
    for k, b in zip(M.A_K, M.batches_a(host.host)):
        g = 64 // k
        shapes = M.shapes_a(k)
        assert {n for n, _, _ in shapes} == {g - 1, g, g + 1, 2 * g, 2 * g + 1}
        assert {m for _, m, _ in shapes} == {1, max(k - 1, 1), k} and {t for _, _, t in shapes} == {1, 15, 16}
        assert b.n == len(shapes) and (b.k == k).all() and (b.po == M.PO).all()
        assert b.n_new.tolist() == [max(n, 0) for n, _, _ in shapes]
        live = b.n_new > 0
        last_olds = b.n_old - (b.n_new - 1) * k
        assert last_olds[live].tolist() == [m for n, m, _ in shapes if n > 0]
        assert ((b.L - 1) % M.PO + 1)[live].tolist() == [t for n, _, t in shapes if n > 0]
        assert b.units == int(((b.n_new + g - 1) // g).sum())
    for k, passes, b in zip(M.B_K, M.B_PASSES, M.batches_b(host.host)):
        assert b.n_old.tolist() == [k - 1, k - 1, k, k, k + 1, k + 1] and b.n_new.tolist() == [1, 1, 1, 1, 2, 2]
        assert b.units == int(b.n_new.sum()) and -(-k // 64) == passes


def test_group_c_d_e_f_builders(host):
    mixed, empty, short = M.batches_c(host.host)
    assert mixed.n_new.tolist() == [0, 0, 0, 3, 0, 0, 65, 0, 2, 1, 0, 1, 1, 0, 0] and mixed.units == 1 + 2 + 2 + 1 + 1 + 1
    assert empty.units == 0 and empty.want.size == M.SPARE and (empty.want == M.CANARY).all()
    assert short.n_old.tolist() == [1, 1, 1, 1] and short.n_new.tolist() == [1, 1, 1, 1]
    d = M.batch_d(host.host)
    e = M.empty_d()
    assert d.n == 263_000 and int(e.sum()) == 276 and (d.n_new[e] == 0).all() and d.units == d.n - 276 > M.STRIDE_UNITS
    assert set(d.n_new[~e].tolist()) == {1, 2, 3} and set(d.n_old.tolist()) == {0, 1, 2, 3, 4, 5, 6}
    # the waves' second pass starts inside a run of empty blobs
    w = M.STRIDE_UNITS
    assert e[w - 1:w + 3].all() and not e[w - 2] and not e[w + 3]
    # a template blob's sums are zlib's
    i = int(np.flatnonzero(d.n_new == 3)[0])
    assert d.want[d.out_off[i]:d.out_off[i] + 3].tolist() != [M.CANARY] * 3
    eb = M.batch_e(host.host)
    assert set(eb.po.tolist()) == set(M.E_PO) and (eb.k > 64).any() and (eb.k <= 64).any() and (eb.L == 0).sum() == 5
    live = eb.n_old > 0
    assert int(eb.sums_off[live].min()) == 1000 and int(eb.out_off[live].min()) == 1000
    assert (np.diff(eb.sums_off[live]) < 0).any() and (np.diff(eb.out_off[live]) < 0).any()
    assert eb.want.size - M.SPARE - 1000 > int(eb.n_new.sum())  # gaps
    f = M.batch_f()
    assert (f.po == 1 << 33).all() and set(f.k.tolist()) == set(M.F_K) and f.L.min() > (1 << 39)
    assert (f.L % f.po != 0).all() and f.n_old.max() == 257
    assert sorted(f.n_new[f.k == 129].tolist()) == [1, 1, 2, 2] and sorted(f.n_new[f.k == 3].tolist()) == [43, 43, 44, 86]


@pytest.mark.parametrize("group,count", [("A", 15 * (1 + 2 + 10 * 3)), ("B", 30), ("C", 24), ("D", 263_000),
                                         ("E", len(M.blobs_e())), ("F", 8)])
def test_groups_pass_on_the_host_batch_form(host, group, count):
    n, bad = M.run_group_counted(group, host)
    assert n > 0 and (count is None or n == count)
    assert bad == []


@pytest.mark.parametrize("group", ["A", "B", "C", "E", "F"])
def test_groups_pass_blob_by_blob_through_repiece_sums(group):
    n, bad = M.run_group_counted(group, M.SumsBackend())
    assert n > 0
    assert bad == []


def test_a_ratio_that_covers_the_blob_gives_its_crc32(host):
    data = host.host[1234:1234 + 100_003]
    for po in (1, 3, 64, 4096):
        old = np.array([zlib.crc32(data[a:a + po]) for a in range(0, data.size, po)], dtype=np.uint32)
        for npl in (po * -(-data.size // po), po * (1 << 20)):
            out = np.full(2, M.CANARY, dtype=np.uint32)
            _capi.check(lib.krk_repiece_sums(old.ctypes.data_as(u32p), old.size, data.size, po, npl, out.ctypes.data_as(u32p), 1))
            assert out.tolist() == [zlib.crc32(data), M.CANARY], (po, npl)


def test_reporting_names_the_blob_and_the_stray_word(host):
    b = M.batch_e(host.host)
    got = b.want.copy()
    i = int(np.flatnonzero(b.n_new == 3)[0])
    got[b.out_off[i] + 2] ^= 1
    got[-1] = 7
    out = M.compare("X", b, got)
    assert len(out) == 2 and out[0][0].startswith(f"X blob {i} (") and out[0][0].endswith("new piece 2")
    assert out[0][1] ^ out[0][2] == 1 and out[1] == (f"X: output word {got.size - 1}, which belongs to no blob, was written", 7, M.CANARY)


def test_refusals_write_nothing():
    old = np.arange(64, dtype=np.uint32)
    for what, row, code, text in M.refusals():
        out = np.full(64, M.CANARY, dtype=np.uint32)
        blobs = M.refusal_batch(row)
        rc = lib.krk_repiece_batch(blobs.ctypes.data_as(M.blobp), 3, old.ctypes.data_as(u32p), out.ctypes.data_as(u32p))
        assert rc == code, what
        assert text is None or lib.krk_last_error().decode() == text, what
        assert (out == M.CANARY).all(), what
        length, pl, npl = row
        rc = lib.krk_repiece_sums(old.ctypes.data_as(u32p), 7, length, pl, npl, out.ctypes.data_as(u32p), 64)
        assert rc == code, what
        assert text is None or lib.krk_last_error().decode() == text, what
        assert (out == M.CANARY).all(), what
    # krk_repiece_sums' own rows: 100 bytes in pieces of 16 are 7 sums, 4 at 32
    out = np.full(64, M.CANARY, dtype=np.uint32)
    for n_sums in (6, 8, 0):
        assert lib.krk_repiece_sums(old.ctypes.data_as(u32p), n_sums, 100, 16, 32, out.ctypes.data_as(u32p), 64) == _capi.KRK_EINVAL
        assert lib.krk_last_error().decode() == f"{n_sums} piece sums for 7 pieces"
    for n_out in (3, 0):
        assert lib.krk_repiece_sums(old.ctypes.data_as(u32p), 7, 100, 16, 32, out.ctypes.data_as(u32p), n_out) == _capi.KRK_ERANGE
    assert (out == M.CANARY).all()
    # the accepted neighbours: an exact fit, an empty blob with NULL arrays, an empty batch
    assert lib.krk_repiece_sums(old.ctypes.data_as(u32p), 7, 100, 16, 32, out.ctypes.data_as(u32p), 4) == _capi.KRK_OK
    assert (out[:4] != M.CANARY).all() and (out[4:] == M.CANARY).all()
    assert lib.krk_repiece_sums(None, 0, 0, 16, 32, None, 0) == _capi.KRK_OK
    assert lib.krk_repiece_batch(None, 0, None, None) == _capi.KRK_OK


def test_repiece_batch_dev_without_a_device():
    """An empty batch is KRK_OK anywhere and a refusal needs no device; a real batch needs a gfx950
    device (KRK_ENODEV here when there is none -- with one, tests/test_gpu_repiece_matrix.py)."""
    from kraken_amd import device as D
    assert lib.krk_repiece_batch_dev(None, 0, None, None, None) == _capi.KRK_OK
    bad = M.refusal_batch((100, 16, 40))
    assert lib.krk_repiece_batch_dev(bad.ctypes.data_as(M.blobp), 3, None, None, None) == _capi.KRK_EINVAL
    if D.device_count() == 0:
        good = M.refusal_batch((100, 16, 32))
        old = np.zeros(64, dtype=np.uint32)
        rc = lib.krk_repiece_batch_dev(good.ctypes.data_as(M.blobp), 3, old.ctypes.data, old.ctypes.data, None)
        assert rc == _capi.KRK_ENODEV
