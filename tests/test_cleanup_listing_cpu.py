"""Cleanup plans from a raw cache listing where no GPU is (placement "host"): castore.Listing's
force_cleanup_plan against maybeDelete a name at a time and against castore.force_cleanup_plan,
cleanup_scan_plan against readyForDeletion a file at a time, the _last_access_time codec against
its golden bytes, and DirCAS.Listing() over a temporary cache (the checks live in
tests/cleanup_listing_cases.py; tests/test_gpu_cleanup_listing.py runs them at placement "gpu")."""
import pytest

from kraken_amd import _capi, castore, device as D
from tests import cleanup_listing_cases as L


def test_force_cleanup_plan_equals_maybe_delete_name_by_name(orc):
    L.check_force_cleanup_plan(orc, "host")


def test_cleanup_scan_plan_equals_ready_for_deletion_file_by_file():
    L.check_cleanup_scan_plan()


def test_last_access_time_golden_bytes_round_trip_and_errors():
    L.check_last_access_time()


def test_dircas_listing_with_and_without_sidecars(tmp_path, orc):
    L.check_dircas_listing(tmp_path, orc, "host")


def test_gpu_placement_without_a_device_is_an_error_not_a_fallback():
    ls = castore.Listing(["ab"], mtime_ns=[0])
    with pytest.raises(ValueError):
        ls.parse(placement="auto")
    if D.device_count() == 0:
        with pytest.raises(_capi.KrakenError) as e:
            ls.parse(placement="gpu")
        assert e.value.code == _capi.KRK_ENODEV


def test_dev_entry_points_refuse_then_need_a_device():
    """Every _dev entry point answers its refusals with KRK_EINVAL, device or not; a real call
    without a gfx950 device is KRK_ENODEV and touches nothing: there is no fall-back to the host."""
    import ctypes as C

    import numpy as np

    from kraken_amd._capi import lib
    ls = castore.Listing(["ab" * 32, "zz"], mtime_ns=[0, 0])
    mask = np.zeros(1024, dtype=np.uint64).ctypes.data_as(C.POINTER(C.c_uint64))
    out = np.full(64, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    o, t, off, mt = out.ctypes.data, ls.text.ctypes.data, ls.off.ctypes.data, ls.mtime_ns.ctypes.data
    E, N = _capi.KRK_EINVAL, _capi.KRK_ENODEV
    assert lib.krk_digest_parse_hex_dev(None, off, 2, o, None, None, None) == E
    assert lib.krk_digest_parse_hex_dev(t, None, 2, o, None, None, None) == E
    assert lib.krk_digest_parse_hex_dev(t, off, 2, None, None, None, None) == E
    assert lib.krk_digest_format_hex_dev(None, 2, o, None) == E
    assert lib.krk_digest_format_hex_dev(o, 2, None, None) == E
    assert lib.krk_cleanup_plan_dev(None, off, 2, mt, 0, 0, mask, 1, o, None, None, 0, o + 64, None) == E
    assert lib.krk_cleanup_plan_dev(t, None, 2, mt, 0, 0, mask, 1, o, None, None, 0, o + 64, None) == E
    assert lib.krk_cleanup_plan_dev(t, off, 2, mt, 0, 0, None, 1, o, None, None, 0, o + 64, None) == E
    assert lib.krk_cleanup_plan_dev(t, off, 2, mt, 0, 0, mask, 1, None, None, None, 0, o + 64, None) == E
    assert lib.krk_cleanup_plan_dev(t, off, 2, mt, 0, 0, mask, 1, o, None, None, 0, None, None) == E
    assert lib.krk_cleanup_plan_dev(t, off, 2, mt, 0, 0, mask, 1, o, None, None, 2, o + 64, None) == E  # NULL idx, cap 2
    if D.device_count() == 0:
        assert lib.krk_digest_parse_hex_dev(t, off, 2, o, None, None, None) == N
        assert lib.krk_digest_format_hex_dev(o, 2, o + 128, None) == N
        assert lib.krk_cleanup_plan_dev(t, off, 2, mt, 0, 0, mask, 1, o, None, None, 0, o + 64, None) == N
    assert (out == 0xFFFFFFFFFFFFFFFF).all()
