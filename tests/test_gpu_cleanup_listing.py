"""GPU parity of the Python surface (placement "gpu"): castore.Listing's parse and
force_cleanup_plan through krk_digest_parse_hex_dev and krk_cleanup_plan_dev -- from pageable
columns uploaded by the call and from page-locked ones the device reads in place -- against
maybeDelete a name at a time, castore.force_cleanup_plan and the host placement; and
DirCAS.Listing() over a temporary cache (the checks live in tests/cleanup_listing_cases.py)."""
import numpy as np
import pytest

from kraken_amd import castore
from tests import cleanup_listing_cases as L

pytestmark = pytest.mark.gpu


def test_force_cleanup_plan_equals_maybe_delete_name_by_name(gpu, orc):
    L.check_force_cleanup_plan(orc, "gpu")


def test_page_locked_listing_equals_the_host_placement(gpu, orc):
    labels = L.labels_of(5)
    ring = L.ring_of(orc, labels, 3)
    names, mtimes, now, ttl, _ = L.listing_300(ring, labels[2])
    s = 1_000_000_000
    ls = castore.Listing(names, mtime_ns=mtimes * s)
    want = ls.force_cleanup_plan(now * s, ttl * s, ring, labels[2], placement="host")
    wd, wv, we = ls.parse(placement="host")
    ls.pin()
    for _ in range(2):  # the second call reuses the listing's buffers
        idx, errors = ls.force_cleanup_plan(now * s, ttl * s, ring, labels[2], placement="gpu")
        assert idx.tolist() == want[0].tolist() and errors == want[1]
        d, v, e = ls.parse(placement="gpu")
        assert np.array_equal(d, wd) and np.array_equal(v, wv) and e == we


def test_scan_plan_last_access_time_and_dircas_listing(gpu, tmp_path, orc):
    L.check_cleanup_scan_plan()
    L.check_last_access_time()
    L.check_dircas_listing(tmp_path, orc, "gpu")
