"""The window matrix (tests/window_matrix.py) on the device: the host-resident window passes -- run_windows of
window_pass.cpp under WindowSched (the digest calls of windows.cpp) and PackSched (the CRC-only calls of
crc_host.cpp), the slot ring, par_copy and par_read of staging.hpp -- at their chunk, slot and transport edges.  Every output array is compared whole (canaries on both sides, prefilled with 0xFF) against
hashlib.sha256 / zlib.crc32 images, a mismatch names the blob, the piece and the windows, slots and chunks its bytes
went through, and krk_windows_last_* must equal the Python replay of the schedule after every call.

Group C: A, A2 and B through every way up; D: 9 MiB windows that par_copy / par_read split; E: layouts, n = 1, empty
blobs only and a host-offload subset; F: the CRC-only packers.  tests/test_window_matrix_cpu.py proves the cases."""
import json
import os
import subprocess
import sys

import pytest

from tests import window_matrix as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _report(bad):
    assert bad == [], "\n".join(bad[:12])


C_CASES = {
    "A": M.case_a,                          # by the leg's alignment
    "A2-Pc5": lambda align: M.case_a2(),
    "A2-P4096": lambda align: M.case_a2(4096),
    "A2x-Pc5": lambda align: M.case_a2x(),
    "A2x-P4096": lambda align: M.case_a2x(4096),
    "B": lambda align: M.case_b(),
}


@pytest.mark.parametrize("leg", M.LEGS)
@pytest.mark.parametrize("name", list(C_CASES))
def test_group_c_every_way_up(gpu, tmp_path, monkeypatch, name, leg):
    case = C_CASES[name](M.leg_align(leg))
    files_b = name == "B" and leg.startswith("files")
    # B's files: 17,084 of them (5 MB, a second or two to write; the leg runs however long the disk takes, a skip
    # by the clock made it come and go with the load of the machine); a process's descriptor budget may cap the
    # live files below KRK_LIVE_CAP
    _report(M.run_leg(case, leg, tmp_path, monkeypatch.setenv, lower_cap_ok=files_b))


@pytest.mark.parametrize("ring", [2, 4])
def test_group_c_ring_depths(gpu, ring):
    """The ring depth is fixed per process (KRK_STAGING_WINDOWS): group A, staged and from buffered files, in one fresh
    child process a depth, so a window's slot is reused every second / fourth window."""
    env = dict(os.environ, KRK_STAGING_WINDOWS=str(ring))
    r = subprocess.run([sys.executable, "-m", "tests.window_matrix", "staged", "files"], capture_output=True, text=True,
                       cwd=ROOT, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert [(x["leg"], x["ring"], x["n_mismatches"]) for x in lines] == [("staged", ring, 0), ("files", ring, 0)], lines


@pytest.mark.parametrize("leg", ["staged", "arena0", "files", "files_aio", "files_sync"])
@pytest.mark.parametrize("P", [M.MiB, 65_537])
def test_group_d_windows_wide_enough_to_split(gpu, tmp_path, monkeypatch, P, leg):
    _report(M.run_leg(M.case_d(P), leg, tmp_path, monkeypatch.setenv))


@pytest.mark.parametrize("base", ["A2", "D"])
def test_group_e_permuted_gapped_offsets(gpu, tmp_path, monkeypatch, base):
    """Sums offsets in reverse order, seven words apart, from word 1,000: words below the span and after it keep
    their canary; a gap word inside the span comes back zero from krk_metainfo_digest_host / _files and
    krk_piece_sums_files (GPU placement) and is left alone by krk_piece_sums_host (include/kraken_hip.h)."""
    case = M.case_e_layout(M.case_a2(4096) if base == "A2" else M.case_d(65_537))
    _report(M.run_entries(case, tmp_path, monkeypatch.setenv))


def test_group_e_one_blob(gpu, tmp_path, monkeypatch):
    _report(M.run_entries(M.case_e_single(), tmp_path, monkeypatch.setenv))


def test_group_e_empty_blobs_only(gpu, tmp_path, monkeypatch):
    """No piece exists: the sums array keeps every canary; every digest is sha256 of nothing."""
    _report(M.run_entries(M.case_e_empty(), tmp_path, monkeypatch.setenv, page_locked_if_empty=True))


def test_group_e_host_offload_subset(gpu, tmp_path, monkeypatch):
    _report(M.run_mixed(M.case_e_mixed(), tmp_path, monkeypatch.setenv))


@pytest.mark.parametrize("share", ["1", "0.5", "mid"])
def test_group_f_piece_sums_host(gpu, monkeypatch, share):
    """krk_piece_sums_host on a krk_host_alloc arena: the whole batch, half of it, and a share that ends inside a blob
    at a piece edge on the GPU's packer, the rest on host threads; krk_crc_host_split reports the share to whole
    pieces."""
    case = M.case_f(16)
    _report(M.run_sums_host(case, M.f_mid_fraction(case) if share == "mid" else share, True, monkeypatch.setenv))


def test_group_f_piece_sums_host_pageable(gpu, monkeypatch):
    """The same packer over pageable memory (the forced share takes it to the GPU): staged through par_copy."""
    _report(M.run_sums_host(M.case_f(16), "1", False, monkeypatch.setenv, misalign=15))


@pytest.mark.parametrize("direct", [False, True])
def test_group_f_piece_sums_files(gpu, tmp_path, monkeypatch, direct):
    _report(M.run_sums_files(M.case_f(4096), tmp_path, direct, monkeypatch.setenv))
