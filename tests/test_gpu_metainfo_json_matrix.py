"""GPU parity: the _torrentmeta JSON kernels (metainfo_json.hip) at their scan-pass, grid-stride,
store-step and unit edges through krk_metainfo_serialize_batch_dev and
krk_metainfo_parse_sums_batch_dev -- every byte of out, every out_len, every status word, every
sums word and the canaries between and behind the ranges against plain Python (json.dumps, and the
span grammar as a regular expression).  The cases and the comparison live in
tests/metainfo_json_matrix.py; tests/test_metainfo_json_matrix_cpu.py proves the matrix's coverage
conditions and runs the same cases through the host forms.  One test a group; the buffers of a
test are allocated once and freed at its end."""
import pytest

from tests import metainfo_json_matrix as M

pytestmark = pytest.mark.gpu


def run(calls, **kw):
    with M.DeviceBackend() as dev:
        made, bad = M.run_cases(dev, calls, **kw)
    assert made == len(calls) > 0 and bad == [], f"{len(bad)} mismatches in {made} calls, first {bad[:5]}"


def test_s1_serialize_scan_passes(gpu):
    """PASS-1, PASS, PASS+1, 2 PASS, 2 PASS + 1 and 3 PASS + 517 units: the scan's carry, its
    barrier between passes and the ragged last pass."""
    assert [c.n_units for c in M.s1_cases()] == list(M.TOTALS)
    run(M.s1_cases())


def test_s2_serialize_last_step_shapes(gpu):
    """A final step of 1..12 bytes at every phase of a dword, in step 0 of unit 0, a later step of
    unit 0 and step 0 of a later unit (the backend asserts out is 4-byte aligned)."""
    assert M.s2_coverage(M.s2_case()) == M.S2_SHAPES
    run([M.s2_case()])


def test_s3_serialize_owner_search(gpu):
    """Runs of null / [] blobs at the head, in the middle and at the tail; calls without a unit;
    1 .. 257 blobs with units."""
    run(M.s3_cases())


def test_s4_serialize_grid_stride(gpu):
    """G + 3 one-sum blobs: unit u and unit u + G share a workgroup."""
    assert M.s4_case().n_units > M.G
    run([M.s4_case()])


def test_p1_parse_scan_passes(gpu):
    assert [c.n_units for c in M.p1_cases()] == list(M.TOTALS)
    run(M.p1_cases())


def test_p2_parse_break_positions(gpu):
    """One byte broken in unit 0, 63, 64, 65, 127, 128 or the last of a 131-unit span: bit 0, and
    the valid neighbours untouched."""
    run([M.p2_case()])


def test_p3_parse_malformed_numbers_across_a_unit_edge(gpu):
    run([M.p3_case()])


def test_p4_parse_count_guard_at_scale(gpu):
    """status == 2 exactly, and every word outside [sums_off, sums_off + expect_n) a canary."""
    run([M.p4_case()])


def test_p5_parse_owner_search_stride_and_page_locked_outputs(gpu):
    run(M.p5_cases() + [M.p5_stride_case()])
    run([M.p5_pinned_case()], pinned=True)
