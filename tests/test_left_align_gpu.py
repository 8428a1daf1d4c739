"""compare_vcf --left_align on the device (csrc/compare.hip: la_case_kernel, shift_kernel and the scans between them) against its host twin,
integer for integer: records, arena bytes, the pass's statistics, outcomes and the counter block, on the shapes at which the kernels can go
wrong (tests/leftalign_cases.py), the crafted cases, generated pairs, and through the command line."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import leftalign_cases as lc  # noqa: E402
from clair_amd import _capi, compare_vcf as cv  # noqa: E402
from test_left_align import assert_same, case_files, cells, cli_outputs, generated, grid, plain, run_case, shaped_cases  # noqa: E402


def same_on_both(case):
    device, host = run_case(case, "device"), run_case(case, "host")
    assert device["backend"] == "device"
    assert_same(plain(device), plain(host), case["name"])
    return device


@pytest.mark.parametrize("case", lc.crafted(), ids=lambda c: c["name"])
def test_device_equals_the_host_twin_on_crafted_cases(case):
    same_on_both(case)


def test_device_equals_the_host_twin_on_the_shift_grid():
    """Shift distances 0 .. 200 around the 64 steps of a ballot, event lengths 1 .. 130 around the 64 lanes that write them, insertions and
    deletions, both forms of the closed rule."""
    case, _, n_moved = grid()
    device = same_on_both(case)
    n = len(lc.LENGTHS) * len(lc.SHIFTS) * 2
    assert cells(device["counts"]) == {("calls", "INS"): {"TP": n}, ("calls", "DEL"): {"TP": n}, ("truth", "INS"): {"TP": n}, ("truth", "DEL"): {"TP": n}}
    assert device["left_align"]["calls"]["shifted"] == n_moved


@pytest.mark.parametrize("case", shaped_cases(), ids=lambda c: c["name"])
def test_device_equals_the_host_twin_on_shapes(case):
    """An event of 5 000 bases; runs that end at a contig's start and one base short of it, with the same repeat in the contig before; record
    counts around the scan's workgroup of COMPARE_SCAN_BLOCK, so that the arena's prefix sum and the candidate list cross workgroups; a side
    without an indel and one of indels only."""
    assert _capi.COMPARE_SCAN_BLOCK == 2048
    device = same_on_both(case)
    if case["name"] == "contig_boundaries":
        assert (device["left_align"]["calls"]["at_contig_start"], device["left_align"]["calls"]["shifted"]) == (6, 4)


@pytest.mark.parametrize("seed,n,break_order", [(300, 1200, True), (300, 1200, False)])
def test_device_equals_the_host_twin_on_generated_pairs(seed, n, break_order):
    case, full = generated(seed, n, break_order)
    device = same_on_both(case)
    assert [device["stats"][s]["permuted"] for s in cv.SIDES] == ([1, 1] if break_order else [0, 0])


def test_command_line_prints_the_same_on_both_backends(tmp_path):
    case, _ = generated(300, 1200, True)
    paths = case_files(tmp_path, case)
    outputs = dict((backend, cli_outputs(tmp_path, paths, backend, backend)) for backend in ("device", "host", "auto"))
    assert outputs["device"] == outputs["host"] == outputs["auto"]
    assert outputs["device"][0].count("\n") == 7 and '"left_align"' in outputs["device"][1] and len(outputs["device"][2]) > 1000
