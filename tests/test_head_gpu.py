"""GPU tier of the head tier (tests/head_cases.py): the same cases as tests/test_head_emu.py on the real libcfun_hip.so --
the classifier GEMMs past one K chunk and past 64 chunks, RoIAlign / un-molding / mask targets / resize past their grid caps,
NMS at its sort, LDS-switch and prefetch edges (here with v_readlane in the LDS-resident scan).

Every comparison under the rule appends a row (e32, the kernel's error, the bound, the ratio) to membound_cases.REPORT, which
head_cases shares.  A module-scoped fixture owns that list for this file: it empties it before the first selected test and
prints the rows of whatever was selected after the last one; ``CFUN_PARITY_TABLE=<file>`` appends them to a file
(profiles/head_parity.txt is a run of the whole file)."""
import os

import pytest

import head_cases as hc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def parity_table():
    hc.REPORT.clear()
    yield
    lines = hc.report_lines()
    print("\n".join(lines))
    path = os.environ.get("CFUN_PARITY_TABLE")
    if path and lines:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")
    hc.REPORT.clear()


def test_launch_constants(gpu):
    hc.check_launch_constants(gpu)


# ---- A. classifier GEMMs
@pytest.mark.parametrize("k", hc.FC_K_EDGES)
def test_fc_k_edges(gpu, k):
    hc.check_fc_abi(gpu, 5, k, 12)


@pytest.mark.parametrize("k", hc.FC_CHUNK_EDGES)
def test_fc_finish_row_groups(gpu, k):
    hc.check_fc_abi(gpu, 3, k, 8)


@pytest.mark.parametrize("r", hc.FC_R_EDGES)
def test_fc_r_edges(gpu, r):
    hc.check_fc_abi(gpu, r, 516, 20)


@pytest.mark.parametrize("o", hc.FC_O_EDGES)
def test_fc_o_edges(gpu, o):
    hc.check_fc_abi(gpu, 17, 516, o)


@pytest.mark.parametrize("epi", hc.FC_EPILOGUES)
def test_fc_epilogues(gpu, epi):
    hc.check_fc_abi(gpu, 17, 516, 19, epi)
    hc.check_fc_ops(gpu, 17, 516, 19, epi)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["max_rows", "max_rows_plus_1", "r64_o1024"])
def test_fc_dw_row_chunks(gpu, which):
    hc.check_fc_ops(gpu, *hc.fc_row_chunk_cases(gpu)[which])


def test_fc_zero_rows(gpu):
    hc.check_fc_zero_rows(gpu)


def test_fc_refusals(gpu):
    hc.check_fc_refusals(gpu)


# ---- B. RoIAlign
def test_roi_fwd_sweeps(gpu):
    hc.check_roi_fwd_sweeps(gpu)


def test_roi_bwd_sweeps(gpu):
    hc.check_roi_bwd_sweeps(gpu)


@pytest.mark.parametrize("pools", [(1, 2, 7), (2, 7, 12), (7, 12, 1), (12, 1, 2), (4, 4, 4)], ids=lambda p: "pool%d_%d_%d" % p)
def test_roi_resampling_edges(gpu, pools):
    hc.check_roi_resampling_edges(gpu, *pools)


def test_roi_box_coordinates(gpu):
    hc.check_roi_box_coordinates(gpu)


@pytest.mark.parametrize("r", [64, 65])
def test_roi_counts(gpu, r):
    hc.check_roi_counts(gpu, r)


def test_roi_zero_rois(gpu):
    hc.check_roi_zero_rois(gpu)


def test_roi_overlap(gpu):
    hc.check_roi_overlap(gpu)


def test_roi_slabs(gpu):
    hc.check_roi_slabs(gpu)


# ---- C. NMS
@pytest.mark.parametrize("n", hc.NMS_SIZES)
def test_nms_sizes(gpu, n):
    hc.check_nms_size(gpu, n)


def test_nms_row_scan_child(gpu, tmp_path):
    hc.check_nms_row_scan_child(gpu, tmp_path)


def test_nms_max_num(gpu):
    hc.check_nms_max_num(gpu)


def test_nms_empty_and_limits(gpu):
    hc.check_nms_empty_and_limits(gpu)


def test_nms_thresholds(gpu):
    hc.check_nms_thresholds(gpu)


def test_nms_chain(gpu):
    hc.check_nms_chain(gpu)


@pytest.mark.parametrize("n", [65, 1025])
def test_nms_ties(gpu, n):
    hc.check_nms_ties(gpu, n)


# ---- D. targets and inference tail
@pytest.mark.parametrize("c", hc.UNMOLD_C)
def test_unmold_argmax(gpu, c):
    hc.check_unmold_argmax(gpu, c)


def test_unmold_argmax_constant(gpu):
    hc.check_unmold_argmax_constant(gpu)


def test_unmold_refusals(gpu):
    hc.check_unmold_refusals(gpu)


@pytest.mark.parametrize("c", [2, 3, 8])
def test_unmold_overlap(gpu, c):
    hc.check_unmold_overlap(gpu, c)


def test_unmold_overlap_counts(gpu):
    hc.check_unmold_overlap_counts(gpu)


def test_unmold_sweeps(gpu):
    hc.check_unmold_sweeps(gpu)


def test_mask_target_sweeps(gpu):
    hc.check_mask_target_sweeps(gpu)


def test_mask_target_coordinates(gpu):
    hc.check_mask_target_coordinates(gpu)


@pytest.mark.parametrize("name", sorted(hc.RESIZE_CASES))
def test_resize(gpu, name):
    hc.check_resize(gpu, name)


def test_resize_sweeps(gpu):
    hc.check_resize_sweeps(gpu)
