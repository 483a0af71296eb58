"""CPU tier of the head tier (tests/head_cases.py): the classifier GEMMs of fc.hip, RoIAlign / NMS / mask targets / the
un-molding kernels of roi_nms.hip and resize.hip on the HIP emulator, against float64 under the product-shape tier's rule
and bit for bit where the kernels promise that.

The GPU tier (tests/test_head_gpu.py) runs the same cases on the real library.  Cases that live in the GPU file only,
because they need more than about a minute on the emulator: none -- the largest ones here (the two-sweeps-and-a-ragged-third
geometry cases: 4.2 M map-gradient elements, 4.26 M voxels, 8.45 M resize outputs) take seconds to tens of seconds.  The
emulator reads lane words with __shfl where the device uses v_readlane in k_nms_scan_lds; what the cases say about that one
intrinsic is said by the GPU tier alone."""
import pytest

import head_cases as hc


def test_launch_constants(emu):
    hc.check_launch_constants(emu)


# ---- A. classifier GEMMs
@pytest.mark.parametrize("k", hc.FC_K_EDGES)
def test_fc_k_edges(emu, k):
    hc.check_fc_abi(emu, 5, k, 12)


@pytest.mark.parametrize("k", hc.FC_CHUNK_EDGES)
def test_fc_finish_row_groups(emu, k):
    hc.check_fc_abi(emu, 3, k, 8)


@pytest.mark.parametrize("r", hc.FC_R_EDGES)
def test_fc_r_edges(emu, r):
    hc.check_fc_abi(emu, r, 516, 20)


@pytest.mark.parametrize("o", hc.FC_O_EDGES)
def test_fc_o_edges(emu, o):
    hc.check_fc_abi(emu, 17, 516, o)


@pytest.mark.parametrize("epi", hc.FC_EPILOGUES)
def test_fc_epilogues(emu, epi):
    hc.check_fc_abi(emu, 17, 516, 19, epi)
    hc.check_fc_ops(emu, 17, 516, 19, epi)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["max_rows", "max_rows_plus_1", "r64_o1024"])
def test_fc_dw_row_chunks(emu, which):
    hc.check_fc_ops(emu, *hc.fc_row_chunk_cases(emu)[which])


def test_fc_zero_rows(emu):
    hc.check_fc_zero_rows(emu)


def test_fc_refusals(emu):
    hc.check_fc_refusals(emu)


# ---- B. RoIAlign
def test_roi_fwd_sweeps(emu):
    hc.check_roi_fwd_sweeps(emu)


def test_roi_bwd_sweeps(emu):
    hc.check_roi_bwd_sweeps(emu)


@pytest.mark.parametrize("pools", [(1, 2, 7), (2, 7, 12), (7, 12, 1), (12, 1, 2), (4, 4, 4)], ids=lambda p: "pool%d_%d_%d" % p)
def test_roi_resampling_edges(emu, pools):
    hc.check_roi_resampling_edges(emu, *pools)


def test_roi_box_coordinates(emu):
    hc.check_roi_box_coordinates(emu)


@pytest.mark.parametrize("r", [64, 65])
def test_roi_counts(emu, r):
    hc.check_roi_counts(emu, r)


def test_roi_zero_rois(emu):
    hc.check_roi_zero_rois(emu)


def test_roi_overlap(emu):
    hc.check_roi_overlap(emu)


def test_roi_slabs(emu):
    hc.check_roi_slabs(emu)


# ---- C. NMS
@pytest.mark.parametrize("n", hc.NMS_SIZES)
def test_nms_sizes(emu, n):
    hc.check_nms_size(emu, n)


def test_nms_row_scan_child(emu, tmp_path):
    hc.check_nms_row_scan_child(emu, tmp_path)


def test_nms_max_num(emu):
    hc.check_nms_max_num(emu)


def test_nms_empty_and_limits(emu):
    hc.check_nms_empty_and_limits(emu)


def test_nms_thresholds(emu):
    hc.check_nms_thresholds(emu)


def test_nms_chain(emu):
    hc.check_nms_chain(emu)


@pytest.mark.parametrize("n", [65, 1025])
def test_nms_ties(emu, n):
    hc.check_nms_ties(emu, n)


# ---- D. targets and inference tail
@pytest.mark.parametrize("c", hc.UNMOLD_C)
def test_unmold_argmax(emu, c):
    hc.check_unmold_argmax(emu, c)


def test_unmold_argmax_constant(emu):
    hc.check_unmold_argmax_constant(emu)


def test_unmold_refusals(emu):
    hc.check_unmold_refusals(emu)


@pytest.mark.parametrize("c", [2, 3, 8])
def test_unmold_overlap(emu, c):
    hc.check_unmold_overlap(emu, c)


def test_unmold_overlap_counts(emu):
    hc.check_unmold_overlap_counts(emu)


def test_unmold_sweeps(emu):
    hc.check_unmold_sweeps(emu)


def test_mask_target_sweeps(emu):
    hc.check_mask_target_sweeps(emu)


def test_mask_target_coordinates(emu):
    hc.check_mask_target_coordinates(emu)


@pytest.mark.parametrize("name", sorted(hc.RESIZE_CASES))
def test_resize(emu, name):
    hc.check_resize(emu, name)


def test_resize_sweeps(emu):
    hc.check_resize_sweeps(emu)
