"""GPU tier of the heart sample path: the cases of sample_heart_cases.py on the real libcfun_hip.so (cuda:0), then every one of
them again under guarded_memory(); the last test accounts for the entries of _lib.HEART_SAMPLE_EXPORTS."""
import sys

import pytest

import guard
import sample_heart_cases as hc

pytestmark = pytest.mark.gpu

_ids = lambda t: "-".join("x".join(map(str, s)) for s in t)


@pytest.mark.parametrize("pair", hc.W_CASES + hc.H_CASES + hc.D_CASES, ids=_ids)
def test_tile_edges(gpu, pair):
    hc.check_sweep(gpu, pair)


def test_ratios_per_axis(gpu):
    hc.check_ratios(gpu)


def test_extents_of_one(gpu):
    hc.check_extents_of_one(gpu)


def test_angles(gpu):
    hc.check_angles(gpu)


def test_image_and_label_dtypes(gpu):
    hc.check_dtypes(gpu)


def test_memory_orders(gpu):
    hc.check_orders(gpu)


def test_clip_absent_inactive_active(gpu):
    hc.check_clip(gpu)


def test_truncation_by_hand(gpu):
    hc.check_truncate_by_hand(gpu)


def test_label_null(gpu):
    hc.check_no_label(gpu)


def test_boxes_faces_plane_empty(gpu):
    hc.check_boxes(gpu)


def test_nan_source_and_all_zero_volume(gpu):
    hc.check_non_finite_and_zero(gpu)


def test_two_runs_bit_for_bit(gpu):
    hc.check_repeatable(gpu)


def test_refusals_write_nothing(gpu):
    hc.check_refusals(gpu)


def test_bad_source_extent(gpu):
    hc.check_bad_source_extent(gpu)


def test_wrapper_preconditions(gpu):
    hc.check_wrapper_preconditions(gpu)


def test_gpu_shape(gpu):
    hc.check_gpu_shape(gpu)


def test_make_sample_heart_feeds_train_epoch(gpu):
    hc.check_make_sample_heart_feeds_train_epoch(gpu)


def test_consistent_with_the_composed_route(gpu):
    hc.check_consistent_with_the_composed_route(gpu)


def test_detect_heart(gpu):
    hc.check_detect_heart(gpu)


# every case above a second time with every allocation guarded and poisoned, every dense input shadowed and the workspace
# exactly cfun_sample_heart_workspace_bytes() large (tests/guard.py); verify() at the end of each
guard.guarded_copies(sys.modules[__name__], globals(), "guarded")


def test_zz_heart_sample_entries_ran_under_guard_and_match_the_header():
    """Runs last in this file: cfun_sample_heart.h's symbols equal _lib.HEART_SAMPLE_EXPORTS, the table is disjoint from the
    others, and every launching entry of it was called under guarded_memory() by this file."""
    hc.check_coverage("gpu")
