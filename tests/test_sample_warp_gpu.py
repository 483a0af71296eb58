"""GPU tier of the warp path: the cases of sample_warp_cases.py on the real libcfun_hip.so (cuda:0), then every one of them again
under guarded_memory(); the last test accounts for the entries of _lib.WARP_SAMPLE_EXPORTS."""
import sys

import pytest

import guard
import sample_warp_cases as wc

pytestmark = pytest.mark.gpu

_ids = lambda s: "x".join(map(str, s))


@pytest.mark.parametrize("shape", wc.W_CASES + wc.H_CASES + wc.D_CASES, ids=_ids)
def test_tile_edges(gpu, shape):
    wc.check_sweep(gpu, shape)


def test_brick_spans_one_two_four_control_cells(gpu):
    wc.check_cells_per_brick(gpu)


def test_grid_extents_two_three_max(gpu):
    wc.check_grid_extents(gpu)


def test_grid_coarser_equal_finer_than_the_brick(gpu):
    wc.check_grid_against_brick(gpu)


def test_every_flip_combination(gpu):
    wc.check_flips(gpu)


def test_eight_angles_scaled_up_and_down(gpu):
    wc.check_angles_and_scales(gpu)


def test_translation_partly_and_wholly_out(gpu):
    wc.check_translations(gpu)


def test_boxes_faces_plane_empty(gpu):
    wc.check_boxes(gpu)


def test_nan_source_and_nan_control_value(gpu):
    wc.check_non_finite(gpu)


def test_two_runs_bit_for_bit(gpu):
    wc.check_repeatable(gpu)


def test_equals_frame_rotate_resize_at_four_angles(gpu):
    wc.check_equals_frame_rotate_resize(gpu)


def test_misaligned_outputs_take_the_scalar_stores(gpu):
    wc.check_misaligned_outputs(gpu)


def test_refusals_write_nothing(gpu):
    wc.check_refusals(gpu)


def test_wrapper_preconditions(gpu):
    wc.check_wrapper_preconditions(gpu)


def test_gpu_shape(gpu):
    wc.check_gpu_shape(gpu)


@pytest.mark.parametrize("route", ["plain", "heart", "lits"])
def test_route_with_augment_feeds_train_epoch(gpu, route):
    wc.check_route(gpu, route)


# every case above a second time with every allocation guarded and poisoned, every dense input shadowed and the workspace
# exactly cfun_sample_warp_workspace_bytes() large (tests/guard.py); verify() at the end of each
guard.guarded_copies(sys.modules[__name__], globals(), "guarded")


def test_zz_warp_entries_ran_under_guard_and_match_the_header():
    """Runs last in this file: cfun_sample_warp.h's symbols equal _lib.WARP_SAMPLE_EXPORTS, the table is disjoint from the
    others, and every launching entry of it was called under guarded_memory() by this file."""
    wc.check_coverage("gpu")
