"""CPU tier of the warp path: the cases of sample_warp_cases.py on the HIP emulator (the same kernel sources), then every one of
them again under guarded_memory(); the last test accounts for the entries of _lib.WARP_SAMPLE_EXPORTS."""
import sys

import pytest

import guard
import sample_warp_cases as wc

_ids = lambda s: "x".join(map(str, s))


@pytest.fixture()
def emu_direct(emu, monkeypatch):
    # (as in test_modules_emu.py: module-sized graphs run the direct kernels on the emulator)
    monkeypatch.setenv("CFUN_CONV_ALGO", "direct")
    return emu


@pytest.mark.parametrize("shape", wc.W_CASES + wc.H_CASES + wc.D_CASES, ids=_ids)
def test_tile_edges(emu, shape):
    wc.check_sweep(emu, shape)


def test_brick_spans_one_two_four_control_cells(emu):
    wc.check_cells_per_brick(emu)


def test_grid_extents_two_three_max(emu):
    wc.check_grid_extents(emu)


def test_grid_coarser_equal_finer_than_the_brick(emu):
    wc.check_grid_against_brick(emu)


def test_every_flip_combination(emu):
    wc.check_flips(emu)


def test_eight_angles_scaled_up_and_down(emu):
    wc.check_angles_and_scales(emu)


def test_translation_partly_and_wholly_out(emu):
    wc.check_translations(emu)


def test_boxes_faces_plane_empty(emu):
    wc.check_boxes(emu)


def test_nan_source_and_nan_control_value(emu):
    wc.check_non_finite(emu)


def test_two_runs_bit_for_bit(emu):
    wc.check_repeatable(emu)


def test_equals_frame_rotate_resize_at_four_angles(emu):
    wc.check_equals_frame_rotate_resize(emu)


def test_misaligned_outputs_take_the_scalar_stores(emu):
    wc.check_misaligned_outputs(emu)


def test_refusals_write_nothing(emu):
    wc.check_refusals(emu)


def test_wrapper_preconditions(emu):
    wc.check_wrapper_preconditions(emu)


def test_draw_warp():
    wc.check_draw_warp()


@pytest.mark.parametrize("route", ["plain", "heart", "lits"])
def test_route_with_augment_feeds_train_epoch(emu_direct, route):
    wc.check_route(emu_direct, route)


# every case above a second time with every allocation guarded and poisoned, every dense input shadowed and the workspace
# exactly cfun_sample_warp_workspace_bytes() large (tests/guard.py); verify() at the end of each
guard.guarded_copies(sys.modules[__name__], globals(), "guarded")


def test_zz_warp_entries_ran_under_guard_and_match_the_header():
    """Runs last in this file: cfun_sample_warp.h's symbols equal _lib.WARP_SAMPLE_EXPORTS, the table is disjoint from the
    others, and every launching entry of it was called under guarded_memory() by this file."""
    wc.check_coverage("emu")
