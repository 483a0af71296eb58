"""CPU tier of the heart sample path: the cases of sample_heart_cases.py on the HIP emulator (the same kernel sources), then every
one of them again under guarded_memory(); the last test accounts for the entries of _lib.HEART_SAMPLE_EXPORTS."""
import sys

import pytest

import guard
import sample_heart_cases as hc

_ids = lambda t: "-".join("x".join(map(str, s)) for s in t)


@pytest.fixture()
def emu_direct(emu, monkeypatch):
    # (as in test_modules_emu.py: module-sized graphs run the direct kernels on the emulator)
    monkeypatch.setenv("CFUN_CONV_ALGO", "direct")
    return emu


@pytest.mark.parametrize("pair", hc.W_CASES + hc.H_CASES + hc.D_CASES, ids=_ids)
def test_tile_edges(emu, pair):
    hc.check_sweep(emu, pair)


def test_ratios_per_axis(emu):
    hc.check_ratios(emu)


def test_extents_of_one(emu):
    hc.check_extents_of_one(emu)


def test_angles(emu):
    hc.check_angles(emu)


def test_image_and_label_dtypes(emu):
    hc.check_dtypes(emu)


def test_memory_orders(emu):
    hc.check_orders(emu)


def test_clip_absent_inactive_active(emu):
    hc.check_clip(emu)


def test_truncation_by_hand(emu):
    hc.check_truncate_by_hand(emu)


def test_label_null(emu):
    hc.check_no_label(emu)


def test_boxes_faces_plane_empty(emu):
    hc.check_boxes(emu)


def test_nan_source_and_all_zero_volume(emu):
    hc.check_non_finite_and_zero(emu)


def test_two_runs_bit_for_bit(emu):
    hc.check_repeatable(emu)


def test_refusals_write_nothing(emu):
    hc.check_refusals(emu)


def test_bad_source_extent(emu):
    hc.check_bad_source_extent(emu)


def test_wrapper_preconditions(emu):
    hc.check_wrapper_preconditions(emu)


def test_make_sample_heart_feeds_train_epoch(emu_direct):
    hc.check_make_sample_heart_feeds_train_epoch(emu_direct)


def test_consistent_with_the_composed_route(emu_direct):
    hc.check_consistent_with_the_composed_route(emu_direct)


def test_detect_heart(emu_direct):
    hc.check_detect_heart(emu_direct)


# every case above a second time with every allocation guarded and poisoned, every dense input shadowed and the workspace
# exactly cfun_sample_heart_workspace_bytes() large (tests/guard.py); verify() at the end of each
guard.guarded_copies(sys.modules[__name__], globals(), "guarded")


def test_zz_heart_sample_entries_ran_under_guard_and_match_the_header():
    """Runs last in this file: cfun_sample_heart.h's symbols equal _lib.HEART_SAMPLE_EXPORTS, the table is disjoint from the
    others, and every launching entry of it was called under guarded_memory() by this file."""
    hc.check_coverage("emu")
