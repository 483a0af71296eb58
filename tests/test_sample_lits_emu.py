"""CPU tier of the LiTS sample path: the cases of sample_lits_cases.py on the HIP emulator (the same kernel sources), then every
one of them again under guarded_memory(); the last test accounts for the entries of _lib.LITS_SAMPLE_EXPORTS."""
import sys

import pytest

import guard
import sample_lits_cases as lc

_ids = lambda t: "-".join("x".join(map(str, s)) for s in t)


@pytest.fixture()
def emu_direct(emu, monkeypatch):
    # (as in test_modules_emu.py: module-sized graphs run the direct kernels on the emulator)
    monkeypatch.setenv("CFUN_CONV_ALGO", "direct")
    return emu


@pytest.mark.parametrize("triple", lc.W_CASES + lc.D_CASES, ids=_ids)
def test_tile_edges(emu, triple):
    lc.check_sweep(emu, triple)


def test_angles(emu):
    lc.check_angles(emu)


def test_offsets_and_extents(emu):
    lc.check_offsets_and_extents(emu)


def test_label_dtypes(emu):
    lc.check_label_dtypes(emu)


def test_strided_sources(emu):
    lc.check_strided_sources(emu)


def test_normalisation(emu):
    lc.check_normalisation(emu)


def test_boxes_faces_plane_empty(emu):
    lc.check_boxes(emu)


def test_two_runs_bit_for_bit(emu):
    lc.check_repeatable(emu)


def test_equals_the_existing_device_routes(emu):
    lc.check_equals_the_existing_device_routes(emu)


def test_refusals_write_nothing(emu):
    lc.check_refusals(emu)


def test_source_at_the_far_faces(emu):
    lc.check_far_faces(emu)


def test_wrapper_preconditions(emu):
    lc.check_wrapper_preconditions(emu)


def test_draw_angle_and_config():
    lc.check_draw_angle_and_config()


def test_make_sample_lits_feeds_train_epoch(emu_direct):
    lc.check_make_sample_lits_feeds_train_epoch(emu_direct)


# every case above a second time with every allocation guarded and poisoned, every dense input shadowed and the workspace
# exactly cfun_sample_lits_workspace_bytes() large (tests/guard.py); verify() at the end of each
guard.guarded_copies(sys.modules[__name__], globals(), "guarded")


def test_zz_lits_sample_entries_ran_under_guard_and_match_the_header():
    """Runs last in this file: cfun_sample_lits.h's symbols equal _lib.LITS_SAMPLE_EXPORTS, and every launching entry of that
    table was called under guarded_memory() by this file."""
    lc.check_coverage("emu")
