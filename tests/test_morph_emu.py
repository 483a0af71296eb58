"""CPU tier of the ball morphology: the cases of morph_cases.py on the HIP emulator (the same kernel sources), then every one of
them again under guarded_memory(); the last test accounts for the entries of _lib.MORPH_EXPORTS."""
import sys

import pytest

import guard
import morph_cases as mc


@pytest.fixture()
def emu_direct(emu, monkeypatch):
    # (as in test_modules_emu.py: module-sized graphs run the direct kernels on the emulator)
    monkeypatch.setenv("CFUN_CONV_ALGO", "direct")
    return emu


@pytest.mark.parametrize("shape", mc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bernoulli(emu, shape):
    mc.check_bernoulli_shape(emu, shape)


def test_blobs(emu):
    mc.check_blobs(emu)


def test_hand_answers(emu):
    mc.check_hand_answers(emu)


def test_priority(emu):
    mc.check_priority(emu)


def test_selected_classes(emu):
    mc.check_selected_classes(emu)


def test_fill_value(emu):
    mc.check_fill_value(emu)


def test_identity_and_wide_cells(emu):
    mc.check_identity_and_wide_cells(emu)


def test_repeatable(emu):
    mc.check_repeatable(emu)


def test_zero_sized_and_c_entry(emu):
    mc.check_zero_sized_and_c_entry(emu)


def test_wrapper_preconditions(emu):
    mc.check_wrapper_preconditions(emu)


def test_value_object(emu):
    mc.check_value_object(emu)


def test_run_test_heart(emu_direct, tmp_path):
    mc.check_run_test_heart(emu_direct, tmp_path)


def test_run_test_lits(emu_direct, tmp_path):
    mc.check_run_test_lits(emu_direct, tmp_path)


# every case above a second time with every allocation guarded and poisoned, every dense input shadowed and the workspace
# exactly cfun_morph_workspace_bytes() large (tests/guard.py); verify() at the end of each
guard.guarded_copies(sys.modules[__name__], globals(), "guarded")


def test_zz_morph_entries_ran_under_guard_and_match_the_header():
    """Runs last in this file: cfun_morph.h's symbols equal _lib.MORPH_EXPORTS, the table is disjoint from the other eight, and
    every launching entry of it was called under guarded_memory() by this file."""
    mc.check_coverage("emu")
