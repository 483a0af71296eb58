"""CPU tier of the connected-component path: the cases of cc_cases.py on the HIP emulator (the same kernel sources), then every one
of them again under guarded_memory(); the last test accounts for the entries of _lib.CC_EXPORTS."""
import sys

import pytest

import cc_cases as cc
import guard


@pytest.fixture()
def emu_direct(emu, monkeypatch):
    # (as in test_modules_emu.py: module-sized graphs run the direct kernels on the emulator)
    monkeypatch.setenv("CFUN_CONV_ALGO", "direct")
    return emu


@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bernoulli(emu, shape):
    cc.check_bernoulli_shape(emu, shape)


def test_random_tie(emu):
    cc.check_random_tie(emu)


def test_hand_tie(emu):
    cc.check_hand_tie(emu)


@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_serpentine(emu, shape):
    cc.check_serpentine(emu, shape)


@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_full_and_empty(emu, shape):
    cc.check_full_and_empty(emu, shape)


def test_diagonal_checkerboard(emu):
    cc.check_diagonal_checkerboard(emu)


def test_blob_and_specks(emu):
    cc.check_blob_and_specks(emu)


def test_values_beyond_k(emu):
    cc.check_values_beyond_k(emu)


def test_repeatable(emu):
    cc.check_repeatable(emu, (17, 10, 67))


def test_zero_sized_and_c_entry(emu):
    cc.check_zero_sized_and_c_entry(emu)


def test_wrapper_preconditions(emu):
    cc.check_wrapper_preconditions(emu)


def test_run_test_heart(emu_direct, tmp_path):
    cc.check_run_test_heart(emu_direct, tmp_path)


def test_run_test_lits(emu_direct, tmp_path):
    cc.check_run_test_lits(emu_direct, tmp_path)


# every case above a second time with every allocation guarded and poisoned, every dense input shadowed and the workspace
# exactly cfun_cc_workspace_bytes() large (tests/guard.py); verify() at the end of each
guard.guarded_copies(sys.modules[__name__], globals(), "guarded")


def test_zz_cc_entries_ran_under_guard_and_match_the_header():
    """Runs last in this file: cfun_cc.h's symbols equal _lib.CC_EXPORTS, the table is disjoint from the other four, and every
    launching entry of it was called under guarded_memory() by this file."""
    cc.check_coverage("emu")
