"""CPU tier of the hole filling: the cases of fill_cases.py on the HIP emulator (the same kernel sources), then every one of them
again under guarded_memory(); the last test accounts for the entries of _lib.FILL_EXPORTS."""
import sys

import pytest

import fill_cases as fc
import guard


@pytest.fixture()
def emu_direct(emu, monkeypatch):
    # (as in test_modules_emu.py: module-sized graphs run the direct kernels on the emulator)
    monkeypatch.setenv("CFUN_CONV_ALGO", "direct")
    return emu


@pytest.mark.parametrize("shape", fc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bernoulli(emu, shape):
    fc.check_bernoulli_shape(emu, shape)


def test_cavity_across_seams(emu):
    fc.check_cavity_across_seams(emu)


def test_uniform_tiles(emu):
    fc.check_uniform_tiles(emu)


@pytest.mark.parametrize("shape", fc.INTERIOR, ids=lambda s: "x".join(map(str, s)))
def test_channel(emu, shape):
    fc.check_channel(emu, shape)


def test_priority(emu):
    fc.check_priority(emu)


def test_values_beyond_k(emu):
    fc.check_values_beyond_k(emu)


def test_fill_value(emu):
    fc.check_fill_value(emu)


def test_repeatable(emu):
    fc.check_repeatable(emu)


def test_zero_sized_and_c_entry(emu):
    fc.check_zero_sized_and_c_entry(emu)


def test_wrapper_preconditions(emu):
    fc.check_wrapper_preconditions(emu)


def test_value_object(emu):
    fc.check_value_object(emu)


def test_run_test_heart(emu_direct, tmp_path):
    fc.check_run_test_heart(emu_direct, tmp_path)


def test_run_test_lits(emu_direct, tmp_path):
    fc.check_run_test_lits(emu_direct, tmp_path)


# every case above a second time with every allocation guarded and poisoned, every dense input shadowed and the workspace
# exactly cfun_fill_workspace_bytes() large (tests/guard.py); verify() at the end of each
guard.guarded_copies(sys.modules[__name__], globals(), "guarded")


def test_zz_fill_entries_ran_under_guard_and_match_the_header():
    """Runs last in this file: cfun_fill.h's symbols equal _lib.FILL_EXPORTS, the table is disjoint from the other seven, and every
    launching entry of it was called under guarded_memory() by this file."""
    fc.check_coverage("emu")
