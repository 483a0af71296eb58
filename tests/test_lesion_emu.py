"""CPU tier of the lesion-scoring path: the cases of lesion_cases.py on the HIP emulator (the same kernel sources), then every one
of them again under guarded_memory(); the last test accounts for the entries of _lib.LESION_EXPORTS."""
import sys

import pytest

import guard
import lesion_cases as lc


@pytest.fixture()
def emu_direct(emu, monkeypatch):
    # (as in test_modules_emu.py: module-sized graphs run the direct kernels on the emulator)
    monkeypatch.setenv("CFUN_CONV_ALGO", "direct")
    return emu


def test_constants():
    lc.check_constants()


def test_rank_chunk_edges(emu):
    lc.check_rank_chunk_edges(emu)


def test_rank_many_chunks(emu):
    lc.check_rank_many_chunks(emu)


def test_rank_shapes(emu):
    lc.check_rank_shapes(emu)


def test_rank_checkerboard_full_empty(emu):
    lc.check_rank_checkerboard_full_empty(emu)


def test_rank_cap(emu):
    lc.check_rank_cap(emu)


def test_overlap_shapes(emu):
    lc.check_overlap_shapes(emu)


def test_overlap_many_workgroups(emu):
    lc.check_overlap_many_workgroups(emu)


def test_overlap_runs(emu):
    lc.check_overlap_runs(emu)


def test_overlap_table_full(emu):
    lc.check_overlap_table_full(emu)


def test_entries(emu):
    lc.check_entries(emu)


def test_repeatable(emu):
    lc.check_repeatable(emu)


def test_wrapper_preconditions(emu):
    lc.check_wrapper_preconditions(emu)


def test_planted(emu):
    lc.check_planted(emu)


def test_nan_rates(emu):
    lc.check_nan_rates(emu)


def test_run_test_lits(emu_direct, tmp_path):
    lc.check_run_test_lits(emu_direct, tmp_path)


# every case above a second time with every allocation guarded and poisoned, every dense input shadowed and the workspace
# exactly cfun_lesion_workspace_bytes() large (tests/guard.py); verify() at the end of each
guard.guarded_copies(sys.modules[__name__], globals(), "guarded")


def test_zz_lesion_entries_ran_under_guard_and_match_the_header():
    """Runs last in this file: cfun_lesion.h's symbols equal _lib.LESION_EXPORTS, the table is disjoint from the other six, and
    every launching entry of it was called under guarded_memory() by this file."""
    lc.check_coverage("emu")
