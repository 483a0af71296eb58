"""CPU tier of the scoring path: the cases of eval_cases.py on the HIP emulator (the same kernel sources), then every one of them
again under guarded_memory(); the last test accounts for the entries of _lib.EVAL_EXPORTS."""
import sys

import pytest

import eval_cases as ec
import guard


@pytest.fixture()
def emu_direct(emu, monkeypatch):
    # (as in test_modules_emu.py: module-sized graphs run the direct kernels on the emulator)
    monkeypatch.setenv("CFUN_CONV_ALGO", "direct")
    return emu


@pytest.mark.parametrize("shape", ec.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_counts(emu, shape):
    ec.check_counts_shape(emu, shape)


def test_strided_sources(emu):
    ec.check_strided_sources(emu)


def test_edge_cases(emu):
    ec.check_edge_cases(emu)


def test_wrapper_preconditions(emu):
    ec.check_wrapper_preconditions(emu)


def test_scores_against_the_reference(emu):
    ec.check_scores_golden(emu)


def test_run_test_heart(emu_direct, tmp_path):
    ec.check_run_test_heart(emu_direct, tmp_path)


def test_run_test_lits(emu_direct, tmp_path):
    ec.check_run_test_lits(emu_direct, tmp_path)


# every case above a second time with every allocation guarded and poisoned, every dense input shadowed and the workspace
# exactly cfun_seg_confusion_workspace_bytes() large (tests/guard.py); verify() at the end of each
guard.guarded_copies(sys.modules[__name__], globals(), "guarded")


def test_zz_eval_entries_ran_under_guard_and_match_the_header():
    """Runs last in this file: cfun_eval.h's symbols equal _lib.EVAL_EXPORTS, the table is disjoint from the other three, and every
    launching entry of it was called under guarded_memory() by this file."""
    ec.check_coverage("emu")
