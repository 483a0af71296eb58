"""GPU tier of the lesion-scoring path: the cases of lesion_cases.py on the real libcfun_hip.so (cuda:0), then every one of them
again under guarded_memory(); the last test accounts for the entries of _lib.LESION_EXPORTS."""
import sys

import pytest

import guard
import lesion_cases as lc

pytestmark = pytest.mark.gpu


def test_constants():
    lc.check_constants()


def test_rank_chunk_edges(gpu):
    lc.check_rank_chunk_edges(gpu)


def test_rank_many_chunks(gpu):
    lc.check_rank_many_chunks(gpu)


def test_rank_shapes(gpu):
    lc.check_rank_shapes(gpu)


def test_rank_checkerboard_full_empty(gpu):
    lc.check_rank_checkerboard_full_empty(gpu)


def test_rank_cap(gpu):
    lc.check_rank_cap(gpu)


def test_overlap_shapes(gpu):
    lc.check_overlap_shapes(gpu)


def test_overlap_many_workgroups(gpu):
    lc.check_overlap_many_workgroups(gpu)


def test_overlap_runs(gpu):
    lc.check_overlap_runs(gpu)


def test_overlap_table_full(gpu):
    lc.check_overlap_table_full(gpu)


def test_entries(gpu):
    lc.check_entries(gpu)


def test_repeatable(gpu):
    lc.check_repeatable(gpu)


def test_wrapper_preconditions(gpu):
    lc.check_wrapper_preconditions(gpu)


def test_planted(gpu):
    lc.check_planted(gpu)


def test_nan_rates(gpu):
    lc.check_nan_rates(gpu)


def test_run_test_lits(gpu, tmp_path):
    lc.check_run_test_lits(gpu, tmp_path)


# every case above a second time with every allocation guarded and poisoned, every dense input shadowed and the workspace
# exactly cfun_lesion_workspace_bytes() large (tests/guard.py); verify() at the end of each
guard.guarded_copies(sys.modules[__name__], globals(), "guarded")


def test_zz_lesion_entries_ran_under_guard_and_match_the_header():
    """Runs last in this file: cfun_lesion.h's symbols equal _lib.LESION_EXPORTS, the table is disjoint from the other six, and
    every launching entry of it was called under guarded_memory() by this file."""
    lc.check_coverage("gpu")
