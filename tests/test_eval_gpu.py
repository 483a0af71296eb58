"""GPU tier of the scoring path: the cases of eval_cases.py on the real libcfun_hip.so (cuda:0), then every one of them again under
guarded_memory(); the last test accounts for the entries of _lib.EVAL_EXPORTS."""
import sys

import pytest

import eval_cases as ec
import guard

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", ec.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_counts(gpu, shape):
    ec.check_counts_shape(gpu, shape)


def test_strided_sources(gpu):
    ec.check_strided_sources(gpu)


def test_edge_cases(gpu):
    ec.check_edge_cases(gpu)


def test_wrapper_preconditions(gpu):
    ec.check_wrapper_preconditions(gpu)


def test_scores_against_the_reference(gpu):
    ec.check_scores_golden(gpu)


def test_run_test_heart(gpu, tmp_path):
    ec.check_run_test_heart(gpu, tmp_path)


def test_run_test_lits(gpu, tmp_path):
    ec.check_run_test_lits(gpu, tmp_path)


# every case above a second time with every allocation guarded and poisoned, every dense input shadowed and the workspace
# exactly cfun_seg_confusion_workspace_bytes() large (tests/guard.py); verify() at the end of each
guard.guarded_copies(sys.modules[__name__], globals(), "guarded")


def test_zz_eval_entries_ran_under_guard_and_match_the_header():
    """Runs last in this file: cfun_eval.h's symbols equal _lib.EVAL_EXPORTS, the table is disjoint from the other three, and every
    launching entry of it was called under guarded_memory() by this file."""
    ec.check_coverage("gpu")
