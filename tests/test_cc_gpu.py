"""GPU tier of the connected-component path: the cases of cc_cases.py on the real libcfun_hip.so (cuda:0), then every one of them
again under guarded_memory(); the last test accounts for the entries of _lib.CC_EXPORTS."""
import sys

import pytest

import cc_cases as cc
import guard

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bernoulli(gpu, shape):
    cc.check_bernoulli_shape(gpu, shape)


def test_random_tie(gpu):
    cc.check_random_tie(gpu)


def test_hand_tie(gpu):
    cc.check_hand_tie(gpu)


@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_serpentine(gpu, shape):
    cc.check_serpentine(gpu, shape)


@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_full_and_empty(gpu, shape):
    cc.check_full_and_empty(gpu, shape)


def test_diagonal_checkerboard(gpu):
    cc.check_diagonal_checkerboard(gpu)


def test_blob_and_specks(gpu):
    cc.check_blob_and_specks(gpu)


def test_values_beyond_k(gpu):
    cc.check_values_beyond_k(gpu)


def test_repeatable(gpu):
    cc.check_repeatable(gpu, (17, 10, 67))


def test_big(gpu):
    cc.check_big(gpu)


def test_zero_sized_and_c_entry(gpu):
    cc.check_zero_sized_and_c_entry(gpu)


def test_wrapper_preconditions(gpu):
    cc.check_wrapper_preconditions(gpu)


def test_run_test_heart(gpu, tmp_path):
    cc.check_run_test_heart(gpu, tmp_path)


def test_run_test_lits(gpu, tmp_path):
    cc.check_run_test_lits(gpu, tmp_path)


# every case above a second time with every allocation guarded and poisoned, every dense input shadowed and the workspace
# exactly cfun_cc_workspace_bytes() large (tests/guard.py); verify() at the end of each
guard.guarded_copies(sys.modules[__name__], globals(), "guarded")


def test_zz_cc_entries_ran_under_guard_and_match_the_header():
    """Runs last in this file: cfun_cc.h's symbols equal _lib.CC_EXPORTS, the table is disjoint from the other four, and every
    launching entry of it was called under guarded_memory() by this file."""
    cc.check_coverage("gpu")
