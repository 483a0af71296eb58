"""GPU tier of the hole filling: the cases of fill_cases.py on the real libcfun_hip.so (cuda:0), then every one of them again under
guarded_memory(); the last test accounts for the entries of _lib.FILL_EXPORTS."""
import sys

import pytest

import fill_cases as fc
import guard

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", fc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bernoulli(gpu, shape):
    fc.check_bernoulli_shape(gpu, shape)


def test_cavity_across_seams(gpu):
    fc.check_cavity_across_seams(gpu)


def test_uniform_tiles(gpu):
    fc.check_uniform_tiles(gpu)


@pytest.mark.parametrize("shape", fc.INTERIOR, ids=lambda s: "x".join(map(str, s)))
def test_channel(gpu, shape):
    fc.check_channel(gpu, shape)


def test_priority(gpu):
    fc.check_priority(gpu)


def test_values_beyond_k(gpu):
    fc.check_values_beyond_k(gpu)


def test_fill_value(gpu):
    fc.check_fill_value(gpu)


def test_repeatable(gpu):
    fc.check_repeatable(gpu)


def test_big(gpu):
    fc.check_big(gpu)


def test_zero_sized_and_c_entry(gpu):
    fc.check_zero_sized_and_c_entry(gpu)


def test_wrapper_preconditions(gpu):
    fc.check_wrapper_preconditions(gpu)


def test_value_object(gpu):
    fc.check_value_object(gpu)


def test_run_test_heart(gpu, tmp_path):
    fc.check_run_test_heart(gpu, tmp_path)


def test_run_test_lits(gpu, tmp_path):
    fc.check_run_test_lits(gpu, tmp_path)


# every case above a second time with every allocation guarded and poisoned, every dense input shadowed and the workspace
# exactly cfun_fill_workspace_bytes() large (tests/guard.py); verify() at the end of each
guard.guarded_copies(sys.modules[__name__], globals(), "guarded")


def test_zz_fill_entries_ran_under_guard_and_match_the_header():
    """Runs last in this file: cfun_fill.h's symbols equal _lib.FILL_EXPORTS, the table is disjoint from the other seven, and every
    launching entry of it was called under guarded_memory() by this file."""
    fc.check_coverage("gpu")
