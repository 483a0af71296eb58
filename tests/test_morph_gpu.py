"""GPU tier of the ball morphology: the cases of morph_cases.py on the real libcfun_hip.so (cuda:0), then every one of them again
under guarded_memory(); the last test accounts for the entries of _lib.MORPH_EXPORTS."""
import sys

import pytest

import guard
import morph_cases as mc


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", mc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bernoulli(gpu, shape):
    mc.check_bernoulli_shape(gpu, shape)


def test_blobs(gpu):
    mc.check_blobs(gpu)


def test_hand_answers(gpu):
    mc.check_hand_answers(gpu)


def test_priority(gpu):
    mc.check_priority(gpu)


def test_selected_classes(gpu):
    mc.check_selected_classes(gpu)


def test_fill_value(gpu):
    mc.check_fill_value(gpu)


def test_identity_and_wide_cells(gpu):
    mc.check_identity_and_wide_cells(gpu)


def test_repeatable(gpu):
    mc.check_repeatable(gpu)


def test_big(gpu):
    mc.check_big(gpu)


def test_zero_sized_and_c_entry(gpu):
    mc.check_zero_sized_and_c_entry(gpu)


def test_wrapper_preconditions(gpu):
    mc.check_wrapper_preconditions(gpu)


def test_value_object(gpu):
    mc.check_value_object(gpu)


def test_run_test_heart(gpu, tmp_path):
    mc.check_run_test_heart(gpu, tmp_path)


def test_run_test_lits(gpu, tmp_path):
    mc.check_run_test_lits(gpu, tmp_path)


# every case above a second time with every allocation guarded and poisoned, every dense input shadowed and the workspace
# exactly cfun_morph_workspace_bytes() large (tests/guard.py); verify() at the end of each
guard.guarded_copies(sys.modules[__name__], globals(), "guarded")


def test_zz_morph_entries_ran_under_guard_and_match_the_header():
    """Runs last in this file: cfun_morph.h's symbols equal _lib.MORPH_EXPORTS, the table is disjoint from the other eight, and
    every launching entry of it was called under guarded_memory() by this file."""
    mc.check_coverage("gpu")
