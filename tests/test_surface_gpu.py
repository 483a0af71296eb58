"""GPU tier of the surface-distance path: the cases of surface_cases.py on the real libcfun_hip.so (cuda:0), then every one of
them again under guarded_memory(); the last test accounts for the entries of _lib.SURFACE_EXPORTS."""
import sys

import pytest

import guard
import surface_cases as sc

pytestmark = pytest.mark.gpu


def _id(s):
    return "x".join(map(str, s))


@pytest.mark.parametrize("shape", sc.SHAPES, ids=_id)
def test_bernoulli_field(gpu, shape):
    sc.check_bernoulli_field(gpu, shape)


@pytest.mark.parametrize("shape", sc.SHAPES, ids=_id)
def test_bernoulli_stats(gpu, shape):
    sc.check_bernoulli_stats(gpu, shape)


@pytest.mark.parametrize("shape", sc.slab_shapes(), ids=_id)
def test_slab_shape(gpu, shape):
    sc.check_slab_shape(gpu, shape)


def test_ellipsoids(gpu):
    sc.check_ellipsoids(gpu)


@pytest.mark.parametrize("shape", sc.SHAPES, ids=_id)
def test_full_and_empty(gpu, shape):
    sc.check_full_and_empty(gpu, shape)


def test_absent_and_beyond(gpu):
    sc.check_absent_and_beyond(gpu)


def test_label_dtypes(gpu):
    sc.check_label_dtypes(gpu)


def test_repeatable(gpu):
    sc.check_repeatable(gpu, (17, 10, 67))


def test_big(gpu):
    sc.check_big(gpu)


def test_zero_sized_and_c_entry(gpu):
    sc.check_zero_sized_and_c_entry(gpu)


def test_wrapper_preconditions(gpu):
    sc.check_wrapper_preconditions(gpu)


def test_run_test_heart(gpu, tmp_path):
    sc.check_run_test_heart(gpu, tmp_path)


def test_run_test_lits(gpu, tmp_path):
    sc.check_run_test_lits(gpu, tmp_path)


# every case above a second time with every allocation guarded and poisoned, every dense input shadowed and the workspace
# exactly cfun_surface_workspace_bytes() large (tests/guard.py); verify() at the end of each
guard.guarded_copies(sys.modules[__name__], globals(), "guarded")


def test_zz_surface_entries_ran_under_guard_and_match_the_header():
    """Runs last in this file: cfun_surface.h's symbols equal _lib.SURFACE_EXPORTS, the table is disjoint from the other five,
    and every launching entry of it was called under guarded_memory() by this file."""
    sc.check_coverage("gpu")
