"""CPU tier of the surface-distance path: the cases of surface_cases.py on the HIP emulator (the same kernel sources), then every
one of them again under guarded_memory(); the last test accounts for the entries of _lib.SURFACE_EXPORTS."""
import sys

import pytest

import guard
import surface_cases as sc


@pytest.fixture()
def emu_direct(emu, monkeypatch):
    # (as in test_modules_emu.py: module-sized graphs run the direct kernels on the emulator)
    monkeypatch.setenv("CFUN_CONV_ALGO", "direct")
    return emu


def _id(s):
    return "x".join(map(str, s))


@pytest.mark.parametrize("shape", sc.SHAPES, ids=_id)
def test_bernoulli_field(emu, shape):
    sc.check_bernoulli_field(emu, shape)


@pytest.mark.parametrize("shape", sc.SHAPES, ids=_id)
def test_bernoulli_stats(emu, shape):
    sc.check_bernoulli_stats(emu, shape)


@pytest.mark.parametrize("shape", sc.slab_shapes(), ids=_id)
def test_slab_shape(emu, shape):
    sc.check_slab_shape(emu, shape)


def test_ellipsoids(emu):
    sc.check_ellipsoids(emu)


@pytest.mark.parametrize("shape", sc.SHAPES, ids=_id)
def test_full_and_empty(emu, shape):
    sc.check_full_and_empty(emu, shape)


def test_absent_and_beyond(emu):
    sc.check_absent_and_beyond(emu)


def test_label_dtypes(emu):
    sc.check_label_dtypes(emu)


def test_repeatable(emu):
    sc.check_repeatable(emu, (17, 10, 67))


def test_zero_sized_and_c_entry(emu):
    sc.check_zero_sized_and_c_entry(emu)


def test_wrapper_preconditions(emu):
    sc.check_wrapper_preconditions(emu)


def test_run_test_heart(emu_direct, tmp_path):
    sc.check_run_test_heart(emu_direct, tmp_path)


def test_run_test_lits(emu_direct, tmp_path):
    sc.check_run_test_lits(emu_direct, tmp_path)


# every case above a second time with every allocation guarded and poisoned, every dense input shadowed and the workspace
# exactly cfun_surface_workspace_bytes() large (tests/guard.py); verify() at the end of each
guard.guarded_copies(sys.modules[__name__], globals(), "guarded")


def test_zz_surface_entries_ran_under_guard_and_match_the_header():
    """Runs last in this file: cfun_surface.h's symbols equal _lib.SURFACE_EXPORTS, the table is disjoint from the other five,
    and every launching entry of it was called under guarded_memory() by this file."""
    sc.check_coverage("emu")
