"""CPU tier of the training-sample path: the cases of sample_cases.py on the HIP emulator (the same kernel sources), then every
one of them again under guarded_memory(); the last test accounts for the entries of _lib.SAMPLE_EXPORTS."""
import sys

import pytest

import guard
import sample_cases as sc


@pytest.fixture()
def emu_direct(emu, monkeypatch):
    # (as in test_modules_emu.py: module-sized graphs run the direct kernels on the emulator)
    monkeypatch.setenv("CFUN_CONV_ALGO", "direct")
    return emu


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rotate_and_box(emu, shape):
    sc.check_rotate_shape(emu, shape)


def test_rotate_strided_sources(emu):
    sc.check_rotate_strided(emu)


def test_boxes_faces_plane_empty(emu):
    sc.check_rotate_boxes(emu)


def test_rotate_wrapper_preconditions(emu):
    sc.check_rotate_wrapper_preconditions(emu)


@pytest.mark.parametrize("tag", ["bt875", "bt1001"])
def test_rpn_targets_golden_and_keys(emu, tag):
    sc.check_targets_golden(emu, tag)


def test_rpn_targets_few_negatives(emu):
    sc.check_targets_few_negatives(emu)


def test_rpn_targets_random_keys(emu):
    sc.check_targets_random_keys(emu)


def test_rpn_targets_zero_size(emu):
    sc.check_targets_zero_size(emu)


@pytest.mark.parametrize("tag", ["main13", "main0", "lits"])
def test_load_image_gt_golden(emu, tag):
    sc.check_load_image_gt_golden(emu, tag)


def test_make_sample_feeds_train_epoch(emu_direct):
    sc.check_make_sample_feeds_train_epoch(emu_direct)


# every case above a second time with every allocation guarded and poisoned, every dense input shadowed and the workspace
# exactly cfun_sample_workspace_bytes() large (tests/guard.py); verify() at the end of each
guard.guarded_copies(sys.modules[__name__], globals(), "guarded")


def test_zz_sample_entries_ran_under_guard_and_match_the_header():
    """Runs last in this file: cfun_sample.h's symbols equal _lib.SAMPLE_EXPORTS, and every launching entry of that table was
    called under guarded_memory() by this file."""
    sc.check_coverage("emu")
