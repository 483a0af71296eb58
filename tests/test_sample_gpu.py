"""GPU tier of the training-sample path: the cases of sample_cases.py on the real libcfun_hip.so (cuda:0), then every one of them
again under guarded_memory(); the last test accounts for the entries of _lib.SAMPLE_EXPORTS."""
import sys

import pytest

import guard
import sample_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rotate_and_box(gpu, shape):
    sc.check_rotate_shape(gpu, shape)


def test_rotate_strided_sources(gpu):
    sc.check_rotate_strided(gpu)


def test_boxes_faces_plane_empty(gpu):
    sc.check_rotate_boxes(gpu)


def test_rotate_wrapper_preconditions(gpu):
    sc.check_rotate_wrapper_preconditions(gpu)


@pytest.mark.parametrize("tag", ["bt875", "bt1001"])
def test_rpn_targets_golden_and_keys(gpu, tag):
    sc.check_targets_golden(gpu, tag)


def test_rpn_targets_few_negatives(gpu):
    sc.check_targets_few_negatives(gpu)


def test_rpn_targets_random_keys(gpu):
    sc.check_targets_random_keys(gpu)


def test_rpn_targets_zero_size(gpu):
    sc.check_targets_zero_size(gpu)


@pytest.mark.parametrize("tag", ["main13", "main0", "lits"])
def test_load_image_gt_golden(gpu, tag):
    sc.check_load_image_gt_golden(gpu, tag)


def test_make_sample_feeds_train_epoch(gpu):
    sc.check_make_sample_feeds_train_epoch(gpu)


# every case above a second time with every allocation guarded and poisoned, every dense input shadowed and the workspace
# exactly cfun_sample_workspace_bytes() large (tests/guard.py); verify() at the end of each
guard.guarded_copies(sys.modules[__name__], globals(), "guarded")


def test_zz_sample_entries_ran_under_guard_and_match_the_header():
    """Runs last in this file: cfun_sample.h's symbols equal _lib.SAMPLE_EXPORTS, and every launching entry of that table was
    called under guarded_memory() by this file."""
    sc.check_coverage("gpu")
