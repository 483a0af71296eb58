"""GPU tier of the LiTS sample path: the cases of sample_lits_cases.py on the real libcfun_hip.so (cuda:0), then every
one of them again under guarded_memory(); the last test accounts for the entries of _lib.LITS_SAMPLE_EXPORTS."""
import sys

import pytest

import guard
import sample_lits_cases as lc

pytestmark = pytest.mark.gpu

_ids = lambda t: "-".join("x".join(map(str, s)) for s in t)


@pytest.mark.parametrize("triple", lc.W_CASES + lc.D_CASES, ids=_ids)
def test_tile_edges(gpu, triple):
    lc.check_sweep(gpu, triple)


def test_angles(gpu):
    lc.check_angles(gpu)


def test_offsets_and_extents(gpu):
    lc.check_offsets_and_extents(gpu)


def test_label_dtypes(gpu):
    lc.check_label_dtypes(gpu)


def test_strided_sources(gpu):
    lc.check_strided_sources(gpu)


def test_normalisation(gpu):
    lc.check_normalisation(gpu)


def test_boxes_faces_plane_empty(gpu):
    lc.check_boxes(gpu)


def test_two_runs_bit_for_bit(gpu):
    lc.check_repeatable(gpu)


def test_equals_the_existing_device_routes(gpu):
    lc.check_equals_the_existing_device_routes(gpu)


def test_refusals_write_nothing(gpu):
    lc.check_refusals(gpu)


def test_source_at_the_far_faces(gpu):
    lc.check_far_faces(gpu)


def test_product_shape(gpu):
    lc.check_product_shape(gpu)


def test_wrapper_preconditions(gpu):
    lc.check_wrapper_preconditions(gpu)


def test_draw_angle_and_config():
    lc.check_draw_angle_and_config()


def test_make_sample_lits_feeds_train_epoch(gpu):
    lc.check_make_sample_lits_feeds_train_epoch(gpu)


# every case above a second time with every allocation guarded and poisoned, every dense input shadowed and the workspace
# exactly cfun_sample_lits_workspace_bytes() large (tests/guard.py); verify() at the end of each
guard.guarded_copies(sys.modules[__name__], globals(), "guarded")


def test_zz_lits_sample_entries_ran_under_guard_and_match_the_header():
    """Runs last in this file: cfun_sample_lits.h's symbols equal _lib.LITS_SAMPLE_EXPORTS, and every launching entry of that
    table was called under guarded_memory() by this file."""
    lc.check_coverage("gpu")
