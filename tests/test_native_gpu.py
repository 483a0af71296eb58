"""GPU tier of the native-grid path: the cases of native_cases.py on the real libcfun_hip.so (cuda:0), then every one of them
again under guarded_memory(); the last test accounts for the entries of _lib.NATIVE_EXPORTS."""
import sys

import pytest

import guard
import native_cases as nc

pytestmark = pytest.mark.gpu

_ids = lambda t: "-".join("x".join(map(str, s)) for s in t)


@pytest.mark.parametrize("quad", nc.W_CASES + nc.H_CASES + nc.D_CASES, ids=_ids)
def test_mold_tile_edges(gpu, quad):
    nc.check_mold_sweep(gpu, quad)


def test_mold_ratios_per_axis(gpu):
    nc.check_mold_ratios(gpu)


def test_mold_extents_of_one(gpu):
    nc.check_mold_extents_of_one(gpu)


def test_mold_frame_fill_and_parity(gpu):
    nc.check_mold_frame_fill_and_parity(gpu)


def test_mold_dtypes_and_orders(gpu):
    nc.check_mold_dtypes_and_orders(gpu)


def test_mold_clip_and_normalise(gpu):
    nc.check_mold_clip_and_normalise(gpu)


def test_mold_non_finite_sources_spread(gpu):
    nc.check_mold_non_finite(gpu)


def test_mold_two_runs_bit_for_bit(gpu):
    nc.check_mold_repeatable(gpu)


def test_mold_refusals_write_nothing(gpu):
    nc.check_mold_refusals(gpu)


@pytest.mark.parametrize("pair", nc.MAP_EDGES, ids=_ids)
def test_map_tile_edges(gpu, pair):
    nc.check_map_edges(gpu, pair)


def test_map_extents_of_one(gpu):
    nc.check_map_extents_of_one(gpu)


def test_map_stride_pairs(gpu):
    nc.check_map_strides(gpu)


def test_map_refusals_write_nothing(gpu):
    nc.check_map_refusals(gpu)


def test_bench_shape(gpu):
    nc.check_bench_shape(gpu)


def test_spacing_and_shape_by_hand():
    nc.check_spacing_and_shape_by_hand()


def test_mold_inputs_native(gpu):
    nc.check_mold_inputs_native(gpu)


def test_detect_native(gpu):
    nc.check_detect_native(gpu)


def test_predict_for_submit(gpu, tmp_path):
    nc.check_predict_for_submit(gpu, tmp_path)


# every case above a second time with every allocation guarded and poisoned and every dense input shadowed (tests/guard.py);
# verify() at the end of each
guard.guarded_copies(sys.modules[__name__], globals(), "guarded")


def test_zz_native_entries_ran_under_guard_and_match_the_header():
    """Runs last in this file: cfun_native.h's symbols equal _lib.NATIVE_EXPORTS, the table is disjoint from the others, and both
    entries were called under guarded_memory() by this file."""
    nc.check_coverage("gpu")
