"""CPU tier of the native-grid path: the cases of native_cases.py on the HIP emulator (the same kernel sources), then every one
of them again under guarded_memory(); the last test accounts for the entries of _lib.NATIVE_EXPORTS."""
import sys

import pytest

import guard
import native_cases as nc

_ids = lambda t: "-".join("x".join(map(str, s)) for s in t)


@pytest.fixture()
def emu_direct(emu, monkeypatch):
    # (as in test_modules_emu.py: module-sized graphs run the direct kernels on the emulator)
    monkeypatch.setenv("CFUN_CONV_ALGO", "direct")
    return emu


@pytest.mark.parametrize("quad", nc.W_CASES + nc.H_CASES + nc.D_CASES, ids=_ids)
def test_mold_tile_edges(emu, quad):
    nc.check_mold_sweep(emu, quad)


def test_mold_ratios_per_axis(emu):
    nc.check_mold_ratios(emu)


def test_mold_extents_of_one(emu):
    nc.check_mold_extents_of_one(emu)


def test_mold_frame_fill_and_parity(emu):
    nc.check_mold_frame_fill_and_parity(emu)


def test_mold_dtypes_and_orders(emu):
    nc.check_mold_dtypes_and_orders(emu)


def test_mold_clip_and_normalise(emu):
    nc.check_mold_clip_and_normalise(emu)


def test_mold_non_finite_sources_spread(emu):
    nc.check_mold_non_finite(emu)


def test_mold_two_runs_bit_for_bit(emu):
    nc.check_mold_repeatable(emu)


def test_mold_refusals_write_nothing(emu):
    nc.check_mold_refusals(emu)


@pytest.mark.parametrize("pair", nc.MAP_EDGES, ids=_ids)
def test_map_tile_edges(emu, pair):
    nc.check_map_edges(emu, pair)


def test_map_extents_of_one(emu):
    nc.check_map_extents_of_one(emu)


def test_map_stride_pairs(emu):
    nc.check_map_strides(emu)


def test_map_refusals_write_nothing(emu):
    nc.check_map_refusals(emu)


def test_spacing_and_shape_by_hand():
    nc.check_spacing_and_shape_by_hand()


def test_mold_inputs_native(emu):
    nc.check_mold_inputs_native(emu)


def test_detect_native(emu_direct):
    nc.check_detect_native(emu_direct)


def test_predict_for_submit(emu_direct, tmp_path):
    nc.check_predict_for_submit(emu_direct, tmp_path)


# every case above a second time with every allocation guarded and poisoned and every dense input shadowed (tests/guard.py);
# verify() at the end of each
guard.guarded_copies(sys.modules[__name__], globals(), "guarded")


def test_zz_native_entries_ran_under_guard_and_match_the_header():
    """Runs last in this file: cfun_native.h's symbols equal _lib.NATIVE_EXPORTS, the table is disjoint from the others, and both
    entries were called under guarded_memory() by this file."""
    nc.check_coverage("emu")
