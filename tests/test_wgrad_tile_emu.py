"""CPU tier (HIP emulator) of the weight-gradient tile geometry: every case of wgrad_tile_cases.py once as G16 and once as G8."""
import pytest

import wgrad_tile_cases as wt
from cfun_amd._lib import ALGO_MFMA, ALGO_WINO


@pytest.mark.parametrize("name", sorted(wt.DIRECT_CASES))
def test_direct_wgrad_both_geometries(emu, name):
    n, dhw, ci, co, k, kw = wt.DIRECT_CASES[name]
    wt.check_conv_both(emu, n, dhw, ci, co, k, ALGO_MFMA, kw)


@pytest.mark.parametrize("name", sorted(wt.FUSED_CASES))
def test_fused_wgrad_both_geometries(emu, name):
    n, dhw, ci, co, k, kw = wt.FUSED_CASES[name]
    wt.check_conv_both(emu, n, dhw, ci, co, k, ALGO_MFMA, kw)


@pytest.mark.parametrize("name", sorted(wt.FOLD_CASES))
def test_folded_wgrad_both_geometries(emu, name):
    wt.check_fold_both(emu, *wt.FOLD_CASES[name])


@pytest.mark.parametrize("name", sorted(wt.WINO_CASES))
def test_winograd_wgrad_both_geometries(emu, name):
    n, dhw, ci, co, k, kw = wt.WINO_CASES[name]
    wt.check_conv_both(emu, n, dhw, ci, co, k, ALGO_WINO, kw)


def test_no_g8_instantiation_reports_g16(emu):
    wt.check_no_g8_instantiation()


def test_auto_selection_table(emu, monkeypatch):
    monkeypatch.delenv("CFUN_TILE_GEOM", raising=False)
    wt.check_auto_table()
