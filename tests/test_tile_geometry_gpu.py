"""GPU tier (real library, cuda:0) of the output-tile geometry: every case of tile_geometry_cases.py once as G16 and once as G8."""
import pytest

import tile_geometry_cases as tg
from cfun_amd._lib import ALGO_MFMA

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("name", sorted(tg.DIRECT_CASES))
def test_direct_conv_both_geometries(gpu, name):
    n, dhw, ci, co, kw = tg.DIRECT_CASES[name]
    tg.check_conv_both(gpu, n, dhw, ci, co, ALGO_MFMA, kw)


@pytest.mark.parametrize("name", sorted(tg.FOLD_CASES))
def test_folded_up_conv_both_geometries(gpu, name):
    tg.check_fold_both(gpu, *tg.FOLD_CASES[name])


@pytest.mark.parametrize("algo", sorted(tg.WINO_ALGOS))
@pytest.mark.parametrize("name", sorted(tg.WINO_CASES))
def test_winograd_conv_both_geometries(gpu, name, algo):
    n, dhw, ci, co, kw = tg.WINO_CASES[name]
    tg.check_conv_both(gpu, n, dhw, ci, co, tg.WINO_ALGOS[algo], kw)


def test_auto_selection_table(gpu, monkeypatch):
    monkeypatch.delenv("CFUN_TILE_GEOM", raising=False)
    tg.check_auto_table()
