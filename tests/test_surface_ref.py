"""CPU only: the restatement tests/surface_ref.py itself, against scipy's exact Euclidean distance transform and against answers
written by hand.  The device tiers (test_surface_emu.py, test_surface_gpu.py) are then held to the restatement bit for bit."""
import numpy as np
import pytest
from scipy import ndimage

import surface_cases as sc
import surface_ref as sr

# One rounding of a2, one of the product and two additions lie between the float32 field and the exact squared distance.
REL = (1.0 + 2.0 ** -24) ** 4 - 1.0


def _edt2(surf, spacing):
    return ndimage.distance_transform_edt(~surf, sampling=spacing) ** 2


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_field_against_scipy(shape):
    """Bernoulli maps at three densities.  Unit spacing: every term is an integer below 2^24, so the field is exact and equals
    the rounded square of scipy's distance.  Dyadic spacing (1.25, 0.78125, 0.78125): the squares are 1600 / 1024 and 625 / 1024,
    every term and every sum is a multiple of 2^-10, exact in float32 while it stays below 2^14 -- equality is required there and
    the relative bound beyond.  The two anisotropic spacings: the relative bound REL."""
    seen = 0
    worst = 0.0
    for p in (0.02, 0.3, 0.7):
        m = sc.bernoulli(shape, p, 3, 7 + shape[0] + shape[2])
        for cls in (1, 2):
            surf = sr.surface(m, cls)
            for spacing in sc.SPACINGS:
                f = sr.field(surf, spacing)
                assert f.dtype == np.float32 and f.shape == shape
                if not surf.any():
                    assert np.isinf(f).all()
                    continue
                seen += 1
                want = _edt2(surf, spacing)
                got = f.astype(np.float64)
                if spacing == sc.SPACINGS[0]:
                    assert np.array_equal(got, np.rint(want))
                elif spacing == sc.SPACINGS[1]:
                    exact = want < 2.0 ** 14 - 1.0
                    assert np.array_equal(f[exact], want[exact].astype(np.float32))
                    assert (np.abs(got - want) <= REL * want).all()
                else:
                    err = np.abs(got - want)
                    assert (err <= REL * want).all(), (spacing, float((err / np.maximum(want, 1e-300)).max()) / 2.0 ** -24)
                    worst = max(worst, float((err[want > 0] / want[want > 0]).max(initial=0.0)))
    assert seen or shape == (1, 1, 1)
    assert worst <= REL


def test_surface_is_the_erosion_formula_and_a_cube_has_26():
    m = np.zeros((7, 7, 7), np.uint8)
    m[2:5, 2:5, 2:5] = 1
    s = sr.surface(m, 1)
    assert int(s.sum()) == 26 and not s[3, 3, 3] and s[2:5, 2:5, 2:5].sum() == 26
    full = np.full((4, 5, 6), 3, np.uint8)
    assert int(sr.surface(full, 3).sum()) == 4 * 5 * 6 - 2 * 3 * 4          # a voxel on a face of the volume is surface
    assert not sr.surface(full, 1).any()
    two = np.array([[[1, 1, 2, 2]]], np.uint8)
    assert sr.surface(two, 1).tolist() == [[[True, True, False, False]]]


@pytest.mark.parametrize("spacing", sc.SPACINGS, ids=str)
def test_one_voxel_each(spacing):
    pred, label = np.zeros((4, 3, 9), np.uint8), np.zeros((4, 3, 9), np.uint8)
    pred[1, 2, 3] = 1
    label[3, 0, 7] = 1
    d = float(np.sqrt((2 * spacing[0]) ** 2 + (2 * spacing[1]) ** 2 + (4 * spacing[2]) ** 2))      # || delta o s ||
    row = sr.class_stats(pred, label, 1, spacing)
    assert (row["n_pred"], row["n_label"]) == (1, 1) and row["q_lo_sq"] == row["q_hi_sq"]      # n = 2: ranks 0 and 1, both d
    got = sr.scores(row)
    for name, v in got.items():
        assert abs(v - d) <= REL * d, (name, v, d)                      # (a root halves the relative error of the square)
    assert abs(row["np_percentile"] - d) <= REL * d


@pytest.mark.parametrize("spacing", sc.SPACINGS, ids=str)
def test_two_planes(spacing):
    """Two one-voxel-thick full planes four voxels apart along x: every voxel of either is surface, every distance is 4 sx."""
    pred, label = np.zeros((3, 4, 9), np.uint8), np.zeros((3, 4, 9), np.uint8)
    pred[:, :, 2] = 2
    label[:, :, 6] = 2
    row = sr.class_stats(pred, label, 2, spacing)
    d = 4.0 * spacing[2]
    assert (row["n_pred"], row["n_label"]) == (12, 12)
    assert (np.unique(row["d2_pl"]).size, np.unique(row["d2_lp"]).size) == (1, 1)
    for name, v in sr.scores(row).items():
        assert abs(v - d) <= REL * d, (name, v, d)
    assert sr.class_stats(pred, label, 1, spacing)["n_pred"] == 0


def test_cube_in_cube():
    """A 3^3 cube centred in a 5^3 cube, unit spacing.  A = 26 voxels, B = 125 - 27 = 98.  Every voxel of A has a coordinate on
    the small cube's face, one step from the large cube's face: every pred -> label distance is 1.  A voxel of B with m of its
    coordinates on the large cube's faces is nearest to the voxel of A it is clamped to, at sqrt(m): 6 x 9 face voxels at 1,
    12 x 3 edge voxels at sqrt(2), 8 corners at sqrt(3)."""
    pred, label = np.zeros((9, 8, 7), np.uint8), np.zeros((9, 8, 7), np.uint8)
    label[1:6, 1:6, 1:6] = 1
    pred[2:5, 2:5, 2:5] = 1
    row = sr.class_stats(pred, label, 1, (1.0, 1.0, 1.0), q=95.0)
    assert (row["n_pred"], row["n_label"]) == (26, 98)
    assert row["sum_pl"] == 26.0 and row["sumsq_pl"] == 26.0 and row["max_sq_pl"] == 1.0
    assert sorted(np.unique(row["d2_lp"], return_counts=True)[1].tolist()) == [8, 36, 54]
    assert row["sumsq_lp"] == 54.0 + 72.0 + 24.0 and row["max_sq_lp"] == 3.0
    assert abs(row["sum_lp"] - (54.0 + 36.0 * np.sqrt(2.0) + 8.0 * np.sqrt(3.0))) <= 98 * 2.0 ** -52 * row["sum_lp"]
    s = sr.scores(row)
    assert s["hausdorff"] == np.sqrt(3.0) and s["asd_pred_to_label"] == 1.0
    assert abs(s["rmsd"] - np.sqrt(176.0 / 124.0)) <= 4 * 2.0 ** -52 * s["rmsd"]
    # 124 values sorted: 80 ones, 36 roots of two, 8 roots of three; pos = 123 * 0.95 = 116.85 -> ranks 116 and 117 are both sqrt(3)
    assert (row["q_lo_sq"], row["q_hi_sq"]) == (3.0, 3.0) and s["hd_percentile"] == np.sqrt(3.0)


def test_class_on_one_side_only_is_nan():
    pred, label = np.zeros((3, 3, 5), np.uint8), np.zeros((3, 3, 5), np.uint8)
    pred[1, 1, 1] = 1
    label[1, 1, 3] = 2
    for c in (1, 2):
        row = sr.class_stats(pred, label, c, (1.0, 1.0, 1.0))
        assert row["n_pred"] + row["n_label"] == 1 and all(row[name] == 0.0 for name in sr.FIELDS[2:])
        assert all(np.isnan(v) for v in sr.scores(row).values())
    rows = sr.stats(pred, label, 3, (1.0, 1.0, 1.0))
    assert len(rows) == 3 and not any(rows[0][name] for name in sr.FIELDS)


def test_percentile_by_hand():
    """A = {x = 0}, B = {x = 1, 3, 6} on one row, unit spacing: the directed sets are {1} and {1, 3, 6}, sorted 1, 1, 3, 6.
    q = 50: pos = 3 * 0.5 = 1.5, ranks 1 and 2, frac 0.5: (1 + 3) / 2 = 2.  q = 95: pos = 2.85, ranks 2 and 3: 3 + 0.85 * 3."""
    pred, label = np.zeros((1, 1, 8), np.uint8), np.zeros((1, 1, 8), np.uint8)
    pred[0, 0, 0] = 1
    label[0, 0, [1, 3, 6]] = 1
    row = sr.class_stats(pred, label, 1, (1.0, 1.0, 1.0), q=50.0)
    assert (row["q_lo_sq"], row["q_hi_sq"], row["frac"]) == (1.0, 9.0, 0.5)
    assert sr.scores(row)["hd_percentile"] == 2.0 == row["np_percentile"]
    row = sr.class_stats(pred, label, 1, (1.0, 1.0, 1.0), q=95.0)
    assert (row["q_lo_sq"], row["q_hi_sq"]) == (9.0, 36.0) and row["frac"] != 0.0 and abs(row["frac"] - 0.85) < 1e-12
    assert abs(sr.scores(row)["hd_percentile"] - 5.55) < 1e-12 and abs(row["np_percentile"] - 5.55) < 1e-12
    assert sr.rank_rule(4, 0.0) == (0, 1, 0.0) and sr.rank_rule(4, 1.0) == (3, 3, 0.0) and sr.rank_rule(1, 0.95) == (0, 0, 0.0)


def test_percentile_rule_is_numpys():
    """The header's rule -- pos = (n - 1) * qf on exact order statistics -- against np.percentile of the concatenation.  numpy
    forms its index as n * qf + (1 - qf) - 1 and interpolates with another formula: the two indices differ by a few roundings
    of values up to n, so the results agree within 8 n 2^-53 of the gap between the two ranks plus a few ulps of the value."""
    for seed, shape, q in ((1, (9, 9, 65), 95.0), (2, (17, 10, 67), 37.5), (3, (3, 17, 130), 99.9)):
        pred, label = sc.bernoulli(shape, 0.3, 3, seed), sc.bernoulli(shape, 0.3, 3, seed + 10)
        row = sr.class_stats(pred, label, 1, sc.SPACINGS[3], q=q)
        n = row["n_pred"] + row["n_label"]
        lo, hi = np.sqrt(row["q_lo_sq"]), np.sqrt(row["q_hi_sq"])
        have = sr.scores(row)["hd_percentile"]
        assert abs(have - row["np_percentile"]) <= 8 * n * 2.0 ** -53 * (hi - lo) + 8 * 2.0 ** -53 * hi
