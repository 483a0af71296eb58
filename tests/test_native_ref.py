"""CPU tier, no kernel launched: tests/native_ref.py (the numpy restatement cfun_mold_native and cfun_map_resize are held to)
against what pins the rule of include/cfun_native.h.

scikit-image is not installed; oracle.cfun_oracle.skimage_resize is scipy.ndimage.zoom(mode='grid-constant', grid_mode=True) plus
the clip, the code path skimage.transform.resize takes for these inputs.  Pinned:
  * steps 3-5 equal skimage_resize(src, R, 1) BIT FOR BIT in float64, before the float32 cast, on six shape pairs (up- and
    down-sampling per axis, equal extents, extents down to 2) and on an all-positive source, where the clip acts;
  * the whole rule equals that resize cast to float32 and pushed through sample_lits_ref.frame_rotate_resize without a map
    (cfun_sample_lits.h's rule: the frame, the nearest resize, the normalisation) -- the claim of the feature -- bit for bit;
  * hand answers; the byte rule equals skimage_resize(map, shape, 0) exactly."""
import numpy as np
import pytest

import native_ref as nr
import sample_lits_ref as lr
from oracle import cfun_oracle as orc

PAIRS = [((9, 12, 17), (11, 10, 40)), ((31, 29, 13), (27, 35, 29)), ((20, 20, 7), (20, 24, 23)), ((64, 64, 20), (57, 57, 66)),
         ((7, 5, 3), (3, 2, 2)), ((40, 40, 30), (40, 40, 30))]
_ids = lambda t: "-".join("x".join(map(str, s)) for s in t)


def _hu(shape, seed=0):
    return np.random.default_rng(seed).integers(-1024, 3000, shape).astype(np.int16)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


@pytest.mark.parametrize("pair", PAIRS, ids=_ids)
def test_resample_equals_zoom_bit_for_bit_in_float64(pair):
    shape, resampled = pair
    src = _hu(shape, sum(shape))
    want = orc.skimage_resize(src, resampled, 1)
    got = nr.resample(src, resampled, (src.min(), src.max()))
    assert want.dtype == got.dtype == np.float64 and got.shape == tuple(resampled)
    assert np.array_equal(_bits(got), _bits(want)), "%d of %d differ" % (int((got != want).sum()), got.size)


@pytest.mark.parametrize("pair", PAIRS[:4], ids=_ids)
def test_the_clip_acts_on_an_all_positive_source(pair):
    """grid-constant blends the faces with the zero outside: below the source's minimum when every voxel is positive."""
    import scipy.ndimage as ndi
    shape, resampled = pair
    src = np.random.default_rng(1).integers(500, 900, shape).astype(np.int16)
    raw = ndi.zoom(src.astype(np.float64), [r / float(n) for r, n in zip(resampled, shape)], order=1, mode="grid-constant", cval=0.0,
                   grid_mode=True)
    want = orc.skimage_resize(src, resampled, 1)
    assert (raw < src.min()).any() and want.min() == src.min(), "test setup: the oracle's clip does not act"
    assert np.array_equal(_bits(nr.resample(src, resampled, (src.min(), src.max()))), _bits(want))
    assert np.array_equal(_bits(nr.resample(src, resampled, None)), _bits(raw))          # ... and without it, zoom itself


# source (H,W,D), resampled, frame, output: both parities of P - R, R filling the frame on an axis, a few voxels inside it
QUADS = [((9, 12, 17), (11, 10, 40), (14, 13, 45), (9, 8, 20)),
         ((31, 29, 13), (27, 35, 29), (30, 35, 40), (33, 20, 17)),
         ((20, 20, 7), (20, 24, 23), (20, 24, 23), (16, 16, 8)),
         ((7, 5, 3), (3, 2, 2), (12, 11, 9), (10, 12, 7))]


@pytest.mark.parametrize("quad", QUADS, ids=_ids)
@pytest.mark.parametrize("kind", ["int16", "float32", "positive"])
def test_composition_identity(quad, kind):
    """native(src) == the fork's two steps: resize(order=1).astype(float32), then frame / nearest resize / normalise."""
    shape, resampled, frame, out = quad
    if kind == "int16":
        src = _hu(shape, 2)
    elif kind == "float32":
        src = np.random.default_rng(3).normal(0.0, 400.0, shape).astype(np.float32)
    else:
        src = np.random.default_rng(4).integers(100, 260, shape).astype(np.int16)      # inside the HU window: the clip shows
    stored = orc.skimage_resize(src, resampled, 1).astype(np.float32)                  # preprocessing.py:29-31
    want = lr.frame_rotate_resize(stored, np.zeros(resampled, np.uint8), frame, out, angle=None)[0]
    got = nr.mold_native(src, resampled, frame, out)
    assert got.dtype == np.float32 and got.shape == (out[2], out[0], out[1])
    assert np.array_equal(_bits(got), _bits(want)), "%d of %d differ" % (int((got != want).sum()), got.size)
    assert got.std() > 0.01
    some = [0, out[2] - 1, out[2] // 2]
    assert np.array_equal(_bits(nr.mold_native(src, resampled, frame, out, planes=some)), _bits(got[some]))


# -------------------------------------------------------------------------------------------------------------- hand answers
def test_equal_extents_copy_the_voxel():
    src = _hu((6, 5, 4), 5)
    assert np.array_equal(nr.resample(src, src.shape), src.astype(np.float64))
    got = nr.mold_native(src, src.shape, src.shape, src.shape, clip=None, norm=False)
    assert np.array_equal(got, src.astype(np.float32).transpose(2, 0, 1))


def test_one_axis_doubled_gives_three_quarter_blends():
    src = np.array([8.0, 16.0, 40.0]).reshape(3, 1, 1)
    got = nr.resample(src, (6, 1, 1))[:, 0, 0]
    # c = (r + 0.5) / 2 - 0.5: -0.25 0.25 0.75 1.25 1.75 2.25 -> the faces blend with the zero outside
    assert got.tolist() == [0.75 * 8, 0.75 * 8 + 0.25 * 16, 0.25 * 8 + 0.75 * 16, 0.75 * 16 + 0.25 * 40, 0.25 * 16 + 0.75 * 40, 0.75 * 40]


def test_half_weight_zero_border_at_a_face():
    src = np.full((4, 1, 1), 100.0)
    got = nr.resample(src, (2, 1, 1))[:, 0, 0]            # c = 0.5, 2.5: inside
    assert got.tolist() == [100.0, 100.0]
    got = nr.resample(src, (16, 1, 1))[:, 0, 0]           # c = -0.375 ...: the first tap lies outside
    assert got[0] == 100.0 * 0.625 and got[-1] == 100.0 * 0.625 and got[2] == 100.0
    src = np.full((1, 1, 1), 100.0)
    assert nr.resample(src, (2, 1, 1))[:, 0, 0].tolist() == [75.0, 75.0]      # c = -0.25, 0.25: three quarters of the only voxel
    assert nr.resample(src, (2, 1, 1), (100.0, 100.0))[:, 0, 0].tolist() == [100.0, 100.0]


def test_a_resampled_extent_of_one():
    src = np.arange(24, dtype=np.float64).reshape(4, 3, 2)
    got = nr.resample(src, (1, 3, 2))                     # c = 0.5 * 4 - 0.5 = 1.5: the mean of rows 1 and 2
    assert np.array_equal(got[0], 0.5 * src[1] + 0.5 * src[2])
    got = nr.resample(src, (1, 1, 1))                     # c = 1.5, 1.0, 0.5
    assert got[0, 0, 0] == 0.25 * (src[1, 1, 0] + src[1, 1, 1] + src[2, 1, 0] + src[2, 1, 1])


def test_a_source_extent_of_one():
    src = np.arange(12, dtype=np.float64).reshape(4, 3, 1) + 1
    got = nr.resample(src, (4, 3, 1))
    assert np.array_equal(got, src)
    got = nr.resample(src, (4, 3, 4))                     # c = -0.375 -0.125 0.125 0.375: weights 0.625 0.875 0.875 0.625
    assert np.array_equal(got, src * np.array([0.625, 0.875, 0.875, 0.625]))
    assert np.array_equal(_bits(nr.resample(src, (4, 3, 4), (src.min(), src.max()))), _bits(orc.skimage_resize(src, (4, 3, 4), 1)))


def test_the_frame_zero_is_not_normalised_and_hu_zero_is_a_half():
    src = np.zeros((2, 2, 1), np.int16)
    got = nr.mold_native(src, (2, 2, 1), (4, 4, 1), (4, 4, 1))
    assert got[0, 1:3, 1:3].tolist() == [[0.5, 0.5], [0.5, 0.5]] and got.sum() == 2.0


def test_non_finite_sources_spread_and_a_nan_survives_the_clip():
    src = np.random.default_rng(6).normal(0.0, 200.0, (6, 6, 4)).astype(np.float32)
    src[2, 3, 1], src[4, 1, 2] = np.nan, np.inf
    got = nr.resample(src, (9, 9, 6))
    assert np.isnan(got).sum() > 1 and np.isinf(got).sum() > 1
    assert np.array_equal(np.isnan(nr.clip_range(got, (-5.0, 5.0))), np.isnan(got))
    # a tap of weight 0 is still multiplied: equal extents, the NaN's high-side neighbour blends 1.0 * v + 0.0 * NaN
    same = nr.resample(src, src.shape)
    assert np.isnan(same[1, 3, 1]) and np.isnan(same[2, 2, 1]) and np.isnan(same[2, 3, 0]) and not np.isnan(same[3, 3, 1])


# ------------------------------------------------------------------------------------------------------------- the byte rule
@pytest.mark.parametrize("pair", [((9, 12, 17), (11, 10, 40)), ((31, 29, 13), (27, 35, 29)), ((20, 20, 7), (20, 24, 23)),
                                  ((7, 5, 3), (3, 2, 2)), ((5, 1, 4), (1, 3, 1)), ((6, 6, 6), (6, 6, 6))], ids=_ids)
def test_map_resize_equals_the_order_0_resize(pair):
    shape, out = pair
    src = np.random.default_rng(7).integers(0, 256, shape).astype(np.uint8)
    got = nr.map_resize(src, out)
    assert got.dtype == np.uint8 and np.array_equal(got, orc.skimage_resize(src, out, 0))
