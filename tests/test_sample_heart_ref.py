"""CPU tier, no kernel launched: tests/sample_heart_ref.py (the numpy restatement cfun_sample_heart is held to) against what pins
the rule of include/cfun_sample_heart.h.

scikit-image is not installed; oracle.cfun_oracle.skimage_resize is scipy.ndimage.zoom(mode='grid-constant', grid_mode=True) plus
the clip, the code path skimage.transform.resize takes for these inputs.  Pinned:
  * the image before the z-score equals skimage_resize(src, out, 1), the reference's cast back (``astype(int16)``: toward zero)
    or none, the float32 cast, then tests/sample_ref.py's rotation and re-layout -- the chain the reference runs -- BIT FOR BIT,
    on six shape pairs (up- and down-sampling per axis, extents of 1), with and without the cast, at four angles;
  * labels and boxes equal skimage_resize(mask, out, 0) pushed through sample_ref.rotate_and_box exactly;
  * hand answers."""
import numpy as np
import pytest

import sample_heart_ref as hr
import sample_ref as sr
from oracle import cfun_oracle as orc

# (source, output) as (H, W, D): up on every axis, down on every axis, mixed, equal, an output extent of 1, a source extent of 1
PAIRS = [((9, 12, 7), (14, 17, 11)), ((31, 29, 13), (20, 18, 8)), ((20, 14, 7), (14, 20, 12)), ((16, 16, 6), (16, 16, 6)),
         ((7, 9, 5), (10, 1, 1)), ((1, 8, 1), (6, 11, 4))]
ANGLES = [None, 0, 13, -20]
_ids = lambda t: "-".join("x".join(map(str, s)) for s in t)


def _hu(shape, seed=0):
    return np.random.default_rng(seed).integers(-1024, 3000, shape).astype(np.int16)


def _mask(shape, seed=0):
    rng = np.random.default_rng(seed)
    m = np.zeros(shape, np.int16)
    lo = [n // 5 for n in shape]
    m[lo[0]:, lo[1]:, lo[2]:] = rng.integers(0, 3, [n - l for n, l in zip(shape, lo)])
    return m


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


@pytest.mark.parametrize("pair", PAIRS, ids=_ids)
@pytest.mark.parametrize("truncate", [True, False], ids=["cast_back", "float"])
def test_image_equals_resize_cast_rotate_bit_for_bit(pair, truncate):
    shape, out = pair
    src = _hu(shape, sum(shape))
    resized = orc.skimage_resize(src, out, 1)
    assert resized.dtype == np.float64
    stored = resized.astype(np.int16) if truncate else resized                # utils.py:392 for an int16 loader dtype, or no cast
    if truncate:
        assert tuple(out) == tuple(shape) or resized.size < 20 or (stored != np.round(resized)).any(), \
            "test setup: truncation indistinguishable from rounding"
    for angle in ANGLES:
        want = np.ascontiguousarray(sr.rotate_slices(stored.astype(np.float32), angle).transpose(2, 0, 1))
        got = hr.sample_heart(src, None, out, angle, truncate=truncate)[0]
        assert got.dtype == np.float32 and got.shape == (out[2], out[0], out[1])
        assert np.array_equal(_bits(got), _bits(want)), "angle %r: %d of %d differ" % (angle, int((got != want).sum()), got.size)
    some = sorted({0, out[2] - 1, out[2] // 2})
    assert np.array_equal(_bits(hr.sample_heart(src, None, out, 13, truncate=truncate, planes=some)[0]),
                          _bits(hr.sample_heart(src, None, out, 13, truncate=truncate)[0][some]))


@pytest.mark.parametrize("pair", PAIRS, ids=_ids)
def test_the_clip_acts_on_an_all_positive_source(pair):
    shape, out = pair
    src = np.random.default_rng(1).integers(500, 900, shape).astype(np.int16)
    want = orc.skimage_resize(src, out, 1).astype(np.int16).astype(np.float32).transpose(2, 0, 1)
    got = hr.sample_heart(src, None, out, None, truncate=True)[0]
    assert np.array_equal(_bits(got), _bits(np.ascontiguousarray(want)))
    plain = hr.sample_heart(src, None, out, None, clip=None, truncate=True)[0]
    if (plain < src.min()).any():                                             # a face blended with the zero outside: the clip acts
        assert got.min() == src.min() and not np.array_equal(got, plain)
    if pair == PAIRS[0]:
        assert (plain < src.min()).any(), "test setup: the clip acts on no pair"


@pytest.mark.parametrize("pair", PAIRS, ids=_ids)
def test_labels_and_boxes_equal_the_order_0_resize_rotated(pair):
    shape, out = pair
    mask = _mask(shape, 3)
    resized = orc.skimage_resize(mask, out, 0)
    for angle in ANGLES:
        _, r_lab, r_raw, r_box, r_empty = sr.rotate_and_box(np.zeros(out, np.float32), resized, angle)
        _, lab, raw, box, empty = hr.sample_heart(_hu(shape), mask, out, angle)
        assert lab.dtype == np.uint8 and np.array_equal(lab, r_lab), angle
        assert raw.tolist() == r_raw.tolist() and box.tolist() == r_box.tolist() and empty == r_empty, angle


def test_label_low_bits_are_stored_and_the_value_read_is_boxed():
    mask = np.zeros((6, 6, 4), np.int16)
    mask[1, 1, 1], mask[4, 4, 2], mask[2, 3, 0] = 256, 3, -1                  # stored 0 yet counted; plain; stored 255, left out
    _, lab, raw, _, empty = hr.sample_heart(_hu((6, 6, 4)), mask, (6, 6, 4), None)
    assert lab[1, 1, 1] == 0 and lab[2, 4, 4] == 3 and lab[0, 2, 3] == 255
    assert raw.tolist() == [1, 1, 1, 3, 5, 5] and empty == 0


# -------------------------------------------------------------------------------------------------------------- hand answers
def test_equal_extents_at_angle_0_are_the_identity_re_laid():
    src = _hu((6, 5, 4), 5)
    for angle in (None, 0):
        got = hr.sample_heart(src, src.astype(np.int16) & 3, src.shape, angle, truncate=True)
        assert np.array_equal(got[0], src.astype(np.float32).transpose(2, 0, 1))
        assert np.array_equal(got[1], (src & 3).astype(np.uint8).transpose(2, 0, 1))


def test_one_axis_doubled_gives_three_quarter_blends():
    src = np.array([8.0, 16.0, 40.0]).reshape(3, 1, 1)
    got = hr.sample_heart(src, None, (6, 1, 1), None, clip=None)[0][0, :, 0]
    # c = (r + 0.5) / 2 - 0.5: -0.25 0.25 0.75 1.25 1.75 2.25 -> the faces blend with the zero outside
    assert got.tolist() == [0.75 * 8, 0.75 * 8 + 0.25 * 16, 0.25 * 8 + 0.75 * 16, 0.75 * 16 + 0.25 * 40, 0.25 * 16 + 0.75 * 40, 0.75 * 40]
    assert hr.sample_heart(src, None, (6, 1, 1), None)[0][0, :, 0].tolist()[::5] == [8.0, 30.0]      # the clip to [8, 40]: 6 -> 8


def test_half_weight_zero_border_at_a_face():
    src = np.full((4, 1, 1), 100.0)
    got = hr.sample_heart(src, None, (16, 1, 1), None, clip=None)[0][0, :, 0]      # c = -0.375 ...: the first tap lies outside
    assert got[0] == 100.0 * 0.625 and got[-1] == 100.0 * 0.625 and got[2] == 100.0
    src = np.full((1, 1, 1), 100.0)
    assert hr.sample_heart(src, None, (2, 1, 1), None, clip=None)[0][0, :, 0].tolist() == [75.0, 75.0]
    assert hr.sample_heart(src, None, (2, 1, 1), None)[0][0, :, 0].tolist() == [100.0, 100.0]


def test_truncation_is_toward_zero():
    for pair, blends in (((-2.0, 4.0), [-1.5, -0.5, 2.5, 3.0]), ((2.0, -4.0), [1.5, 0.5, -2.5, -3.0])):
        src = np.array(pair).reshape(2, 1, 1)
        assert hr.sample_heart(src, None, (4, 1, 1), None, clip=None)[0][0, :, 0].tolist() == blends
        got = hr.sample_heart(src, None, (4, 1, 1), None, clip=None, truncate=True)[0][0, :, 0]
        assert got.tolist() == [float(int(b)) for b in blends]                # -1.5 -> -1, -0.5 -> 0, 0.5 -> 0, 2.5 -> 2
        assert got.tolist() == np.array(blends).astype(np.int16).tolist()     # the reference's astype


def test_a_nan_source_spreads_and_survives_clip_and_cast():
    src = np.random.default_rng(6).normal(0.0, 200.0, (6, 6, 4)).astype(np.float32)
    src[2, 3, 1] = np.nan
    got = hr.sample_heart(src, None, (9, 9, 6), 13, clip=(-50.0, 50.0), truncate=True)[0]
    assert 1 < np.isnan(got).sum() < got.size // 2
    fin = got[~np.isnan(got)]
    assert fin.min() >= -50 and fin.max() <= 50 and np.array_equal(fin, np.trunc(fin))
    # a tap of weight 0 is still multiplied: at equal extents the NaN reaches its high-side neighbours
    same = hr.sample_heart(src, None, src.shape, None, clip=None)[0].transpose(1, 2, 0)
    assert np.isnan(same[1, 3, 1]) and np.isnan(same[2, 2, 1]) and np.isnan(same[2, 3, 0]) and not np.isnan(same[3, 3, 1])


def test_an_all_zero_volume_z_scores_to_nan():
    s = hr.sample_heart(np.zeros((5, 4, 3), np.int16), None, (7, 6, 5), 13, truncate=True)[0]
    assert not s.any()
    stats, z64, z32 = hr.zscore(s)
    assert stats[0] == 0 and stats[1] == 0 and np.isnan(z64).all() and np.isnan(z32).all()
    stats, z64, _ = hr.zscore(np.array([1.0, 3.0], np.float32))
    assert stats.tolist() == [2.0, 1.0] and z64.tolist() == [-1.0, 1.0]
