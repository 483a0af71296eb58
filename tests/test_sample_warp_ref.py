"""CPU tier, no kernel launched: tests/sample_warp_ref.py (the numpy restatement cfun_sample_warp is held to) against what pins
the rule of include/cfun_sample_warp.h.

  * scipy.ndimage.map_coordinates on the restatement's OWN coordinate stack: labels and the order-0 image exactly wherever every
    coordinate lies in [0, n - 1] and at least 1e-6 from a half-integer (scipy rounds half to even and treats the border its own
    way: those voxels are left out, and at least half of all voxels must remain); the order-1 image against
    mode='grid-constant' on the float64 source over EVERY voxel within 2^-23 max|src|, one float32 rounding.
  * hand answers for every step.
NOT pinned: imgaug's Affine and PiecewiseAffine (not available to this project's environments); the trilinear control grid is
this project's own rule."""
import numpy as np
import pytest
from scipy import ndimage

import sample_ref as sr
import sample_warp_ref as wr
from cfun_amd import sample

# shape (D, H, W), grid, sigma, angle, flips (z, y, x)
SCIPY_CASES = [((9, 12, 17), (3, 3, 4), 1.5, 13, (False, True, False)),
               ((16, 20, 24), (4, 5, 5), 2.5, -20, (True, False, True)),
               ((5, 33, 31), (2, 6, 6), 3.0, 7, (False, False, False))]


def _volume(shape, seed):
    rng = np.random.default_rng(seed)
    img = rng.normal(100.0, 350.0, shape).astype(np.float32)
    lab = rng.integers(0, 3, shape).astype(np.uint8)
    return img, lab


@pytest.mark.parametrize("shape,g,sigma,angle,flips", SCIPY_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_against_scipy_map_coordinates(shape, g, sigma, angle, flips):
    img, lab = _volume(shape, 3)
    grid = np.random.default_rng(4).normal(0.0, sigma, (3,) + g).astype(np.float32)
    amap = sample.rotation_map(angle, shape[1], shape[2])
    s = wr.coords(shape, grid, amap, flips)
    n = np.array(shape, np.float64)[:, None, None, None]
    frac = np.abs(s - np.floor(s) - 0.5)
    exact = ((s >= 0.0) & (s <= n - 1.0) & (frac >= 1e-6)).all(axis=0)
    share = exact.mean()
    for order in (0, 1):
        r_img, r_lab, _, _, _ = wr.warp(img, lab, grid, amap, flips, order)
        want_lab = ndimage.map_coordinates(lab, s, order=0, mode="constant")
        bad = int((r_lab != want_lab)[exact].sum())
        changed = float((r_lab != lab).mean())
        print("%s order %d: %.0f %% of the voxels compared exactly, %d label mismatches, %.0f %% of the labels changed"
              % (shape, order, 100 * share, bad, 100 * changed))
        assert share >= 0.5, "fewer than half of the voxels take part in the exact comparison"
        assert bad == 0
        assert 0.1 <= changed <= 0.9, "test setup: the warp does not act on the labels"
        if order == 0:
            want = ndimage.map_coordinates(img, s, order=0, mode="constant")
            assert np.array_equal(r_img[exact].view(np.int32), want[exact].view(np.int32))
        else:
            want = ndimage.map_coordinates(img.astype(np.float64), s, order=1, mode="grid-constant")
            err = float(np.abs(r_img.astype(np.float64) - want).max())
            bound = 2.0 ** -23 * float(np.abs(img).max())
            print("%s: largest order-1 error %.3e (bound %.3e)" % (shape, err, bound))
            assert err <= bound


def test_planes_are_the_whole_volumes_planes():
    img, lab = _volume((7, 9, 11), 5)
    grid = np.random.default_rng(6).normal(0.0, 1.0, (3, 3, 3, 3)).astype(np.float32)
    amap = sample.affine_map(13, 9, 11, scale=(1.1, 0.9), translate=(1, -2))
    whole = wr.warp(img, lab, grid, amap, (True, False, True), 1)
    some = wr.warp(img, lab, grid, amap, (True, False, True), 1, planes=[0, 3, 6])
    assert np.array_equal(some[0].view(np.int32), whole[0][[0, 3, 6]].view(np.int32)) and np.array_equal(some[1], whole[1][[0, 3, 6]])


# ------------------------------------------------------------------------------------------------------------ hand answers
def _ints(shape):
    img = (np.arange(np.prod(shape), dtype=np.float32).reshape(shape) % 97) + 1.0
    lab = (np.arange(np.prod(shape)).reshape(shape) % 3 + 1).astype(np.uint8)
    return img, lab


def test_identity():
    img, lab = _ints((4, 5, 6))
    for order in (0, 1):
        got = wr.warp(img, lab, image_order=order)
        assert np.array_equal(got[0], img) and np.array_equal(got[1], lab)
        assert got[2].tolist() == [0, 0, 0, 4, 5, 6] and got[3].tolist() == [0, 0, 0, 4, 5, 6] and got[4] == 0
    zero = np.zeros((3, 2, 2, 2), np.float32)
    assert np.array_equal(wr.warp(img, lab, zero, sample.rotation_map(0, 5, 6), image_order=1)[0], img)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_single_flip(axis):
    img, lab = _ints((4, 5, 6))
    flips = tuple(a == axis for a in range(3))
    for order in (0, 1):
        got = wr.warp(img, lab, flips=flips, image_order=order)
        assert np.array_equal(got[0], np.flip(img, axis)) and np.array_equal(got[1], np.flip(lab, axis))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_constant_grid_of_one_is_a_shift_with_a_zero_face(axis):
    img, lab = _ints((4, 5, 6))
    grid = np.zeros((3, 2, 3, 2), np.float32)
    grid[axis] = 1.0
    want_i, want_l = np.zeros_like(img), np.zeros_like(lab)
    dst = [slice(None)] * 3
    src = [slice(None)] * 3
    dst[axis], src[axis] = slice(0, -1), slice(1, None)
    want_i[tuple(dst)], want_l[tuple(dst)] = img[tuple(src)], lab[tuple(src)]
    for order in (0, 1):
        got = wr.warp(img, lab, grid, image_order=order)
        assert np.array_equal(got[0], want_i) and np.array_equal(got[1], want_l)
    assert got[2].tolist()[3 + axis] == img.shape[axis] - 1                 # the box lost the zero face


def test_constant_grid_of_a_half_under_order_one():
    img, lab = _ints((2, 3, 5))
    grid = np.zeros((3, 2, 2, 2), np.float32)
    grid[2] = 0.5
    got = wr.warp(img, lab, grid, image_order=1)
    want = np.zeros_like(img)
    want[..., :-1] = 0.5 * img[..., :-1] + 0.5 * img[..., 1:]               # the two-voxel average
    want[..., -1] = 0.5 * img[..., -1]                                       # the half-weight border: the far tap lies outside
    assert np.array_equal(got[0], want)
    shifted = np.zeros_like(lab)
    shifted[..., :-1] = lab[..., 1:]                                         # x + 0.5 rounds half away from zero: x + 1
    assert np.array_equal(got[1], shifted)


def test_linear_stretch_of_one_row():
    """A 2^3 grid whose far x face is +2 along x on W = 5: d_x = 2 * x / 4, p_x = 0, 1.5, 3, 4.5, 6."""
    img = np.array([10.0, 20.0, 40.0, 80.0, 160.0], np.float32).reshape(1, 1, 5)
    lab = np.array([1, 2, 3, 4, 5], np.uint8).reshape(1, 1, 5)
    grid = np.zeros((3, 2, 2, 2), np.float32)
    grid[2, :, :, 1] = 2.0
    assert wr.coords((1, 1, 5), grid)[2, 0, 0].tolist() == [0.0, 1.5, 3.0, 4.5, 6.0]
    got = wr.warp(img, lab, grid, image_order=1)
    assert got[0].reshape(-1).tolist() == [10.0, 30.0, 80.0, 80.0, 0.0]      # 4.5: half of 160, the far tap outside; 6: outside
    assert got[1].reshape(-1).tolist() == [1, 3, 4, 0, 0]                    # 1.5 -> 2, 4.5 -> 5: outside
    assert wr.warp(img, lab, grid, image_order=0)[0].reshape(-1).tolist() == [10.0, 40.0, 80.0, 0.0, 0.0]


def test_nan_source_voxel_behind_a_zero_weight():
    img, lab = _ints((4, 5, 6))
    img[2, 2, 3] = np.nan
    got = wr.warp(img, lab, image_order=1)[0]                                # identity: every far tap has the weight 0
    nan = np.argwhere(np.isnan(got)).tolist()
    assert sorted(nan) == sorted([z, y, x] for z in (1, 2) for y in (1, 2) for x in (2, 3))
    ok = ~np.isnan(got)
    assert np.array_equal(got[ok], img[ok])
    got0 = wr.warp(img, lab, image_order=0)[0]
    assert int(np.isnan(got0).sum()) == 1


def test_nan_control_value_gives_zeros():
    img, lab = _ints((4, 5, 6))
    grid = np.zeros((3, 2, 2, 2), np.float32)
    grid[1, 1, 0, 1] = np.nan                                                # eight weights everywhere: 0 * NaN is a NaN
    for order in (0, 1):
        got = wr.warp(img, lab, grid, image_order=order)
        assert not got[0].any() and not np.isnan(got[0]).any() and not got[1].any()
        assert got[4] == 1 and not got[2].any() and not got[3].any()
    inf = np.zeros((3, 2, 2, 2), np.float32)
    inf[2] = np.inf
    got = wr.warp(img, lab, inf, image_order=1)
    assert not got[0].any() and not np.isnan(got[0]).any() and not got[1].any()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_extent_of_one(axis):
    """n_a == 1: u = 0, cell 0, weight 0 -- a displacement of 0.4 along that axis keeps the nearest voxel and weighs the
    order-1 value by 0.6; a shift along another axis still acts."""
    shape = tuple(1 if a == axis else 5 for a in range(3))
    img, lab = _ints(shape)
    i, t = wr.control(1, 4)
    assert i.tolist() == [0] and t.tolist() == [0.0]
    grid = np.zeros((3, 2, 2, 2), np.float32)
    grid[axis] = 0.4
    got = wr.warp(img, lab, grid, image_order=1)
    assert np.array_equal(got[0], ((1.0 - np.float64(np.float32(0.4))) * img.astype(np.float64)).astype(np.float32))
    assert np.array_equal(got[1], lab)
    other = (axis + 1) % 3
    grid = np.zeros((3, 2, 2, 2), np.float32)
    grid[other] = 1.0
    got = wr.warp(img, lab, grid, image_order=0)
    assert np.array_equal(np.take(got[0], range(4), other), np.take(img, range(1, 5), other))
    assert not np.take(got[0], [4], other).any()


def test_affine_map_equals_rotation_map():
    for angle in (0, 7, -13, 20, 45, 90, 180, 33.3):
        for h, w in ((9, 12), (320, 320), (17, 5)):
            assert sample.affine_map(angle, h, w) == sample.rotation_map(angle, h, w)
    m = sample.affine_map(0, 8, 10, scale=(2, 4), translate=(1, -3))
    assert m == (0.25, -0.0, 4.5 - 0.25 * (4.5 - 3), 0.0, 0.5, 3.5 - 0.5 * (3.5 + 1))
