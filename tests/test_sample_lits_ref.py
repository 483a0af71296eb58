"""CPU tier, no kernel launched: tests/sample_lits_ref.py (the numpy restatement cfun_sample_lits is held to) against what pins
the rule of include/cfun_sample_lits.h.

scikit-image is not installed, so nothing could be recorded from the fork's Dataset.__getitem__.  Pinned instead:
  * without a map, image and label equal oracle.cfun_oracle.skimage_resize(frame, out, 0) of the explicitly built frame exactly;
  * angle 0 is bit-identical to no map;
  * with a rotation, the result equals scipy.ndimage.affine_transform(order=0, mode='constant') of every slice of the explicit
    frame followed by that resize, wherever the source coordinate lies in [0, P-1] on both axes and at least 1e-6 from a
    half-integer; that region must hold >= 75 % of the output voxels.
Not pinned: exact half-voxel ties, and the last ulp between this operation order and scikit-image's matrix product."""
import numpy as np
import pytest

import sample_lits_ref as lr
from oracle import cfun_oracle as orc

# source / frame / output, each (H, W, D)
TRIPLES = [((21, 18, 9), (30, 26, 14), (16, 12, 6)),
           ((20, 20, 8), (24, 24, 10), (40, 40, 20)),            # an up-sampling
           ((33, 40, 70), (40, 44, 75), (20, 68, 66)),
           ((9, 7, 3), (9, 7, 3), (9, 7, 3))]                    # frame = source = output
_ids = lambda t: "-".join("x".join(map(str, s)) for s in t)


def _pair(shape, seed=0):
    rng = np.random.default_rng(seed)
    image = rng.normal(0.0, 250.0, shape).astype(np.float32)
    mask = rng.integers(0, 3, shape).astype(np.int8)
    return image, mask


def _resized_frames(image, mask, frame, out, rotate=None):
    """The reference's route on the host: explicit frames (the image normalised first), optional per-slice transform, resize."""
    fi, fm = lr.explicit_frame(lr.normalise(image), frame), lr.explicit_frame(mask.astype(np.uint8), frame)
    if rotate is not None:
        fi = np.stack([rotate(fi[:, :, k]) for k in range(frame[2])], axis=2)
        fm = np.stack([rotate(fm[:, :, k]) for k in range(frame[2])], axis=2)
    return (orc.skimage_resize(fi, out, 0).transpose(2, 0, 1), orc.skimage_resize(fm, out, 0).transpose(2, 0, 1))


@pytest.mark.parametrize("triple", TRIPLES, ids=_ids)
def test_no_map_equals_the_resized_explicit_frame(triple):
    shape, frame, out = triple
    image, mask = _pair(shape)
    img, lab, _, _, _ = lr.frame_rotate_resize(image, mask, frame, out, None)
    ri, rm = _resized_frames(image, mask, frame, out)
    assert img.dtype == np.float32 and lab.dtype == np.uint8 and img.shape == (out[2], out[0], out[1])
    assert np.array_equal(img, ri) and np.array_equal(lab, rm)
    assert lab.any() and img.std() > 0.05


@pytest.mark.parametrize("triple", TRIPLES, ids=_ids)
def test_angle_0_is_bit_identical_to_no_map(triple):
    shape, frame, out = triple
    image, mask = _pair(shape, 1)
    a = lr.frame_rotate_resize(image, mask, frame, out, None)
    b = lr.frame_rotate_resize(image, mask, frame, out, 0)
    assert all(np.array_equal(p, q) for p, q in zip(a[:4], b[:4])) and a[4] == b[4]


@pytest.mark.parametrize("triple", TRIPLES[:3], ids=_ids)        # (not the 9x7 frame: only 59 % of it is comparable at +-30)
@pytest.mark.parametrize("angle", [-30, -13, 7, 30])
def test_rotation_against_scipy_affine_transform(triple, angle):
    from scipy import ndimage
    shape, frame, out = triple
    image, mask = _pair(shape, 2)
    m = lr.rotation_map(angle, frame[0], frame[1])
    # scipy maps output (row, col) -> input (row, col): matrix rows are (m11 m10 | m12) and (m01 m00 | m02) in that order
    mat, offs = np.array([[m[4], m[3]], [m[1], m[0]]]), np.array([m[5], m[2]])
    rot = lambda s: ndimage.affine_transform(s, mat, offset=offs, order=0, mode="constant", cval=0.0)
    ri, rm = _resized_frames(image, mask, frame, out, rot)
    img, lab, _, _, _ = lr.frame_rotate_resize(image, mask, frame, out, angle)
    row, col = lr.frame_coords(frame, out, m)
    frac = lambda t: np.abs(t - np.floor(t) - 0.5)
    ok = (row >= 0) & (row <= frame[0] - 1) & (col >= 0) & (col <= frame[1] - 1) & (frac(row) >= 1e-6) & (frac(col) >= 1e-6)
    assert ok.mean() >= 0.75, "only %.1f %% of the voxels are comparable" % (100 * ok.mean())
    assert np.array_equal(img[:, ok], ri[:, ok]), "%d image mismatches" % int((img[:, ok] != ri[:, ok]).sum())
    assert np.array_equal(lab[:, ok], rm[:, ok]), "%d label mismatches" % int((lab[:, ok] != rm[:, ok]).sum())
    assert (img != lr.frame_rotate_resize(image, mask, frame, out, None)[0]).any()


# -------------------------------------------------------------------------------------------------------------- hand answers
@pytest.mark.parametrize("frame", [(10, 14, 3), (16, 16, 2), (7, 9, 1)])
def test_180_is_the_double_flip_of_the_frame(frame):
    shape = (frame[0] - 3, frame[1] - 2, frame[2])               # an off-centre source: the flip moves it
    image, mask = _pair(shape, 3)
    img, lab, _, _, _ = lr.frame_rotate_resize(image, mask, frame, frame, 180, norm=False)
    assert np.array_equal(img, lr.explicit_frame(image, frame)[::-1, ::-1].transpose(2, 0, 1))
    assert np.array_equal(lab, lr.explicit_frame(mask.astype(np.uint8), frame)[::-1, ::-1].transpose(2, 0, 1))


def test_a_source_that_fills_the_frame_is_the_identity():
    shape = (9, 7, 3)
    image, mask = _pair(shape, 4)
    img, lab, raw, box, empty = lr.frame_rotate_resize(image, mask, shape, shape, None, norm=False)
    assert np.array_equal(img, image.transpose(2, 0, 1)) and np.array_equal(lab, mask.astype(np.uint8).transpose(2, 0, 1))
    assert empty == 0


def test_an_odd_pad_difference_puts_the_extra_voxel_on_the_high_side():
    image = np.ones((4, 5, 2), np.float32)
    mask = np.ones((4, 5, 2), np.int8)
    frame = (7, 8, 5)                                            # P - n = 3 on every axis: 1 low, 2 high
    assert lr.offsets(frame, image.shape) == (1, 1, 1)
    img, lab, raw, _, _ = lr.frame_rotate_resize(image, mask, frame, frame, None, norm=False)
    assert raw.tolist() == [1, 1, 1, 3, 5, 6]                    # (z, y, x): rows 1 .. 4, columns 1 .. 5, planes 1 .. 2
    assert img.sum() == 40 and not img[0].any() and not img[:, 0].any() and not img[:, -2:].any() and not img[:, :, -2:].any()


def test_a_frame_corner_that_rotates_out_of_the_frame_is_zero():
    shape = (12, 12, 2)
    image = np.full(shape, 5.0, np.float32)
    mask = np.full(shape, 2, np.int8)
    img, lab, _, _, _ = lr.frame_rotate_resize(image, mask, shape, shape, 30, norm=False)
    for y, x in ((0, 0), (0, 11), (11, 0), (11, 11)):
        assert img[0, y, x] == 0 and lab[0, y, x] == 0
    assert img[0, 6, 6] == 5 and lab[0, 6, 6] == 2


def test_normalisation_hand_answers():
    got = lr.normalise(np.array([300, -300, 301, -301, 0, np.nan], np.float32))
    assert got[:5].tolist() == [0.0, 1.0, 0.0, 1.0, 0.5] and np.isnan(got[5])
    # the frame's zeros are not normalised: HU 0 inside the source is 0.5, the padding around it is 0
    img = lr.frame_rotate_resize(np.zeros((2, 2, 1), np.float32), np.ones((2, 2, 1), np.int8), (4, 4, 1), (4, 4, 1))[0]
    assert img[0, 1:3, 1:3].tolist() == [[0.5, 0.5], [0.5, 0.5]] and img.sum() == 2.0


def test_normalisation_equals_preprocess_image_lits():
    import torch
    from cfun_amd import utils
    hu = np.concatenate([np.arange(-1100, 1101, dtype=np.float32), np.random.default_rng(5).normal(0, 300, 4096).astype(np.float32)])
    assert np.array_equal(lr.normalise(hu), utils.preprocess_image_lits(torch.from_numpy(hu)).numpy())


def test_low_eight_bits_of_the_label():
    mask = np.array([[[0, 1, 255, 256, 257, -1]]], np.int32)
    lab = lr.frame_rotate_resize(np.zeros(mask.shape, np.float32), mask, mask.shape, mask.shape)[1]
    assert lab[:, 0, 0].tolist() == [0, 1, 255, 0, 1, 255]


@pytest.mark.parametrize("triple", TRIPLES[:3], ids=_ids)
def test_window_equals_the_oracles(triple):
    shape, frame, out = triple
    min_dim, max_dim = out[2], out[0]
    _, _, win = orc.mold_inputs_lits([np.zeros(shape, np.float32)], frame, list(out), min_dim, max_dim, 3)
    assert tuple(win[0]) == lr.window(frame, shape, out, min_dim, max_dim)
