"""CPU tier, no kernel launched: tests/sample_ref.py (the numpy restatement the sample kernels are held to) against the
reference's recorded outputs (tests/golden/sample_targets.npz: extract_bboxes, the 5 % tail, load_image_gt and build_rpn_targets
of the main tree and the LiTS fork), the rotation's known answers, and scipy's nearest affine transform.

What the goldens pin and what they do not: everything behind the rotation is the reference's own output; the rotation itself ran
through a stub augmenter that applies sample_ref's rule (imgaug is not installed), so its parity with imgaug is unpinned."""
import numpy as np
import pytest

import sample_ref as sr
from conftest import load_golden


@pytest.fixture(scope="module")
def g():
    return load_golden("sample_targets")


ulp32_close = sr.ulp32_close


@pytest.mark.parametrize("tag", ["obj", "faces", "plane"])
def test_boxes_equal_the_reference(g, tag):
    lab = g["box_%s_mask" % tag].transpose(2, 0, 1)
    raw, empty = sr.extract_box(lab)
    assert empty == 0 and np.array_equal(raw, g["box_%s_raw" % tag])
    assert np.array_equal(sr.expand_box(raw, lab.shape), g["box_%s_lits" % tag])
    if tag == "plane":
        assert not raw.any()                     # the reference's one-plane quirk
    if tag == "faces":
        assert np.array_equal(sr.expand_box(raw, lab.shape), [0, 0, 0] + list(lab.shape))     # the expansion clamps


def test_empty_label_raises_the_flag():
    raw, empty = sr.extract_box(np.zeros((3, 4, 5), np.uint8))
    assert empty == 1 and not raw.any() and not sr.expand_box(raw, (3, 4, 5)).any()


@pytest.mark.parametrize("tag", ["main13", "main0", "lits"])
def test_load_image_gt_equals_the_reference(g, tag):
    lits = tag == "lits"
    mask = g[tag + "_mask_in"].astype(np.int32)
    image = np.zeros(mask.shape, np.float32) if lits else g[tag + "_image_in"]
    angle = None if lits else float(g[tag + "_angle"])
    ncls, r = [int(v) for v in g[tag + "_cfg"]]
    a = g[tag + "_anchors"]
    s = sr.load_image_gt(image, mask, angle, ncls, a, r, g[tag + "_std"], sr.keys_from_drops(a.shape[0], g[tag + "_drops"]))
    assert np.array_equal(s["gt_boxes"], g[tag + "_bbox"]) and s["gt_boxes"].shape[0] == ncls - 1
    assert np.array_equal(s["rpn_match"][0], g[tag + "_rpn_match"])
    ulp32_close(s["rpn_bbox_t"][0], g[tag + "_rpn_bbox"])
    if not lits:
        assert np.array_equal(s["gt_class_ids"], g[tag + "_class_ids"])
        img = s["image_raw"].astype(np.float32)
        np.testing.assert_allclose(((img - img.mean()) / img.std())[None], g[tag + "_image"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("tag", ["bt875", "bt1001"])
def test_build_rpn_targets_equals_the_reference(g, tag):
    a, r = g[tag + "_anchors"], int(g[tag + "_r"])
    match, bbox, counts = sr.build_rpn_targets(a, g[tag + "_gt"], r, g[tag + "_std"],
                                               sr.keys_from_drops(a.shape[0], g[tag + "_drops"]))
    assert np.array_equal(match, g[tag + "_rpn_match"])
    ulp32_close(bbox.astype(np.float32), g[tag + "_rpn_bbox"])
    assert counts[0] == (match == 1).sum() == r // 2 and counts[1] == (match == -1).sum() == r - r // 2


# ------------------------------------------------------------------------------------------ the rotation's known answers
def _vol(h, w, d=3, seed=0):
    return np.random.default_rng(seed).normal(size=(h, w, d)).astype(np.float32)


@pytest.mark.parametrize("shape", [(10, 14), (16, 16), (7, 9)])
def test_angle_0_is_the_identity(shape):
    v = _vol(*shape)
    assert np.array_equal(sr.rotate_slices(v, 0.0), v) and np.array_equal(sr.rotate_slices(v, None), v)


@pytest.mark.parametrize("shape", [(10, 14), (16, 16), (7, 9)])
def test_180_is_the_double_flip(shape):
    v = _vol(*shape)
    assert np.array_equal(sr.rotate_slices(v, 180.0), v[::-1, ::-1])


@pytest.mark.parametrize("n", [8, 16])
def test_90_on_even_squares_is_the_transpose_flip(n):
    v = _vol(n, n)
    # +90: sx = (y - c) + c, sy = -(x - c) + c, so out[y, x] = in[n - 1 - x, y]; -90: out[y, x] = in[x, n - 1 - y]
    assert np.array_equal(sr.rotate_slices(v, 90.0), v[::-1].transpose(1, 0, 2))
    assert np.array_equal(sr.rotate_slices(v, -90.0), v[:, ::-1].transpose(1, 0, 2))


@pytest.mark.parametrize("shape", [(10, 14), (16, 16), (24, 20)])
@pytest.mark.parametrize("angle", [-20, -7, 7, 13, 20])
def test_rotation_against_scipy_affine_transform(shape, angle):
    """scipy.ndimage.affine_transform(order=0, mode='constant') with the same matrix about the same centre.  Compared where the
    source coordinate lies in [0, n-1] on both axes (scipy's own boundary handling differs outside) and at least 1e-6 from a
    half-integer (the two round ties differently); no mismatch is allowed there, and that region must hold >= 75 % of the voxels."""
    from scipy import ndimage
    h, w = shape
    v = np.random.default_rng(3).normal(size=(h, w)).astype(np.float64)
    c, s = sr.cos_sin(angle)
    cy, cx = h / 2 - 0.5, w / 2 - 0.5
    m = np.array([[c, -s], [s, c]])                    # (sy, sx) = m @ (y - cy, x - cx) + (cy, cx)
    ref = ndimage.affine_transform(v, m, offset=np.array([cy, cx]) - m @ np.array([cy, cx]), order=0, mode="constant", cval=0.0)
    got = sr.rotate_slices(v[..., None], float(angle))[..., 0]
    sy, sx = sr.source_coords(h, w, float(angle))
    frac = lambda t: np.abs(t - np.floor(t) - 0.5)
    ok = (sy >= 0) & (sy <= h - 1) & (sx >= 0) & (sx <= w - 1) & (frac(sy) >= 1e-6) & (frac(sx) >= 1e-6)
    assert ok.mean() >= 0.75, "only %.1f %% of the voxels are comparable" % (100 * ok.mean())
    assert np.array_equal(got[ok], ref[ok]), "%d mismatches" % int((got[ok] != ref[ok]).sum())


def test_sample_module_has_no_host_read_back_and_no_raw_pointer():
    """cfun_amd/sample.py keeps box, tiling and counts on the device (only ``strict`` converts a flag), and its pointers go
    through _lib.ptr / ops.ptr_raw (the guard tier counts raw pointer uses per module, comments included)."""
    import os
    from conftest import ROOT
    src = open(os.path.join(ROOT, "cfun_amd", "sample.py")).read()
    for banned in (".item(", ".cpu(", "nonzero(", ".numpy(", ".tolist(", ".data_ptr("):
        assert banned not in src, banned
