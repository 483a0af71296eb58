"""tests/cc_ref.py against answers written by hand: the device tiers compare against that file, so it is checked on its own."""
import numpy as np

import cc_ref as cr


def _lin(shape, z, y, x):
    return (z * shape[1] + y) * shape[2] + x


def test_space_diagonal():
    n = 5
    v = np.zeros((n, n, n), np.uint8)
    for i in range(n):
        v[i, i, i] = 2
    lab26 = cr.label(v, 26, "class")
    assert lab26.dtype == np.int32 and lab26.sum() == n and (lab26[v > 0] == 1).all()       # one component, rooted at voxel 0
    lab6 = cr.label(v, 6, "class")
    assert [int(lab6[i, i, i]) for i in range(n)] == [_lin(v.shape, i, i, i) + 1 for i in range(n)]      # n components
    _, out, stats = cr.clean(v, 3, 6, "class", largest_only=True)
    assert out.sum() == 2 and out[0, 0, 0] == 2                      # n components of one voxel tie: the smallest label wins
    assert stats.tolist() == [[0, 0, 0], [0, 0, 0], [n, 1, n - 1]]
    _, out, stats = cr.clean(v, 3, 26, "class", largest_only=True)
    assert np.array_equal(out, v) and stats.tolist() == [[0, 0, 0], [0, 0, 0], [1, n, 0]]


def test_checkerboard():
    z, y, x = np.indices((4, 4, 4))
    v = ((z + y + x) % 2 == 0).astype(np.uint8)
    lab6 = cr.label(v, 6, "foreground")
    want = np.where(v > 0, np.arange(64).reshape(4, 4, 4) + 1, 0)
    assert np.array_equal(lab6, want)                                # 32 components of one voxel
    lab26 = cr.label(v, 26, "foreground")
    assert np.array_equal(lab26, v.astype(np.int32))                 # edge neighbours join them all: one component, label 1
    _, _, stats = cr.clean(v, 2, 6, "foreground", largest_only=False, min_voxels=2)
    assert stats.tolist() == [[32, 1, 32], [0, 0, 0]]


def test_cubes_touching_at_a_corner():
    v = np.zeros((4, 4, 4), np.uint8)
    v[0:2, 0:2, 0:2] = 1
    v[2:4, 2:4, 2:4] = 1
    lab6 = cr.label(v, 6, "class")
    assert set(np.unique(lab6)) == {0, 1, _lin(v.shape, 2, 2, 2) + 1}
    assert (lab6[0:2, 0:2, 0:2] == 1).all() and (lab6[2:4, 2:4, 2:4] == 43).all()
    assert np.array_equal(cr.label(v, 26, "class"), v.astype(np.int32))


def test_tie_goes_to_the_smaller_label():
    v = np.zeros((3, 4, 9), np.uint8)
    v[1, 1, 0:3] = 1                                                 # 3 voxels, first index (1*4+1)*9 = 45
    v[0, 2, 5:8] = 1                                                 # 3 voxels, first index 2*9+5 = 23
    v[2, 3, 7:9] = 1                                                 # 2 voxels, first index (2*4+3)*9+7 = 106
    lab, out, stats = cr.clean(v, 2, 26, "class", largest_only=True)
    assert sorted(np.unique(lab)) == [0, 24, 46, 107]
    want = np.zeros_like(v)
    want[0, 2, 5:8] = 1
    assert np.array_equal(out, want) and stats.tolist() == [[0, 0, 0], [3, 3, 5]]
    _, out, stats = cr.clean(v, 2, 26, "class", largest_only=False, min_voxels=3)
    want[1, 1, 0:3] = 1
    assert np.array_equal(out, want) and stats.tolist() == [[0, 0, 0], [3, 3, 2]]
    _, out, stats = cr.clean(v, 2, 26, "class", largest_only=True, min_voxels=4)
    assert not out.any() and stats.tolist() == [[0, 0, 0], [3, 3, 8]]


def test_two_classes_side_by_side():
    v = np.zeros((2, 3, 6), np.uint8)
    v[:, :, 0:2] = 1
    v[:, :, 2:6] = 2
    lab = cr.label(v, 6, "class")
    assert (lab[:, :, 0:2] == 1).all() and (lab[:, :, 2:6] == 3).all()
    assert (cr.label(v, 6, "foreground") == 1).all()
    _, out, stats = cr.clean(v, 3, 6, "foreground", largest_only=True, min_voxels=36)
    assert np.array_equal(out, v) and stats.tolist() == [[1, 36, 0], [0, 0, 0], [0, 0, 0]]
    _, out, stats = cr.clean(v, 3, 6, "class", largest_only=True, min_voxels=13)
    assert (out[:, :, 0:2] == 0).all() and (out[:, :, 2:6] == 2).all() and stats.tolist() == [[0, 0, 0], [1, 12, 12], [1, 24, 0]]


def test_values_beyond_k():
    v = np.zeros((1, 2, 6), np.uint8)
    v[0, 0, 0:2] = 1
    v[0, 0, 2:4] = 9                                                 # >= K
    v[0, 1, 5] = 1
    lab, out, stats = cr.clean(v, 3, 6, "class", largest_only=True)
    assert lab[0, 0].tolist() == [1, 1, 3, 3, 0, 0]                  # labelled like any other byte
    assert out[0, 0].tolist() == [1, 1, 9, 9, 0, 0] and out[0, 1, 5] == 0                    # copied through; in no statistic
    assert stats.tolist() == [[0, 0, 0], [2, 2, 1], [0, 0, 0]]
    lab, out, stats = cr.clean(v, 3, 6, "foreground", largest_only=True)
    assert lab[0, 0].tolist() == [1, 1, 1, 1, 0, 0] and out[0, 0].tolist() == [1, 1, 9, 9, 0, 0] and out[0, 1, 5] == 0
    assert stats.tolist() == [[2, 4, 1], [0, 0, 0], [0, 0, 0]]


def test_empty_and_zero_sized():
    lab, out, stats = cr.clean(np.zeros((2, 3, 4), np.uint8), 4)
    assert not lab.any() and not out.any() and not stats.any() and stats.shape == (4, 3)
    lab, out, stats = cr.clean(np.zeros((0, 3, 4), np.uint8), 4)
    assert lab.shape == out.shape == (0, 3, 4) and not stats.any()
