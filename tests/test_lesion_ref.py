"""tests/lesion_ref.py against hand-written known answers (CPU, no library): the restatement the device is held to must itself
be right.  Every volume is small enough to be checked by eye."""
import numpy as np

import lesion_ref as lr

NAN = float("nan")


def _vol(*boxes, shape=(4, 6, 12)):
    """boxes: (z0, z1, y0, y1, x0, x1) half-open, all set to 2 inside a liver of 1."""
    v = np.ones(shape, np.uint8)
    for z0, z1, y0, y1, x0, x1 in boxes:
        v[z0:z1, y0:y1, x0:x1] = 2
    return v


def _check(s, n_ref, n_pred, groups, dice, recall, precision, f1):
    assert (s["n_ref"], s["n_pred"]) == (n_ref, n_pred)
    assert s["groups"] == groups
    np.testing.assert_array_equal(s["group_dice"], np.array(dice, np.float64))
    np.testing.assert_array_equal(s["recall"], np.array(recall, np.float64))
    np.testing.assert_array_equal(s["precision"], np.array(precision, np.float64))
    np.testing.assert_array_equal(s["f1"], np.array(f1, np.float64))


def test_one_to_one():
    label = _vol((1, 3, 1, 3, 1, 3))                     # 8 voxels
    pred = _vol((1, 3, 1, 3, 2, 4))                      # 8 voxels, 4 shared: iou 4 / 12, dice 8 / 16
    s = lr.scores(pred, label, 2)
    _check(s, 1, 1, [([1], [1])], [0.5], [1.0, 0.0], [1.0, 0.0], [1.0, NAN])
    np.testing.assert_array_equal(s["group_iou"], [4 / 12])
    assert s["sizes_ref"].tolist() == [8] and s["sizes_pred"].tolist() == [8]


def test_split_prediction_is_one_group():
    label = _vol((1, 2, 1, 2, 1, 8))                     # a bar of 7
    pred = _vol((1, 2, 1, 2, 1, 4), (1, 2, 1, 2, 5, 8))  # 3 + 3, the middle voxel missing
    s = lr.scores(pred, label, 2)
    # A = 7, B = 6, I = 6: iou 6 / 7, dice 12 / 13; both predicted pieces are matched
    _check(s, 1, 2, [([1], [1, 2])], [12 / 13], [1.0, 1.0], [1.0, 1.0], [1.0, 1.0])


def test_two_references_bridged_by_one_prediction():
    label = _vol((1, 2, 1, 2, 1, 4), (1, 2, 1, 2, 6, 9))      # 3 + 3
    pred = _vol((1, 2, 1, 2, 1, 9))                           # 8, covers both and the gap
    s = lr.scores(pred, label, 2)
    # A = 6, B = 8, I = 6: iou 6 / 8 = 0.75, dice 12 / 14
    _check(s, 2, 1, [([1, 2], [1])], [12 / 14], [1.0, 1.0], [1.0, 1.0], [1.0, 1.0])


def test_miss_and_false_positive():
    label = _vol((0, 1, 0, 1, 0, 2), (2, 4, 3, 5, 8, 10))     # 2 (found exactly) + 8 (missed)
    pred = _vol((0, 1, 0, 1, 0, 2), (0, 1, 4, 5, 5, 6))       # 2 + a false positive of 1
    s = lr.scores(pred, label, 2)
    # reference lesions in C order: the 2-voxel one, then the 8-voxel one; predictions: the 2-voxel one, then the speck
    _check(s, 2, 2, [([1], [1]), ([2], []), ([], [2])], [1.0, 0.0, 0.0], [0.5, 0.5], [0.5, 0.5], [0.5, 0.5])


def test_iou_of_exactly_one_half_does_not_match_at_one_half():
    label = _vol((1, 2, 1, 2, 1, 5))                     # 4 voxels
    pred = _vol((1, 2, 1, 2, 1, 3))                      # 2 of them: I = 2, A + B - I = 4
    s = lr.scores(pred, label, 2, thresholds=(0.0, 0.49, 0.5))
    assert s["group_iou"].tolist() == [0.5]
    _check(s, 1, 1, [([1], [1])], [4 / 6], [1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [1.0, 1.0, NAN])


def test_both_sides_empty_and_one_side_empty():
    liver = _vol()
    s = lr.scores(liver, liver, 2)
    _check(s, 0, 0, [], [], [NAN, NAN], [NAN, NAN], [NAN, NAN])
    s = lr.scores(_vol((1, 2, 1, 2, 1, 3)), liver, 2)    # nothing to find, one false positive
    _check(s, 0, 1, [([], [1])], [0.0], [NAN, NAN], [0.0, 0.0], [NAN, NAN])
    s = lr.scores(liver, _vol((1, 2, 1, 2, 1, 3)), 2)
    _check(s, 1, 0, [([1], [])], [0.0], [0.0, 0.0], [NAN, NAN], [NAN, NAN])


def test_a_tuple_of_ids_counts_together():
    label = _vol((1, 2, 1, 2, 1, 5))
    label[1, 1, 3:5] = 3                                 # half the bar under another id
    s = lr.scores(label, label, (2, 3))
    _check(s, 1, 1, [([1], [1])], [1.0], [1.0, 1.0], [1.0, 1.0], [1.0, 1.0])
    assert lr.scores(label, label, 2)["sizes_ref"].tolist() == [2]


def test_rank_table_and_contingency():
    v = np.zeros((2, 3, 5), np.uint8)
    v[0, 0, 3:5] = 7                                     # first voxel 3
    v[0, 2, 0] = 1                                       # first voxel 10
    v[1, 1:3, 1] = 7                                     # first voxel 21; touches (0, 2, 0) by a corner only
    ranks, n = lr.rank(v, 26, "class")
    assert n == 3 and ranks[0, 0, 3] == 1 and ranks[0, 2, 0] == 2 and ranks[1, 2, 1] == 3
    count, t = lr.table(v, ranks, n, 2)
    assert count.tolist() == [3, 1]
    assert t.tolist() == [[-1, 25, 0, 0, 0, 2, 3, 5, 0], [3, 2, 0, 0, 3, 1, 1, 5, 7], [10, 1, 0, 2, 0, 1, 3, 1, 1],
                          [-1, 2, 1, 1, 1, 2, 3, 2, -1]]
    fg, n = lr.rank(v, 26, "foreground")                 # the corner now joins the last two
    assert n == 2 and fg[0, 2, 0] == 2 and fg[1, 2, 1] == 2
    assert lr.rank(v, 6, "foreground")[1] == 3
    c = lr.contingency(ranks, fg, 2, 1)                  # ranks clamped at 3, fg at 2
    assert c.tolist() == [[25, 0, 0], [0, 2, 0], [0, 0, 1], [0, 0, 2]] and c.sum() == v.size
