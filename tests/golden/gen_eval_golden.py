#!/usr/bin/env python3
"""Golden vectors of the scoring path (tests/golden/eval_iou.npz).  RUNS ONLY WHERE THE REFERENCE IS (see gen_golden.py, whose
shims and imports this script reuses).  Only DATA is stored.

Recorded, from the reference's own functions, for the main tree and the LiTS fork: utils.compute_per_class_mask_iou on the two
one-hot arrays its test() builds (heart_main.py:321-330) and utils.compute_mask_iou (called on copies: it overwrites its
arguments) for a handful of small seeded label / prediction pairs -- a class absent from both volumes, a class absent from one of
them, a perfect match, an empty prediction.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_eval_golden.py
"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as gg  # noqa: E402  (installs the shims, imports the reference)


def one_hot(vol, k):
    """heart_main.py:321-328: float64 [H,W,D,k-1], plane j set where vol == j + 1."""
    out = np.zeros(vol.shape + (k - 1,))
    for j in range(k - 1):
        out[:, :, :, j][vol == j + 1] = 1
    return out


def volumes(rng, shape, k, present_label, present_pred):
    """~90 % background; labels drawn from ``present_label``, predictions agree with the label on ~70 % of the foreground and
    are drawn from ``present_pred`` elsewhere."""
    label = np.zeros(shape, np.int32)
    fg = rng.rand(*shape) < 0.12
    label[fg] = rng.choice(present_label, int(fg.sum()))
    pred = np.zeros(shape, np.int32)
    pfg = fg ^ (rng.rand(*shape) < 0.03)
    pred[pfg] = rng.choice(present_pred, int(pfg.sum()))
    agree = fg & pfg & (rng.rand(*shape) < 0.7) & np.isin(label, present_pred)
    pred[agree] = label[agree]
    return label, pred


def main():
    rng = np.random.RandomState(31)
    ref_utils = gg.ref_utils
    _, lits_utils = gg.import_lits()
    out, tags = {}, []
    cases = [("all8", (24, 20, 12), 8, list(range(1, 8)), list(range(1, 8))),
             ("absent_both", (17, 23, 9), 8, [1, 2, 3, 5, 6, 7], [1, 2, 3, 5, 6, 7]),       # class 4 in neither volume
             ("absent_pred", (40, 40, 40), 8, list(range(1, 8)), [1, 2, 4, 5, 6, 7]),       # class 3 never predicted
             ("absent_label", (16, 16, 33), 8, [1, 3, 4, 5, 6, 7], list(range(1, 8))),      # class 2 never labelled
             ("lits3", (30, 26, 14), 3, [1, 2], [1, 2])]
    for tag, shape, k, pl, pp in cases:
        label, pred = volumes(rng, shape, k, pl, pp)
        out[tag + "_label"], out[tag + "_pred"], out[tag + "_k"] = label.astype(np.uint8), pred.astype(np.uint8), np.array(k)
        tags.append(tag)
    label, _ = volumes(rng, (20, 18, 10), 8, list(range(1, 8)), list(range(1, 8)))
    out.update(perfect_label=label.astype(np.uint8), perfect_pred=label.astype(np.uint8), perfect_k=np.array(8))
    out.update(nopred_label=label.astype(np.uint8), nopred_pred=np.zeros_like(label, np.uint8), nopred_k=np.array(8))
    tags += ["perfect", "nopred"]
    for tag in tags:
        label, pred, k = out[tag + "_label"].astype(np.int32), out[tag + "_pred"].astype(np.int32), int(out[tag + "_k"])
        for tree, u in (("main", ref_utils), ("lits", lits_utils)):
            out["%s_%s_per_class" % (tag, tree)] = np.asarray(u.compute_per_class_mask_iou(one_hot(label, k), one_hot(pred, k)), np.float64)
            out["%s_%s_mask" % (tag, tree)] = np.asarray(u.compute_mask_iou(label.copy(), pred.copy()), np.float64)
        assert np.array_equal(out[tag + "_main_per_class"], out[tag + "_lits_per_class"])
    out["tags"] = np.array(tags)
    gg.save("eval_iou", **out)


if __name__ == "__main__":
    main()
