#!/usr/bin/env python3
"""Golden vectors of the training-sample path (tests/golden/sample_targets.npz).  RUNS ONLY WHERE THE REFERENCE IS (see
gen_golden.py, whose shims and imports this script reuses).  Only DATA is stored.

Recorded, from the reference's own functions, for the main tree and the LiTS fork:
  * utils.extract_bboxes on label volumes (an ordinary object, one touching all six faces, a one-plane object);
  * the box tail of load_image_gt (model.py:1059-1076) / utils.extend_bbox;
  * load_image_gt itself -- the main tree's with a stub ``imgaug`` whose Affine applies tests/sample_ref.py's rotation (imgaug
    is not installed: the rotation's parity with imgaug is NOT pinned, everything behind it is);
  * build_rpn_targets on hand-made anchor sets, with the ids its two np.random.choice draws dropped.
The generator asserts that no IoU lies within 1e-6 of 0.3 / 0.7: numpy 1 and numpy 2 promote int32 (x) float32 differently
and the fixture must not depend on that.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_sample_golden.py
"""
import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as gg  # noqa: E402  (installs the shims, imports the reference)
import sample_ref as sr  # noqa: E402


def install_imgaug_stub():
    ia = types.ModuleType("imgaug")
    aug = types.ModuleType("imgaug.augmenters")

    class Affine:
        def __init__(self, rotate=0, order=0):
            assert order == 0
            self.rotate = rotate

        def to_deterministic(self):
            return self

        def augment_image(self, image, hooks=None):
            return sr.rotate_slices(image, self.rotate)

    class HooksImages:
        def __init__(self, activator=None):
            self.activator = activator

    aug.Affine = Affine
    ia.augmenters = aug
    ia.HooksImages = HooksImages
    sys.modules["imgaug"] = ia
    sys.modules["imgaug.augmenters"] = aug


class RecordedChoice:
    """np.random.choice replaced by a seeded draw that records what it returned (the ids set neutral)."""

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.drops = []

    def __enter__(self):
        self.orig = np.random.choice

        def choice(ids, size, replace=True):
            out = self.rng.choice(ids, size, replace=replace)
            self.drops.append(np.asarray(out, np.int64))
            return out
        np.random.choice = choice
        return self

    def __exit__(self, *exc):
        np.random.choice = self.orig

    def all(self):
        return np.concatenate(self.drops) if self.drops else np.zeros(0, np.int64)


def assert_iou_margin(anchors, gt):
    ov = sr.overlaps(anchors, gt)
    for thr in (sr.NEG_IOU, sr.POS_IOU):
        assert np.abs(ov - thr).min() > 1e-6, "an IoU within 1e-6 of %g: choose other boxes" % thr


def blob(h, w, d, lo, hi, rng, classes):
    m = np.zeros((h, w, d), np.int32)
    m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = rng.randint(1, classes, (hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]))
    return m


def anchor_set(n, dims, rng, dup_every=7):
    """Cubic-ish boxes with half-integer corners inside ``dims`` (D,H,W); every ``dup_every``-th repeats its predecessor."""
    c = np.stack([rng.randint(0, 2 * dims[k], n) / 2.0 for k in range(3)], axis=1)
    s = rng.randint(4, 25, (n, 3)) / 2.0
    a = np.concatenate([c - s, c + s], axis=1).astype(np.float32)
    a[dup_every::dup_every] = a[dup_every - 1::dup_every][:a[dup_every::dup_every].shape[0]]
    return a


def main():
    install_imgaug_stub()
    rng = np.random.RandomState(20)
    out = {}
    ref_model, ref_utils = gg.ref_model, gg.ref_utils
    lits_model, lits_utils = gg.import_lits()

    # ---- boxes: extract_bboxes and the 5 % tail, both trees
    h, w, d = 24, 20, 12
    masks = dict(obj=blob(h, w, d, (5, 4, 3), (17, 15, 9), rng, 8), faces=blob(h, w, d, (0, 0, 0), (h, w, d), rng, 8),
                 plane=blob(h, w, d, (5, 4, 6), (17, 15, 7), rng, 8))
    for tag, m in masks.items():
        dhw = m.transpose(2, 0, 1)
        raw = ref_utils.extract_bboxes(np.expand_dims(dhw, -1))
        assert np.array_equal(raw[0], lits_utils.extract_bboxes(dhw))
        out["box_%s_mask" % tag] = m.astype(np.uint8)
        out["box_%s_raw" % tag] = raw[0]
        out["box_%s_lits" % tag] = lits_utils.extend_bbox(lits_utils.extract_bboxes(dhw), dhw.shape)

    # ---- the main tree's load_image_gt (stub imgaug = sample_ref's rotation), R small enough that both draws happen
    cfg = gg.make_cfg("beginning", 32, 16, RPN_ANCHOR_SCALES=(16, 32), RPN_TRAIN_ANCHORS_PER_IMAGE=16)
    ih, iw, idp = [int(v) for v in cfg.IMAGE_SHAPE[:3]]
    anchors = ref_utils.generate_pyramid_anchors(cfg.RPN_ANCHOR_SCALES, cfg.RPN_ANCHOR_RATIOS,
                                                 ref_model.compute_backbone_shapes(cfg, cfg.IMAGE_SHAPE), cfg.BACKBONE_STRIDES,
                                                 cfg.RPN_ANCHOR_STRIDE).astype(np.float32)
    image = rng.normal(2.0, 3.0, (ih, iw, idp, 1)).astype(np.float32)
    mask = blob(ih, iw, idp, (6, 9, 2), (25, 24, 14), rng, cfg.NUM_CLASSES)
    dataset = types.SimpleNamespace(num_classes=cfg.NUM_CLASSES)
    dataset.process_mask = lambda m: gg.ref_heart.HeartDataset.process_mask(dataset, m)
    for tag, angle in (("main13", 13.0), ("main0", 0.0)):
        with RecordedChoice(7) as rec:
            im, match, bbox_t, class_ids, bbox, _ = ref_model.load_image_gt(image.copy(), mask.copy(), angle, dataset, cfg, anchors)
        assert_iou_margin(anchors, bbox[:1])
        out.update({tag + "_angle": np.array(angle), tag + "_image_in": image[..., 0], tag + "_mask_in": mask.astype(np.uint8),
                    tag + "_anchors": anchors, tag + "_image": im.astype(np.float32), tag + "_rpn_match": match.astype(np.int32),
                    tag + "_rpn_bbox": bbox_t.astype(np.float64), tag + "_class_ids": class_ids.astype(np.int32),
                    tag + "_bbox": bbox.astype(np.int32), tag + "_drops": rec.all(),
                    tag + "_cfg": np.array([cfg.NUM_CLASSES, cfg.RPN_TRAIN_ANCHORS_PER_IMAGE]),
                    tag + "_std": np.asarray(cfg.RPN_BBOX_STD_DEV, np.float64)})

    # ---- the LiTS fork's load_image_gt (no rotation)
    lcfg = gg.make_lits_cfg("beginning", RPN_TRAIN_ANCHORS_PER_IMAGE=16)
    lh, lw, ld = [int(v) for v in lcfg.IMAGE_SHAPE[:3]]
    lanchors = lits_utils.generate_pyramid_anchors(lcfg.RPN_ANCHOR_SCALES, lcfg.RPN_ANCHOR_RATIOS,
                                                   lits_model.compute_backbone_shapes(lcfg, lcfg.IMAGE_SHAPE),
                                                   lcfg.BACKBONE_STRIDES, lcfg.RPN_ANCHOR_STRIDE).astype(np.float32)
    lmask = blob(lh, lw, ld, (3, 8, 1), (22, 27, 13), rng, lcfg.NUM_CLASSES)
    with RecordedChoice(8) as rec:
        match, bbox_t, bbox = lits_model.load_image_gt(lmask.transpose(2, 0, 1).copy(), lcfg, lanchors)
    assert_iou_margin(lanchors, bbox[:1])
    out.update(lits_mask_in=lmask.astype(np.uint8), lits_anchors=lanchors, lits_rpn_match=match.astype(np.int32),
               lits_rpn_bbox=bbox_t.astype(np.float64), lits_bbox=bbox.astype(np.int32), lits_drops=rec.all(),
               lits_cfg=np.array([lcfg.NUM_CLASSES, lcfg.RPN_TRAIN_ANCHORS_PER_IMAGE]),
               lits_std=np.asarray(lcfg.RPN_BBOX_STD_DEV, np.float64))

    # ---- build_rpn_targets on hand-made sets: duplicates, several GTs, a GT no anchor overlaps well, both budgets exceeded
    dims = (16, 32, 32)
    for tag, n, gts, r in (("bt875", 875, [[2, 4, 4, 12, 20, 20], [6, 12, 10, 16, 30, 28], [0, 0, 29, 1, 1, 32]], 16),
                           ("bt1001", 1001, [[3, 6, 5, 13, 26, 27]], 128)):
        a = anchor_set(n, dims, rng)
        gt = np.array(gts, np.int32)
        # a cluster of near-copies of the first GT: more positives than R // 2
        k = 12 if r == 16 else 80
        a[20:20 + k] = gt[0].astype(np.float32) + rng.randint(-1, 2, (k, 6)) / 2.0
        a[27] = a[26]
        if gt.shape[0] == 3:
            # a later exact copy of the single best anchor of GT 1 and of GT 2 (best IoU below 0.7, GT 2's below 0.3): nothing
            # but "the first index wins a tie" decides which copy turns positive, and rpn_match differs if the other one does
            ov = sr.overlaps(a, gt)
            for j, dst in ((1, 3), (2, 859)):                  # GT 1's copy sits before its original, GT 2's behind it
                best = int(np.argmax(ov[:, j]))
                assert 100 < best and best != dst and (ov[:, j] == ov[best, j]).sum() == 1 and ov[best].max() < sr.POS_IOU
                a[dst] = a[best]
            ov = sr.overlaps(a, gt)
            ties = [np.nonzero(ov[:, j] == ov[:, j].max())[0] for j in (1, 2)]
            assert all(t.size == 2 and ov[t].max() < sr.POS_IOU for t in ties)
            firsts = [int(t[0]) for t in ties]
        else:
            firsts = []
        assert_iou_margin(a, gt)
        tcfg = types.SimpleNamespace(RPN_TRAIN_ANCHORS_PER_IMAGE=r, RPN_BBOX_STD_DEV=cfg.RPN_BBOX_STD_DEV)
        for seed in range(9, 64):                              # the first seed whose positive draw keeps the tied GTs' anchors,
            with RecordedChoice(seed) as rec:                  # so that the recorded rpn_match itself shows which copy won
                match, bbox_t = ref_model.build_rpn_targets(a, gt, tcfg)
            if all(match[i] == 1 for i in firsts):
                break
        else:
            raise AssertionError("no seed keeps the tied anchors")
        with RecordedChoice(seed) as rec2:
            lmatch, lbbox = lits_model.build_rpn_targets(a, gt, tcfg)
        assert np.array_equal(match, lmatch) and np.array_equal(bbox_t, lbbox) and np.array_equal(rec.all(), rec2.all())
        assert len(rec.drops) == 2, "both draws must happen in this fixture"
        out.update({tag + "_anchors": a, tag + "_gt": gt, tag + "_r": np.array(r), tag + "_rpn_match": match.astype(np.int32),
                    tag + "_rpn_bbox": bbox_t.astype(np.float64), tag + "_drops": rec.all(),
                    tag + "_std": np.asarray(cfg.RPN_BBOX_STD_DEV, np.float64)})

    gg.save("sample_targets", **out)


if __name__ == "__main__":
    main()
