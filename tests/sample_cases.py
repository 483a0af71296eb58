"""Cases of the training-sample path (cfun_amd/sample.py, cfun_amd/csrc/sample.hip) shared by test_sample_emu.py and
test_sample_gpu.py: the device against tests/sample_ref.py.  Both sides compute the rotation's source index and the IoU in
float64 in the same operation order, so image and labels must be torch.equal everywhere (edges included), boxes, rpn_match and
counts exact; rpn_bbox (float32 on the device, float64 in the restatement; only log() may differ) within 2 float32 ulp."""
import re

import numpy as np
import torch

import guard
import sample_ref as sr
from conftest import ROOT, load_golden

SHAPES = [(10, 14, 5), (24, 20, 7), (33, 65, 3), (16, 16, 70), (7, 9, 1)]     # [H,W,D]: ragged tiles on every axis, D below and
ANGLES = [13.0, -20.0]                                                        # above a 64-tile, a single plane
STD = np.array([0.1, 0.1, 0.1, 0.2, 0.2, 0.2])


def _rng(seed):
    return np.random.default_rng(seed)


def _volume(shape, seed, kind="blob"):
    h, w, d = shape
    rng = _rng(seed)
    image = rng.normal(1.0, 2.0, shape).astype(np.float32)
    mask = np.zeros(shape, np.int32)
    if kind == "blob":
        lo = [n // 4 for n in shape]
        hi = [max(l + 1, n - n // 5) for l, n in zip(lo, shape)]
        mask[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = rng.integers(0, 8, [b - a for a, b in zip(lo, hi)])
    elif kind == "faces":                      # label > 0 on all six faces: the expansion clamps on every side
        mask[:] = rng.integers(1, 256, shape)
    elif kind == "plane":                      # one plane thick along z: the reference's zero box
        mask[h // 4:h - 1, w // 4:w - 1, d // 2] = 3
    elif kind == "empty":
        pass
    return image, mask


def check_rotate_case(device, image, mask, angle, t_image=None, t_mask=None):
    """image / mask: numpy [H,W,D]; t_image / t_mask: the (possibly strided) device views holding the same values."""
    from cfun_amd import sample
    ti = torch.from_numpy(image).to(device) if t_image is None else t_image
    tm = torch.from_numpy(mask).to(device) if t_mask is None else t_mask
    out, lab, raw, box, empty = sample.rotate_and_box(ti, tm, angle)
    r_img, r_lab, r_raw, r_box, r_empty = sr.rotate_and_box(image, mask, angle)
    assert out.dtype == torch.float32 and lab.dtype == torch.uint8 and raw.dtype == box.dtype == empty.dtype == torch.int32
    assert torch.equal(out.cpu(), torch.from_numpy(r_img)), "image, angle %r" % (angle,)
    assert torch.equal(lab.cpu(), torch.from_numpy(r_lab)), "labels, angle %r" % (angle,)
    assert raw.cpu().tolist() == r_raw.tolist() and box.cpu().tolist() == r_box.tolist(), (raw, r_raw, box, r_box)
    assert empty.cpu().tolist() == [r_empty]
    return out, lab, raw, box, empty


def check_rotate_shape(device, shape):
    image, mask = _volume(shape, 100 + shape[2])
    for angle in ANGLES:
        check_rotate_case(device, image, mask, angle)
    a0 = check_rotate_case(device, image, mask, 0.0)
    n0 = check_rotate_case(device, image, mask, None)            # rotate = 0 (the LiTS form) must equal angle 0
    assert all(torch.equal(p, q) for p, q in zip(a0, n0))
    assert torch.equal(n0[0].cpu(), torch.from_numpy(image).permute(2, 0, 1))


def check_rotate_strided(device):
    """Sources read in place through their strides: a permuted view (the loader's array stored [D,H,W]) and a sliced view."""
    shape = (24, 20, 7)
    image, mask = _volume(shape, 7)
    ti = torch.from_numpy(np.ascontiguousarray(image.transpose(2, 0, 1))).to(device).permute(1, 2, 0)
    tm = torch.from_numpy(np.ascontiguousarray(mask.transpose(1, 2, 0))).to(device).permute(2, 0, 1)
    assert not ti.is_contiguous() and not tm.is_contiguous()
    check_rotate_case(device, image, mask, 13.0, ti, tm)
    big_i, big_m = _volume((26, 43, 10), 8)
    ti, tm = torch.from_numpy(big_i).to(device)[1:25, 2:42:2, 3:], torch.from_numpy(big_m).to(device)[1:25, 2:42:2, 3:]
    assert not ti.is_contiguous()
    check_rotate_case(device, np.ascontiguousarray(big_i[1:25, 2:42:2, 3:]), np.ascontiguousarray(big_m[1:25, 2:42:2, 3:]), -20.0, ti, tm)


def check_rotate_boxes(device):
    for shape in ((10, 14, 5), (16, 16, 70)):
        image, mask = _volume(shape, 21, "faces")
        _, _, raw, box, _ = check_rotate_case(device, image, mask, None)
        d, h, w = shape[2], shape[0], shape[1]
        assert raw.cpu().tolist() == box.cpu().tolist() == [0, 0, 0, d, h, w]          # clamped on all six sides
        check_rotate_case(device, image, mask, 13.0)
        image, mask = _volume(shape, 22, "plane")
        _, _, raw, box, empty = check_rotate_case(device, image, mask, None)
        assert not raw.cpu().any() and not box.cpu().any() and int(empty.cpu()) == 0   # one plane: the zero box, not "empty"
        image, mask = _volume(shape, 23, "empty")
        _, _, raw, box, empty = check_rotate_case(device, image, mask, 7.0)
        assert not raw.cpu().any() and not box.cpu().any() and int(empty.cpu()) == 1


def check_rotate_wrapper_preconditions(device):
    import pytest
    from cfun_amd import sample
    image, mask = _volume((10, 14, 5), 5)
    ti, tm = torch.from_numpy(image).to(device), torch.from_numpy(mask).to(device)
    with pytest.raises(ValueError, match="differ in shape"):
        sample.rotate_and_box(ti, tm[:, :, :4], 0.0)
    with pytest.raises(ValueError, match="integer label"):
        sample.rotate_and_box(ti, ti, 0.0)
    with pytest.raises(ValueError, match=r"\[0, 255\]"):
        sample.rotate_and_box(ti, tm + 300, 0.0, strict=True)
    with pytest.raises(ValueError, match="empty"):
        sample.rotate_and_box(ti, tm * 0, 0.0, strict=True)


# ---------------------------------------------------------------------------------------------------------- RPN targets
class _Cfg:
    def __init__(self, r, num_classes=8):
        self.RPN_TRAIN_ANCHORS_PER_IMAGE = r
        self.RPN_BBOX_STD_DEV = STD
        self.NUM_CLASSES = num_classes


def check_targets_case(device, anchors, gt, r, keys):
    from cfun_amd import sample
    a = anchors.shape[0]
    match, bbox, counts = sample.build_rpn_targets(torch.from_numpy(anchors).to(device), torch.from_numpy(np.asarray(gt)).to(device),
                                                   _Cfg(r), torch.from_numpy(np.asarray(keys).astype(np.int64)).to(device))
    assert tuple(match.shape) == (1, a, 1) and match.dtype == torch.int32
    assert tuple(bbox.shape) == (1, r, 6) and bbox.dtype == torch.float32 and counts.dtype == torch.int32
    r_match, r_bbox, r_counts = sr.build_rpn_targets(anchors, gt, r, STD, keys)
    assert np.array_equal(match.cpu().numpy()[0, :, 0], r_match), "%d rpn_match entries differ" % int(
        (match.cpu().numpy()[0, :, 0] != r_match).sum())
    assert counts.cpu().tolist() == r_counts.tolist()
    sr.ulp32_close(bbox.cpu().numpy()[0], r_bbox)
    return match.cpu().numpy()[0, :, 0], bbox.cpu().numpy()[0], r_counts


def check_targets_golden(device, tag):
    """Keys built from the drops the reference's np.random.choice made reproduce the reference's own rpn_match and rpn_bbox."""
    g = load_golden("sample_targets")
    anchors, gt, r = g[tag + "_anchors"], g[tag + "_gt"], int(g[tag + "_r"])
    ov = sr.overlaps(anchors, gt)
    if gt.shape[0] == 3:
        assert ov[:, 2].max() < sr.NEG_IOU                              # a GT whose best anchor is below 0.3: positive all the same
        dup = np.nonzero((anchors[1:] == anchors[:-1]).all(axis=1))[0]
        assert dup.size > 10 and (ov[dup] == ov[dup + 1]).all()         # duplicated anchors: equal IoU rows
        # GT 1's and GT 2's best IoU is shared by two copies of one anchor whose IoU with every GT is below 0.7: only "every GT's
        # best anchor, the first index wins" decides which copy is positive, and the reference's rpn_match records the first
        ties = [np.nonzero(ov[:, j] == ov[:, j].max())[0] for j in (1, 2)]
        assert all(t.size > 1 and ov[t].max() < sr.POS_IOU for t in ties)
        firsts, laters = [int(t[0]) for t in ties], np.concatenate([t[1:] for t in ties])
        assert (g[tag + "_rpn_match"][firsts] == 1).all() and (g[tag + "_rpn_match"][laters] != 1).all()
    match, bbox, counts = check_targets_case(device, anchors, gt, r, sr.keys_from_drops(anchors.shape[0], g[tag + "_drops"]))
    assert np.array_equal(match, g[tag + "_rpn_match"])
    sr.ulp32_close(bbox, g[tag + "_rpn_bbox"])
    assert counts.tolist() == [r // 2, r - r // 2]                      # both budgets were exceeded in this fixture
    # colliding and full-range keys on the same sets: (key, index) order decides
    rng = _rng(r)
    check_targets_case(device, anchors, gt, r, rng.integers(0, 3, anchors.shape[0]))
    check_targets_case(device, anchors, gt, r, rng.integers(0, 1 << 32, anchors.shape[0], dtype=np.uint64))
    check_targets_case(device, anchors, gt, r, np.zeros(anchors.shape[0], np.int64))
    other = 128 if r == 16 else 16
    match, _, counts = check_targets_case(device, anchors, gt, other, rng.integers(0, 5, anchors.shape[0]))
    if gt.shape[0] == 3:                                                # R = 128 keeps every positive: the tie shows whatever the keys
        assert counts[0] < other // 2 and (match[firsts] == 1).all() and (match[laters] != 1).all()


def check_targets_few_negatives(device):
    """Fewer negatives than the budget (all stay), more positives than R // 2; G = 1 and a first-GT tie at G = 3."""
    rng = _rng(31)
    gt = np.array([[4, 6, 6, 20, 30, 28]], np.float32)
    a = gt + rng.integers(-6, 7, (875, 6)) / 2.0
    a[-9:] = np.array([0, 0, 0, 2, 2, 2], np.float32) + rng.integers(0, 3, (9, 1))          # nine far boxes: the only negatives
    a = a.astype(np.float32)
    full, _, _ = sr.build_rpn_targets(a, gt, 10 ** 6, STD, np.zeros(875))                   # no subsampling
    n_neg = int((full == -1).sum())
    assert 9 <= n_neg < 64 and (full == 1).sum() > 64
    for r in (16, 128):
        match, _, counts = check_targets_case(device, a, gt, r, rng.integers(0, 2, 875))
        assert counts[0] == r // 2 and counts[1] == min(n_neg, r - r // 2) and (match == -1).sum() == counts[1]
    # GT 1 is GT 0 shifted by 2 along z and anchors 0 .. 5 sit symmetrically between the two: bit-equal IoU with both (>= 0.7),
    # opposite dz.  Only "the first GT wins a tie" picks their deltas; key 0 keeps them among the 64 positives that stay.
    gt3 = np.concatenate([gt, gt + np.array([2, 0, 0, 2, 0, 0], np.float32), gt + 1])
    a[:6] = 0.5 * (gt3[0] + gt3[1]) + np.array([[-e, p, q, e, -p, -q] for e, p, q in
                                                ((0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, .5, 0), (1, 0, .5), (-1, .5, .5))], np.float32)
    keys = rng.integers(1, 3, 875)
    keys[:6] = 0
    ov = sr.overlaps(a, gt3)
    assert (ov[:6, 0] == ov[:6, 1]).all() and (ov[:6, 0] >= sr.POS_IOU).all() and (ov[:6, 0] > ov[:6, 2]).all()
    match, bbox, _ = check_targets_case(device, a, gt3, 128, keys)
    assert (match == 1).sum() == 64 and (match[:6] == 1).all()
    assert (bbox[:6, 0] < 0).all()                                      # towards GT 0, the lower one (GT 1 would give dz = -these)


def check_targets_random_keys(device):
    """keys=None draws on the device: the counts and the budgets hold whatever the draw."""
    from cfun_amd import sample
    g = load_golden("sample_targets")
    anchors, gt = g["bt875_anchors"], g["bt875_gt"]
    match, bbox, counts = sample.build_rpn_targets(torch.from_numpy(anchors).to(device), torch.from_numpy(gt).to(device), _Cfg(16))
    m = match.cpu().numpy()[0, :, 0]
    full, _, _ = sr.build_rpn_targets(anchors, gt, 10 ** 6, STD, np.zeros(875))               # no subsampling
    assert counts.cpu().tolist() == [8, 8] and (m == 1).sum() == 8 and (m == -1).sum() == 8
    assert (full[m == 1] == 1).all() and (full[m == -1] == -1).all()
    assert np.isfinite(bbox.cpu().numpy()[0, :8]).all() and not bbox.cpu().numpy()[0, 8:].any()


def check_targets_zero_size(device):
    """A = 0 and G = 0: correctly shaped zeros, nothing launched, nothing written (under guard: no band touched)."""
    from cfun_amd import sample
    anchors = torch.from_numpy(load_golden("sample_targets")["bt875_anchors"]).to(device)
    for a, g in ((anchors[:0], torch.ones(1, 6, device=device)), (anchors, torch.ones(0, 6, device=device))):
        match, bbox, counts = sample.build_rpn_targets(a, g, _Cfg(16))
        assert tuple(match.shape) == (1, a.shape[0], 1) and tuple(bbox.shape) == (1, 16, 6)
        assert not match.cpu().any() and not bbox.cpu().any() and counts.cpu().tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------------------ end to end
def check_load_image_gt_golden(device, tag):
    """cfun_amd.sample.load_image_gt on the reference's recorded inputs against what the reference's own load_image_gt returned
    (the rotation itself went through sample_ref's rule there: see gen_sample_golden.py)."""
    from cfun_amd import sample
    g = load_golden("sample_targets")
    lits = tag == "lits"
    mask = torch.from_numpy(g[tag + "_mask_in"].astype(np.int32)).to(device)
    image = torch.zeros(mask.shape, device=device) + 1.0 if lits else torch.from_numpy(g[tag + "_image_in"]).to(device)
    ncls, r = [int(v) for v in g[tag + "_cfg"]]
    cfg = _Cfg(r, ncls)
    cfg.RPN_BBOX_STD_DEV = g[tag + "_std"]
    a = g[tag + "_anchors"]
    keys = torch.from_numpy(sr.keys_from_drops(a.shape[0], g[tag + "_drops"]).astype(np.int64)).to(device)
    s = sample.load_image_gt(image[..., None], mask, None if lits else float(g[tag + "_angle"]), cfg, torch.from_numpy(a).to(device), keys)
    assert np.array_equal(s["gt_boxes"].cpu().numpy(), g[tag + "_bbox"].astype(np.float32)) and s["gt_boxes"].dtype == torch.float32
    assert np.array_equal(s["rpn_match"].cpu().numpy()[0], g[tag + "_rpn_match"])
    sr.ulp32_close(s["rpn_bbox_t"].cpu().numpy()[0], g[tag + "_rpn_bbox"])
    assert s["gt_class_ids"].cpu().tolist() == list(range(1, ncls))
    assert s["gt_labels"].dtype == torch.uint8 and tuple(s["image"].shape) == (1, 1) + tuple(s["gt_labels"].shape)
    if not lits:
        assert s["gt_class_ids"].cpu().tolist() == g[tag + "_class_ids"].tolist()
        np.testing.assert_allclose(s["image"].cpu().numpy()[0], g[tag + "_image"], rtol=1e-5, atol=1e-6)


def check_make_sample_feeds_train_epoch(device, seed=2):
    """make_sample on the tiny configuration feeds one train_epoch step: the sample's tensors equal the sample_ref-built sample's
    bit for bit, and the step's losses are finite and equal those of the same step fed the sample_ref-built sample."""
    import copy
    import module_cases as mc
    from cfun_amd import sample, step, train, utils
    cfg = mc.tiny_config("beginning")
    cfg.BATCH_SIZE = 1
    torch.manual_seed(seed)
    net = step.CFUNHotPath(cfg).to(device)
    b = cfg.UNET_MASK_BRANCH_CHANNEL
    gen = torch.Generator().manual_seed(1)
    masks = [torch.empty(cfg.TRAIN_ROIS_PER_IMAGE, c).bernoulli_(0.4, generator=gen) / 0.4 for c in (b, 2 * b, 4 * b, 8 * b, 16 * b)]
    net.mask.modified_u_net.dropout_masks = masks
    ref_net = copy.deepcopy(net)
    ref_net.mask.modified_u_net.dropout_masks = masks
    rng = _rng(seed)
    src = (40, 36, 20)                                     # the loader's volume: not the network size
    image = rng.normal(0.0, 1.0, src).astype(np.float32)
    mask = np.zeros(src, np.int32)
    mask[8:32, 7:30, 3:17] = rng.integers(1, cfg.NUM_CLASSES, (24, 23, 14))
    anchors = net.anchors.to(device)
    keys = torch.from_numpy(rng.integers(0, 1 << 32, anchors.shape[0], dtype=np.uint64).astype(np.int64)).to(device)
    angle = 13.0
    s = sample.make_sample(image, mask, angle, cfg, anchors, keys=keys, strict=True)

    mx, mn = int(cfg.IMAGE_MAX_DIM), int(cfg.IMAGE_MIN_DIM)
    dev = torch.device(device)
    r_image = utils.resize_image(torch.from_numpy(image)[..., None].to(dev), min_dim=mn, max_dim=mx, mode="self", device=dev)[0]
    r_mask = utils.resize_mask(torch.from_numpy(mask).to(dev), None, None, max_dim=mx, min_dim=mn, mode="self", device=dev)
    ref = sr.load_image_gt(r_image[..., 0].cpu().numpy(), r_mask.cpu().numpy(), angle, cfg.NUM_CLASSES, anchors.cpu().numpy(),
                           cfg.RPN_TRAIN_ANCHORS_PER_IMAGE, cfg.RPN_BBOX_STD_DEV, keys.cpu().numpy())
    assert ref["empty"] == 0 and (ref["rpn_match"] == 1).any()
    rs = dict(image=utils.mold_image(torch.from_numpy(ref["image_raw"]).to(dev))[None, None],
              gt_class_ids=torch.from_numpy(ref["gt_class_ids"]).to(dev), gt_boxes=torch.from_numpy(ref["gt_boxes"]).to(dev),
              gt_labels=torch.from_numpy(ref["gt_labels"]).to(dev), rpn_match=torch.from_numpy(ref["rpn_match"]).to(dev),
              rpn_bbox_t=torch.from_numpy(ref["rpn_bbox_t"]).to(dev))
    for k in ("image", "gt_class_ids", "gt_boxes", "gt_labels", "rpn_match", "rpn_bbox_t"):
        assert s[k].dtype == rs[k].dtype and torch.equal(s[k], rs[k]), k

    def one_step(n, smp):
        opt = train.make_optimizer(n, cfg, bucket_bytes=1 << 16)
        torch.manual_seed(11)                              # detection_target_layer's randperm draws
        return train.train_epoch(n, [smp], opt, 1, cfg)

    got, want = one_step(net, s), one_step(ref_net, rs)
    assert all(np.isfinite(v) for v in got), got
    assert got == want, (got, want)
    assert got[1] > 0 and got[2] > 0                       # the RPN losses saw the targets


# ------------------------------------------------------------------------------------------------------------ accounting
def sample_header_symbols():
    """The same parse as test_abi.header_symbols, on include/cfun_sample.h."""
    import os
    txt = open(os.path.join(ROOT, "include", "cfun_sample.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(cfun_[a-z0-9_]+)\s*\(", txt)))


SAMPLE_NO_LAUNCH = {"cfun_sample_workspace_bytes": "host-side query: launches nothing, touches no device memory"}


def check_coverage(tier):
    from cfun_amd import _lib
    assert sample_header_symbols() == sorted(_lib.SAMPLE_EXPORTS)
    assert not set(_lib.SAMPLE_EXPORTS) & set(_lib.EXPORTS)
    missed = sorted(set(_lib.SAMPLE_EXPORTS) - set(SAMPLE_NO_LAUNCH) - guard.SEEN[tier])
    assert not missed, "sample entries that launch work but never ran under guard: %s" % missed
