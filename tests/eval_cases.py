"""Cases of the scoring path (cfun_amd/evaluate.py, cfun_amd/csrc/eval.hip) shared by test_eval_emu.py and test_eval_gpu.py: the
device against tests/eval_ref.py (counts: integers, torch.equal) and against the reference's own IoU functions through
tests/golden/eval_iou.npz (rtol 2^-22: below 2^24 voxels the reference's float32 sums are exact, and its result differs from the
float64 quotient of the exact counts by two float32 roundings -- the + 1e-6 and the division -- at most 2 * 2^-24 relative)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import eval_ref as er
import guard
from conftest import ROOT, load_golden

# [H,W,D]: below one 128 x 128 tile on every axis; exact multiples of the 64-lane halves; ragged on all three axes with W % 4 != 0
# and one voxel over 64 in z; several tiles along x and less than one along z; more than one tile along z and along y-as-fast-axis
SHAPES = [(5, 7, 3), (1, 1, 1), (64, 64, 64), (33, 70, 65), (40, 130, 20), (130, 9, 131)]
LAYOUTS = ("zfast", "dense", "yfast")
RTOL = 2.0 ** -22


def _volumes(shape, k, seed, dtype):
    """Seeded label / pred [H,W,D] with ~90 % background; ids >= k in both, negative ids in an int32 label."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    label = np.zeros(n, np.int64)
    pred = np.zeros(n, np.int64)
    fg = rng.random(n) < 0.1
    label[fg] = rng.integers(0, k + 3, int(fg.sum()))
    pfg = rng.random(n) < 0.1
    pred[pfg] = rng.integers(0, k + 3, int(pfg.sum()))
    both = fg & (rng.random(n) < 0.5)
    pred[both] = label[both]
    far = rng.random(n) < 0.01
    pred[far] = 255
    if dtype == np.int32:
        label[rng.random(n) < 0.01] = -1
        label[rng.random(n) < 0.005] = -2 ** 31
        label[rng.random(n) < 0.005] = 70000
    else:
        label[rng.random(n) < 0.01] = 255
    return label.astype(dtype).reshape(shape), pred.astype(np.uint8).reshape(shape)


def _label_view(label_hwd, layout, device):
    """The [D,H,W] view of the label in one of the three storage orders (values as ``label_hwd``)."""
    if layout == "zfast":                                   # the loader's C-ordered [H,W,D] array, read in place
        t = torch.from_numpy(np.ascontiguousarray(label_hwd)).to(device).permute(2, 0, 1)
        assert t.stride(0) == 1 or t.shape[0] == 1
    elif layout == "yfast":                                 # the same array in Fortran order: what cfun_amd.nifti.load returns
        t = torch.from_numpy(np.ascontiguousarray(label_hwd.transpose(2, 1, 0))).to(device).permute(0, 2, 1)
        assert t.stride(1) == 1 or t.shape[1] == 1
    else:                                                   # dense [D,H,W]: sample.load_image_gt's labels
        t = torch.from_numpy(np.ascontiguousarray(label_hwd.transpose(2, 0, 1))).to(device)
        assert t.is_contiguous()
    return t


def check_counts_case(device, label_hwd, pred_hwd, k, layout):
    from cfun_amd import evaluate
    pred = torch.from_numpy(np.ascontiguousarray(pred_hwd.transpose(2, 0, 1))).to(device)
    counts = evaluate.seg_confusion(pred, _label_view(label_hwd, layout, device), k)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (k + 1, k + 1)
    want = er.confusion(pred_hwd, label_hwd, k)
    got = counts.cpu()
    assert torch.equal(got, torch.from_numpy(want)), "k %d %s %s:\n%s\n%s" % (k, layout, label_hwd.dtype, got, want)
    assert int(got.sum()) == label_hwd.size
    return got


def check_counts_shape(device, shape):
    seed = 1000 + shape[0] * 7 + shape[2]
    for dtype in (np.int32, np.uint8):
        label, pred = _volumes(shape, 8, seed, dtype)
        for layout in LAYOUTS:
            check_counts_case(device, label, pred, 8, layout)
    for k in (3, 2, 15):
        label, pred = _volumes(shape, k, seed + k, np.int32)
        check_counts_case(device, label, pred, k, "zfast")
        label, pred = _volumes(shape, k, seed + k, np.uint8)
        check_counts_case(device, label, pred, k, "dense")
        check_counts_case(device, label, pred, k, "yfast")


def check_strided_sources(device):
    """A label that is a slice of a larger array (storage offset, no unit stride on any axis) and the same label z-fastest."""
    from cfun_amd import evaluate
    rng = np.random.default_rng(5)
    big = np.where(rng.random((25, 60, 100)) < 0.15, rng.integers(-1, 11, (25, 60, 100)), 0).astype(np.int32)
    view = torch.from_numpy(big).to(device)[3:-2, ::2, 1::3]                 # [D,H,W] = (20, 30, 33)
    assert view.storage_offset() > 0 and all(s != 1 for s in view.stride())
    lab = np.ascontiguousarray(big[3:-2, ::2, 1::3])
    d, h, w = lab.shape
    pred = np.where(rng.random(lab.shape) < 0.15, rng.integers(0, 11, lab.shape), 0).astype(np.uint8)
    tp = torch.from_numpy(pred).to(device)
    c_slice = evaluate.seg_confusion(tp, view, 8)
    zfast = torch.from_numpy(np.ascontiguousarray(lab.transpose(1, 2, 0))).to(device).permute(2, 0, 1)
    assert zfast.stride(0) == 1
    c_z = evaluate.seg_confusion(tp, zfast, 8)
    assert torch.equal(c_slice, c_z)
    assert torch.equal(c_z.cpu(), torch.from_numpy(er.confusion(pred, lab, 8))) and int(c_z.sum()) == d * h * w
    # a dtype the kernel does not read (int16, float) is converted on the device; the view's values are what counts
    assert torch.equal(evaluate.seg_confusion(tp, view.to(torch.int16), 8), c_z)
    assert torch.equal(evaluate.seg_confusion(tp, zfast.to(torch.float64), 8), c_z)


def check_edge_cases(device):
    from cfun_amd import _lib, evaluate
    shape = (64, 64, 64)
    zeros = np.zeros(shape, np.uint8)
    for layout in LAYOUTS:
        got = check_counts_case(device, zeros.astype(np.int32), zeros, 8, layout)
        assert int(got[0, 0]) == 262144
        got = check_counts_case(device, zeros + 3, zeros + 3, 8, layout)         # one cell past 2^16
        assert int(got[3, 3]) == 262144 and int((got != 0).sum()) == 1
    for dims in ((0, 5, 7), (5, 0, 7), (5, 7, 0)):
        pred = torch.zeros(dims, dtype=torch.uint8, device=device)
        counts = evaluate.seg_confusion(pred, torch.zeros(dims, dtype=torch.int32, device=device), 8)
        assert tuple(counts.shape) == (9, 9) and not counts.cpu().any()
    # rejected by the C entry with nothing launched: counts keeps its sentinel
    lib = _lib.load()
    pred = torch.zeros((2, 3, 4), dtype=torch.uint8, device=device)
    label = torch.zeros((2, 3, 4), dtype=torch.int32, device=device)
    counts = torch.full((17, 17), -7, dtype=torch.int64, device=device)
    ws = _lib.workspace(lib.cfun_seg_confusion_workspace_bytes(2, 3, 4, 8), pred)
    i64, i32 = C.c_int64 * 3, C.c_int32 * 3
    for dims, k in (((2048, 1024, 1024), 8), ((1, 1 << 16, 1 << 15), 8), ((2, 3, 4), 0), ((2, 3, 4), 16), ((2, -3, 4), 8)):
        rc = lib.cfun_seg_confusion(_lib.ptr(pred), _lib.ptr(label), 1, i64(12, 4, 1), i32(*dims), k, _lib.ptr(counts), _lib.ptr(ws),
                                    ws.numel(), _lib.stream(pred))
        assert rc == -1, (dims, k, rc)
        assert lib.cfun_seg_confusion_workspace_bytes(*dims, k) == 0
    rc = lib.cfun_seg_confusion(_lib.ptr(pred), _lib.ptr(label), 2, i64(12, 4, 1), i32(2, 3, 4), 8, _lib.ptr(counts), _lib.ptr(ws),
                                ws.numel(), _lib.stream(pred))
    assert rc == -1
    rc = lib.cfun_seg_confusion(_lib.ptr(pred), _lib.ptr(label), 1, i64(12, 4, 1), i32(2, 3, 4), 8, _lib.ptr(counts), _lib.ptr(ws),
                                0, _lib.stream(pred))
    assert rc == -2                                                              # workspace too small
    assert bool((counts.cpu() == -7).all())
    assert lib.cfun_seg_confusion_workspace_bytes((1 << 15) - 1, 1 << 8, 1 << 8, 15) == 1536 * 256 * 4     # the grid's cap


def check_wrapper_preconditions(device):
    from cfun_amd import _lib, evaluate
    pred = torch.zeros((4, 5, 6), dtype=torch.uint8, device=device)
    label = torch.zeros((4, 5, 6), dtype=torch.int32, device=device)
    with pytest.raises(ValueError, match="differ in shape"):
        evaluate.seg_confusion(pred, label[:, :, :5], 8)
    with pytest.raises(ValueError, match="differ in shape"):
        evaluate.seg_confusion(pred[0], label[0], 8)
    with pytest.raises(ValueError, match="uint8"):
        evaluate.seg_confusion(label, label, 8)
    for k in (0, 16, -1):
        with pytest.raises(ValueError, match="num_classes"):
            evaluate.seg_confusion(pred, label, k)
    huge = torch.zeros(1, dtype=torch.uint8, device=device).expand(2048, 1024, 1024)        # a view: nothing is allocated
    with pytest.raises(ValueError, match=r"2\^31"):
        evaluate.seg_confusion(huge, huge, 8)
    with pytest.raises(RuntimeError, match="contiguous"):
        evaluate.seg_confusion(pred.permute(2, 1, 0).contiguous().permute(2, 1, 0), label, 8)
    if not _lib.is_emulator():
        with pytest.raises(RuntimeError, match="CPU tensor"):
            evaluate.seg_confusion(pred.cpu(), label.cpu(), 8)


def check_scores_golden(device):
    """SegScores against the reference's own compute_per_class_mask_iou / compute_mask_iou, both trees."""
    from cfun_amd import evaluate
    g = load_golden("eval_iou")
    seen_zero = seen_one = False
    for tag in [str(t) for t in g["tags"]]:
        label, pred, k = g[tag + "_label"], g[tag + "_pred"], int(g[tag + "_k"])
        assert label.size < 2 ** 24
        tp = torch.from_numpy(np.ascontiguousarray(pred.transpose(2, 0, 1))).to(device)
        counts = evaluate.seg_confusion(tp, torch.from_numpy(label).to(device).permute(2, 0, 1), k)
        s = evaluate.SegScores(counts)
        assert np.array_equal(s.counts, er.confusion(pred, label, k)) and s.counts.dtype == np.int64
        assert s.per_class_iou.dtype == s.dice.dtype == np.float64 and s.per_class_iou.shape == s.dice.shape == (k - 1,)
        for tree in ("main", "lits"):
            want = g["%s_%s_per_class" % (tag, tree)]
            np.testing.assert_allclose(s.per_class_iou, want, rtol=RTOL, atol=0, err_msg=tag)
            assert (s.per_class_iou[want == 0] == 0).all()
            np.testing.assert_allclose(s.mask_iou, g["%s_%s_mask" % (tag, tree)], rtol=RTOL, atol=0, err_msg=tag)
            seen_zero |= bool((want == 0).any())
            seen_one |= bool((want > 0.999).all())
        np.testing.assert_allclose(s.per_class_iou, er.per_class_iou(s.counts), rtol=1e-15, atol=0)
        np.testing.assert_allclose(s.dice, er.dice(s.counts), rtol=1e-15, atol=0)
        np.testing.assert_allclose(s.mask_iou, er.mask_iou(s.counts), rtol=1e-15, atol=0)
        assert ((s.dice == 0) == (s.per_class_iou == 0)).all() and (s.dice >= s.per_class_iou).all()
    assert seen_zero and seen_one                      # the fixture holds an absent class and the perfect match


# ------------------------------------------------------------------------------------------------- detect_original / run_test
SRC = (40, 48, 20)                                     # the loader's [H,W,D]: not the network's size
AFFINE = np.array([[0.0, -1.25, 0.0, 30.0], [0.8, 0.0, 0.0, -12.0], [0.0, 0.0, 2.5, 7.0], [0.0, 0.0, 0.0, 1.0]])


def _net(device, cfg, max_instances):
    """The network of module_cases.check_inference_vs_oracle: seed 0, a decisive tie-free class head, no confidence filter."""
    from cfun_amd import step
    torch.manual_seed(0)
    cfg.DETECTION_MIN_CONFIDENCE = 0.0
    cfg.DETECTION_MAX_INSTANCES = max_instances
    net = step.CFUNHotPath(cfg).to(device)
    with torch.no_grad():
        net.classifier.linear_class.weight.mul_(40.0)
        net.classifier.linear_bbox.weight.mul_(20.0)
    return net


def _record_inference(net):
    """Keep what predict_inference returned, so that the host-side un-mold can be redone from the same detections."""
    seen = []
    orig = net.predict_inference

    def recording(*args, **kw):
        out = orig(*args, **kw)
        seen.append(out)
        return out
    net.predict_inference = recording
    return seen


def _case_arrays(seed, k):
    rng = np.random.default_rng(seed)
    image = rng.normal(100.0, 300.0, SRC).astype(np.float32)
    label = np.zeros(SRC, np.int32)
    label[6:34, 8:40, 3:17] = rng.integers(0, k, (28, 32, 14))
    return image, label


def _edges_numpy(m, roi, value=10):
    """heart_main.py:336-348 with the indices clipped to dim - 1."""
    lim = [m.shape[0] - 1, m.shape[1] - 1, m.shape[2] - 1]
    y1, x1, z1, y2, x2, z2 = [min(max(int(v), 0), lim[i % 3]) for i, v in enumerate(roi)]
    m[y1, x1:x2, z1] = value
    m[y1, x1:x2, z2] = value
    m[y2, x1:x2, z1] = value
    m[y2, x1:x2, z2] = value
    m[y1:y2, x1, z1] = value
    m[y1:y2, x2, z1] = value
    m[y1:y2, x1, z2] = value
    m[y1:y2, x2, z2] = value
    m[y1, x1, z1:z2] = value
    m[y1, x2, z1:z2] = value
    m[y2, x1, z1:z2] = value
    m[y2, x2, z1:z2] = value
    return m


def check_run_test_heart(device, tmp_path):
    """run_test on the tiny heart configuration: two cases (one a NIfTI pair, one arrays), saved with the box drawn."""
    import module_cases as mc
    from cfun_amd import evaluate, model, nifti
    cfg = mc.tiny_config("beginning")
    k = int(cfg.NUM_CLASSES)
    net = _net(device, cfg, 1)
    seen = _record_inference(net)
    h, w, d = SRC
    assert (h, w, d) != tuple(int(v) for v in cfg.IMAGE_SHAPE[:3])
    (img0, lab0), (img1, lab1) = _case_arrays(2, k), _case_arrays(4, k)      # (seeds whose volumes give a detection)
    p_img, p_lab = os.path.join(str(tmp_path), "ct_train_1001_image.nii"), os.path.join(str(tmp_path), "ct_train_1001_label.nii.gz")
    nifti.save(nifti.Nifti1Image(img0, AFFINE), p_img)
    nifti.save(nifti.Nifti1Image(lab0, AFFINE), p_lab)
    out_dir = os.path.join(str(tmp_path), "results")
    r = evaluate.run_test(net, [(p_img, p_lab), (img1, lab1, AFFINE, "second.nii"), (img1, lab1, AFFINE)], save_dir=out_dir,
                          draw_bbox=True, limit=2)
    assert len(seen) == 2 and len(r["results"]) == 2 and len(r["saved"]) == 2 and r["detect_time"] > 0
    assert r["per_class_ious"].shape == r["dice"].shape == (2, k - 1) and r["mask_ious"].shape == (2,)
    np.testing.assert_array_equal(r["mean"], r["per_class_ious"].mean(axis=0))
    np.testing.assert_array_equal(r["std"], r["per_class_ious"].std(axis=0))
    assert r["mean"].shape == r["std"].shape == (k - 1,) and r["total_mean"] == r["per_class_ious"].mean()
    assert not r["results"][0]["empty"], "test setup: no detection on the first case"
    for i, (image, label, name) in enumerate(((img0, lab0, "ct_train_1001_image.nii"), (img1, lab1, "second.nii"))):
        res = r["results"][i]
        md = res["mask_device"]
        assert md.dtype == torch.uint8 and tuple(md.shape) == (d, h, w) and md.device.type == torch.device(device).type
        det, masks = seen[i]
        _, _, windows = net.mold_inputs([torch.from_numpy(image)[..., None]])
        if res["empty"]:
            host = np.zeros(SRC, np.int64)
        else:                                     # the existing un-mold, given the ORIGINAL shape, on the same detections
            rois, ids, scores, host = model.unmold_detections(det[0], masks[0].permute(0, 2, 3, 4, 1).contiguous(), [1, d, h, w],
                                                              tuple(float(v) for v in windows[0]))
            np.testing.assert_array_equal(res["rois"], rois)
            np.testing.assert_array_equal(res["class_ids"], ids)
            np.testing.assert_array_equal(res["scores"], scores)
            assert host.any()
        assert host.shape == SRC and np.array_equal(md.permute(1, 2, 0).cpu().numpy(), host)
        counts = er.confusion(host, label, k)
        np.testing.assert_allclose(r["per_class_ious"][i], er.per_class_iou(counts), rtol=1e-15, atol=0)
        np.testing.assert_allclose(r["dice"][i], er.dice(counts), rtol=1e-15, atol=0)
        np.testing.assert_allclose(r["mask_ious"][i], er.mask_iou(counts), rtol=1e-15, atol=0)
        # the saved file: name rule, affine, dtype, the map with the twelve edges of rois[0]
        path = os.path.join(out_dir, str(r["per_class_ious"][i].mean()) + "_" + name)
        assert r["saved"][i] == path and os.path.exists(path)
        back = nifti.load(path)
        want = host.astype(np.int32)
        if not res["empty"]:
            want = _edges_numpy(want, res["rois"][0])
            assert (want == 10).any()
        data = back.get_data()
        assert data.dtype == np.int32 and np.array_equal(data, want)
        np.testing.assert_allclose(back.affine, AFFINE, rtol=0, atol=1e-6)
    # a box that touches the far face on every axis: clipped, where the reference raises an IndexError
    m = torch.zeros(SRC, dtype=torch.uint8, device=device)
    evaluate._draw_box_edges(m, (0, 0, 0, h, w, d))
    assert np.array_equal(m.cpu().numpy(), _edges_numpy(np.zeros(SRC, np.uint8), (0, 0, 0, h, w, d)))
    with pytest.raises(IndexError):
        np.zeros(SRC)[h, 0:w, 0] = 10
    # no detection: zeros and empty=True (the reference crashes there)
    cfg.DETECTION_MIN_CONFIDENCE = 1.5
    res = evaluate.detect_original(net, torch.from_numpy(img0)[..., None])
    assert res["empty"] is True and res["rois"].shape == (0, 6) and tuple(res["mask_device"].shape) == (d, h, w)
    assert res["mask_device"].dtype == torch.uint8 and not res["mask_device"].cpu().any()
    r0 = evaluate.run_test(net, [(img0, lab0, AFFINE)])
    assert r0["per_class_ious"].shape == (1, k - 1) and not r0["per_class_ious"].any() and r0["saved"] == []


def check_run_test_lits(device, tmp_path):
    """The fork's path: rois clipped, every box filled with 100, order-0 resize to the NIfTI's own shape, uint8."""
    import module_cases as mc
    from oracle import cfun_oracle as orc
    from cfun_amd import evaluate, model, nifti
    cfg = mc.tiny_lits_config("together", max_dim=64, min_dim=32)
    cfg.PAD_IMAGE_SHAPE = [80, 80, 40]
    k = int(cfg.NUM_CLASSES)
    net = _net(device, cfg, 2)
    seen = _record_inference(net)
    h, w, d = SRC
    rng = np.random.default_rng(9)
    image = rng.normal(0.0, 200.0, SRC).astype(np.float32)
    label = np.zeros(SRC, np.int32)
    label[5:30, 10:44, 2:15] = rng.integers(0, k, (25, 34, 13))
    save_shape = (44, 52, 22)
    out_dir = os.path.join(str(tmp_path), "lits")
    r = evaluate.run_test(net, [(image, label, AFFINE, "liver_7.nii.gz", save_shape)], save_dir=out_dir, draw_bbox=True)
    res = r["results"][0]
    assert not res["empty"], "test setup: no detection"
    det, masks = seen[0]
    _, _, windows = net.mold_inputs([torch.from_numpy(image)])
    rois, ids, scores, host = model.unmold_detections_overlap(det[0], masks[0].permute(0, 2, 3, 4, 1).contiguous(), [1, d, h, w],
                                                              tuple(float(v) for v in windows[0]))
    assert np.array_equal(res["mask_device"].permute(1, 2, 0).cpu().numpy(), host)
    rois = rois.clip(min=0)                                                   # LiTS_main.py:319-323
    rois[:, 3], rois[:, 4], rois[:, 5] = rois[:, 3].clip(max=h - 1), rois[:, 4].clip(max=w - 1), rois[:, 5].clip(max=d - 1)
    np.testing.assert_array_equal(res["rois"], rois.astype(np.int32))
    np.testing.assert_allclose(r["per_class_ious"][0], er.per_class_iou(er.confusion(host, label, k)), rtol=1e-15, atol=0)
    assert r["per_class_ious"].shape == (1, k - 1)
    want = host.copy()
    for y1, x1, z1, y2, x2, z2 in rois.tolist():
        want[y1:y2, x1:x2, z1:z2] = 100
    assert (want == 100).any()
    want = np.round(orc.skimage_resize(want, save_shape, 0)).astype(np.uint8)
    path = os.path.join(out_dir, str(r["per_class_ious"][0].mean()) + "_liver_7.nii.gz")
    assert r["saved"] == [path]
    back = nifti.load(path)
    assert back.get_data().dtype == np.uint8 and back.get_data().shape == save_shape and np.array_equal(back.get_data(), want)
    np.testing.assert_allclose(back.affine, AFFINE, rtol=0, atol=1e-6)
    # the detector-only stage: zeros, no mask scores
    cfg.STAGE = "beginning"
    assert net.detector_phase_only
    r = evaluate.run_test(net, [(image, label, AFFINE)])
    assert r["per_class_ious"].shape == (0, k - 1) and not r["results"][0]["mask_device"].cpu().any()


# ------------------------------------------------------------------------------------------------------------ accounting
def eval_header_symbols():
    """The same parse as test_abi.header_symbols, on include/cfun_eval.h."""
    txt = open(os.path.join(ROOT, "include", "cfun_eval.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(cfun_[a-z0-9_]+)\s*\(", txt)))


EVAL_NO_LAUNCH = {"cfun_seg_confusion_workspace_bytes": "host-side query: launches nothing, touches no device memory"}


def check_coverage(tier):
    from cfun_amd import _lib
    assert eval_header_symbols() == sorted(_lib.EVAL_EXPORTS)
    for other in (_lib.EXPORTS, _lib.SAMPLE_EXPORTS, _lib.TILE_EXPORTS):
        assert not set(_lib.EVAL_EXPORTS) & set(other)
    missed = sorted(set(_lib.EVAL_EXPORTS) - set(EVAL_NO_LAUNCH) - guard.SEEN[tier])
    assert not missed, "scoring entries that launch work but never ran under guard: %s" % missed
