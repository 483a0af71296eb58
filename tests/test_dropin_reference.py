"""CPU tier: the drop-in recipe of INTEGRATION.md held to the reference's own classes, from recorded fixtures.

``tests/golden/gen_golden.py dropin`` ran the reference's ``model.FPN``, ``model.Mask``, ``model.proposal_layer`` and
``MaskRCNN`` (closed-form weights, a shrunken configuration) and recorded, at each module-level swap of INTEGRATION.md
section 1, what the reference hands the swapped name and what it gets back -- the backbone stages' outputs, RoI_Align's
and the U-Net's inputs and outputs, the arguments and result of ``utils.non_max_suppression`` -- plus what the classes
return and the whole training step's outputs, losses and parameter gradients (tests/golden/dropin_*.npz).  cfun_amd's
drop-ins must reproduce every recorded interface, with the same state-dict keys, and the product's own assembly of them
must reproduce the classes' results.  The kernels run through the HIP emulator build (CPU tensors)."""
import numpy as np
import pytest
import torch

from conftest import golden_state_dict, load_golden


@pytest.fixture()
def emu_direct(emu, monkeypatch):
    monkeypatch.setenv("CFUN_CONV_ALGO", "direct")     # module-sized graphs: direct kernels on the fiber emulator
    return emu


def _tiny_cfg(stage="beginning"):
    """gen_golden.dropin_cfg, built from cfun_amd.config."""
    from cfun_amd import config
    cls = type("DropinHeart", (config.HeartConfig,), dict(
        IMAGE_MAX_DIM=32, IMAGE_MIN_DIM=16, MASK_POOL_SIZE=[32, 32, 32], POOL_SIZE=[4, 4, 4], UNET_MASK_BRANCH_CHANNEL=4,
        TOP_DOWN_PYRAMID_SIZE=16, RPN_CONV_CHANNELS=16, FPN_CLASSIFY_FC_LAYERS_SIZE=16, RPN_ANCHOR_SCALES=(16, 32)))
    return cls(stage)


def _close_sub(t, g, name, tol):
    """A 5-D result against its recorded strided subsample (max-abs) and fp64 |.|-checksum (relative)."""
    a = t.detach().cpu().numpy()
    assert a.shape[:2] == g[name + "_sub"].shape[:2], name
    assert float(np.abs(a[:, :, ::4, ::4, ::4] - g[name + "_sub"]).max()) < tol, name
    ref = float(g[name + "_sum"][1])
    assert abs(np.abs(a).astype(np.float64).sum() - ref) <= 1e-4 * ref, name


def test_fpn_with_dropin_backbone(emu_direct):
    """cfun_amd.backbone.P3D19's stages take the reference FPN's state-dict keys and return what the reference stages
    returned inside model.FPN; the FPN over them gives the reference's P2 / P3."""
    from cfun_amd import backbone as my_backbone
    from cfun_amd import model as my_model
    g = load_golden("dropin_fpn")
    cfg = _tiny_cfg()
    fpn = my_model.FPN(*my_backbone.P3D19(config=cfg).stages(), out_channels=16, config=cfg)
    fpn.load_state_dict(golden_state_dict(g), strict=True)          # identical keys and shapes
    fpn.eval()
    x = torch.from_numpy(g["x"])
    with torch.no_grad():
        h = x
        for name in ("c1", "c2", "c3"):
            h = getattr(fpn, name.upper())(h)
            np.testing.assert_allclose(h.numpy(), g[name], rtol=1e-4, atol=2e-5, err_msg=name)
        mp2, mp3 = fpn(x)
    np.testing.assert_allclose(mp2.numpy(), g["p2"], rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(mp3.numpy(), g["p3"], rtol=1e-4, atol=2e-5)


def test_mask_head_with_dropin_unet_and_roi_align(emu_direct):
    """``RoI_Align`` and ``mask_branch.Modified3DUNet`` of cfun_amd on the arguments the reference's model.Mask passed its
    own, same weights, eval mode; and model.Mask built from them end to end."""
    from cfun_amd import mask_branch as my_mask_branch
    from cfun_amd import model as my_model
    g = load_golden("dropin_mask")
    sd = golden_state_dict(g)
    with torch.no_grad():
        aligned = my_model.RoI_Align(torch.from_numpy(g["align_fm"]), [int(v) for v in g["align_pool"]],
                                     torch.from_numpy(g["align_boxes"]))
        np.testing.assert_allclose(aligned.numpy(), g["align_out"], rtol=0, atol=1e-5)
        unet = my_mask_branch.Modified3DUNet(1, 8, "beginning", 4)
        unet.load_state_dict({k[len("modified_u_net."):]: v for k, v in sd.items() if k.startswith("modified_u_net.")},
                             strict=True)
        unet.eval()
        _close_sub(unet(torch.from_numpy(g["unet_in"])), g, "unet_out", 1e-3)
        m_mask = my_model.Mask(1, [32, 32, 32], 8, 4, "beginning")
        m_mask.load_state_dict(sd, strict=True)
        m_mask.eval()
        img = torch.from_numpy(g["img"])
        m_logits, m_probs = m_mask([img, img], torch.from_numpy(g["rois"]))
    assert tuple(m_logits.shape) == (2, 8, 32, 32, 32)
    _close_sub(m_logits, g, "logits", 1e-3)
    _close_sub(m_probs, g, "probs", 5e-4)


def test_proposal_layer_with_dropin_nms(emu_direct):
    """cfun_amd.utils.non_max_suppression returns, on the arguments the reference's model.proposal_layer passed to
    ``utils.non_max_suppression``, exactly what the reference's returned; the product's proposal_layer gives its proposals."""
    from cfun_amd import model as my_model
    from cfun_amd import utils as my_utils
    g = load_golden("dropin_proposal")
    thr, mx = g["nms_cfg"]
    keep = my_utils.non_max_suppression(g["nms_boxes"].copy(), g["nms_scores"].copy(), float(thr), int(mx))
    np.testing.assert_array_equal(np.asarray(keep), g["nms_keep"])
    got = my_model.proposal_layer([torch.from_numpy(g["probs"]), torch.from_numpy(g["bbox"])], proposal_count=12,
                                  nms_threshold=0.7, anchors=torch.from_numpy(g["anchors"]), config=_tiny_cfg())
    assert tuple(got.shape) == g["rois"].shape          # same number of proposals = same NMS decisions
    np.testing.assert_allclose(got.numpy(), g["rois"], rtol=0, atol=2e-6)


def test_whole_maskrcnn_training_step_with_all_dropins(emu_direct):
    """The reference's OWN ``MaskRCNN`` training step -- build(), predict('training'), detection_target_layer,
    compute_losses and backward (model.py:1259-1304, 1391-1514, 984-1000) -- recorded with its randperm draws and
    Dropout3d masks, against the product's step assembled from ALL FOUR drop-ins (``backbone``, ``mask_branch``,
    ``RoI_Align``, non-max suppression) on the same weights and inputs: the nine outputs, the six losses and the parameter
    gradients must agree."""
    from cfun_amd import step
    g = load_golden("dropin_step")
    cfg = _tiny_cfg()
    cfg.MASK_SHAPE = cfg.MINI_MASK_SHAPE = (32, 32, 32)
    cfg.POST_NMS_ROIS_TRAINING = 64
    net = step.CFUNHotPath(cfg)
    net.load_state_dict(golden_state_dict(g), strict=True)
    with torch.no_grad():                       # as the fixture: proposals near their anchors, so that positives exist
        net.rpn.conv_bbox.weight.mul_(0.05)
    unet = net.mask.modified_u_net
    assert type(unet).__module__.startswith("cfun_amd") and type(net.fpn.C1).__module__.startswith("cfun_amd")
    unet.dropout_masks = [torch.from_numpy(g["drop%d" % i]) for i in range(5)]
    perms = tuple(torch.from_numpy(g[k]) for k in sorted(k for k in g if k.startswith("randperm")))
    out, losses, total = step.training_step_full(
        net, torch.from_numpy(g["image"])[None, None], torch.from_numpy(g["gt_class_ids"][0].astype(np.int64)),
        torch.from_numpy(g["gt_boxes"][0]), torch.from_numpy(g["gt_masks_labels"]), torch.from_numpy(g["rpn_match"]),
        torch.from_numpy(g["rpn_bbox_t"]), perms=perms)
    assert out["p_rois"].shape[0] == int(g["n_pos"]) > 0 and out["rois"].shape[0] == int(g["n_rois"])

    def close(a, name, tol):
        b = g[name]
        a = a.detach().cpu().double().numpy()
        assert a.shape == b.shape, name
        assert float(np.abs(a - b).max()) <= tol * max(1.0, float(np.abs(b).max())), name
    close(out["rpn_class_logits"], "rpn_class_logits", 2e-5)
    close(out["rpn_bbox"], "rpn_pred_bbox", 2e-5)
    # GT boxes are 7 copies of one box: the assigned class is an arg-max tie, only "positive or not" is defined
    np.testing.assert_array_equal((out["target_class_ids"] > 0).cpu().numpy(), g["target_class_ids"] > 0)
    close(out["target_deltas"], "target_deltas", 2e-5)
    np.testing.assert_array_equal(out["mask_labels"].cpu().numpy(), g["target_mask_labels"])
    close(out["mrcnn_class_logits"], "mrcnn_class_logits", 2e-5)
    close(out["mrcnn_bbox"], "mrcnn_bbox", 2e-5)
    _close_sub(out["mrcnn_mask_logits"].permute(0, 4, 1, 2, 3), g, "mask_logits", 1e-3)
    _close_sub(out["mrcnn_mask"].permute(0, 4, 1, 2, 3), g, "mask_probs", 1e-3)
    for a, b in zip(losses, g["losses"]):
        assert abs(float(a.detach()) - float(b)) <= 1e-4 * max(abs(float(b)), 1e-3)
    assert abs(float(total.detach()) - float(g["total"])) <= 1e-4 * abs(float(g["total"]))
    params = dict(net.named_parameters())
    checked = 0
    for key in g:
        if not key.startswith(("grad:", "grad4:")):
            continue
        k = key.split(":", 1)[1]
        got = params[k].grad
        assert got is not None, k
        got = got.cpu().numpy()
        if key.startswith("grad4:"):
            got = got[::4, ::4]
        ref = g[key]
        e = float(np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-30))
        assert e < (6e-2 if k.startswith("mask.") else 1e-3), (k, e)     # (U-Net: the 32^3 toy configuration's fp32 noise floor)
        checked += 1
    assert checked >= 90
