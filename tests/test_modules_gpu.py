"""GPU tier: module-level parity on the real library -- golden vectors of the reference, oracle comparison
of whole training steps, state-dict contract."""
import numpy as np
import pytest
import torch

import module_cases as mc
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["unet_beginning_eval", "unet_beginning_train", "unet_finetune_train",
                                  "unet_lits_eval"])
def test_unet_golden(gpu, name):
    mc.check_unet_golden(gpu, name)


def test_fpn_rpn_golden(gpu):
    mc.check_fpn_rpn_golden(gpu)


def test_proposal_layer_golden(gpu):
    mc.check_proposal_layer_golden(gpu)


def test_pyramid_roi_align_golden(gpu):
    mc.check_pyramid_roi_align_golden(gpu)


def test_classifier_golden(gpu):
    mc.check_classifier_golden(gpu)


def test_nms_dropin(gpu):
    mc.check_nms_dropin(gpu)


@pytest.mark.parametrize("stage", ["beginning", "finetune"])
def test_training_step_tiny_vs_oracle(gpu, stage):
    mc.check_training_step_vs_oracle(gpu, mc.tiny_config(stage))


def test_training_step_cfg0_vs_oracle(gpu):
    """BASELINE.json configs[0] shape (64x64x32, b = 20, 96^3 crops, 'beginning'), 2 positive RoIs:
    the full hot path forward + losses + backward against the oracle on the host."""
    from cfun_amd import config
    torch.set_num_threads(max(1, torch.get_num_threads()))
    mc.check_training_step_vs_oracle(gpu, config.heart_config("beginning", 64, 64, 32), n_pos=2)


def test_training_step_finetune_b20_vs_oracle(gpu):
    """The BENCHMARKED module configuration as a step: heart shapes with b = 20 in stage 'finetune' -- 96^3 crops ->
    192^3 masks, i.e. the exact kernel instantiations bench.py runs (40 -> 40 NSUB = 3 and the REM-quad tiles,
    k_wgrad_fused, the per-RoI Dropout3d-sparse conv pairs, the zero-copy level-1 concat, the parity-folded up-convs
    and 5^3 conv, the fused CE + Sobel-edge backward at 192^3) -- forward, 6 losses, backward against the oracle on the
    host, gradients held to the fp64-measured bound.  64x64x32 volume (the FPN / RPN part is size-generic and covered at
    full size by test_cfg2_full_size_step_properties); 1 positive + 2 negative RoIs keep the fp64 oracle to ~25 GB."""
    from cfun_amd import config
    rep = []
    r = mc.check_training_step_vs_oracle(gpu, config.heart_config("finetune", 64, 64, 32), n_pos=1, report=rep)
    for k, e_hip, e_ref in rep:
        print("%-60s relL2(HIP,fp64) %.2e  relL2(fp32,fp64) %.2e" % (k, e_hip, e_ref))
    assert not r["bad"], "\n".join(r["bad"])
    assert r["losses"][5] > 0.0        # the edge loss is live


@pytest.mark.parametrize("which", ["tiny_wino_finetune", "b20_finetune"])
def test_weight_scope_step_bit_identical(gpu, which):
    """ops.WeightScope on the real kernels: the steps whose weight operands come from one cfun_weight_prepare launch per
    scope (packs, Winograd transforms, stride-2 folds, gathered Dropout3d slices) equal the recorded first step bit for
    bit -- at the benchmarked channel counts too (b = 20: 1-D and 2-D Winograd operands, the parity-folded up-convs)."""
    from cfun_amd import config
    cfg = mc.tiny_wino_config("finetune") if which == "tiny_wino_finetune" else config.heart_config("finetune", 64, 64, 32)
    mc.check_weight_scope_bit_identical(gpu, cfg, steps=3)


def test_two_models_alternating(gpu):
    mc.check_two_models_alternating(gpu)


def test_step_bit_reproducible_under_allocator_churn(gpu):
    """The two-stream step repeated under allocator churn, bit for bit."""
    mc.check_step_bit_reproducible_under_churn(gpu, runs=8)


CFG2_PEAK_GB_MAX = 14.0      # measured on the round-6 tree: 9.2 GB (the step incl. the weight-gradient stream's record_stream holds)


def test_cfg2_full_size_step_properties(gpu, monkeypatch):
    """BASELINE.json configs[2] at FULL size (256x256x128, 'finetune', b = 20, 4 + 8 injected RoIs, 96^3 -> 192^3) --
    the step bench.py times: the heads are not skipped, all six losses and the gradients of all 95 trainable tensors are
    finite and non-zero, the step is bit-reproducible with fixed Dropout3d masks, and the value path (MFMA kernels)
    agrees with the generic direct kernels (CFUN_CONV_ALGO=direct) on every loss to 1e-4 relative.  The tensors held here only
    to finite / non-zero / reproducible (VERDICT.md weak spot 2) get their value check per layer: tests/test_product_shapes_gpu.py
    replays every conv this step issues at its true shape against fp64."""
    from cfun_amd import config, step
    cfg = config.heart_config("finetune", 256, 256, 128)
    torch.manual_seed(0)
    net = step.CFUNHotPath(cfg).to(gpu)
    s = step.synthetic_inputs(cfg, gpu, 0)
    assert s["p_rois"].shape[0] == 4 and s["n_rois"].shape[0] == 8
    b = cfg.UNET_MASK_BRANCH_CHANNEL
    gen = torch.Generator().manual_seed(1)
    net.mask.modified_u_net.dropout_masks = [torch.empty(4, c).bernoulli_(0.4, generator=gen) / 0.4
                                             for c in (b, 2 * b, 4 * b, 8 * b, 16 * b)]

    def run():
        net.zero_grad(set_to_none=True)
        out, losses, total = step.training_step(net, s)
        torch.cuda.synchronize()
        return out, [float(l.detach()) for l in losses], {k: p.grad.clone() for k, p in net.named_parameters()
                                                          if p.grad is not None}
    torch.cuda.reset_peak_memory_stats()
    out, l1, g1 = run()
    # (record_stream on the activations the weight-gradient stream reads delays their reuse; the step's peak is
    # pinned so that a change which starts holding whole levels longer shows up here -- 288 GB per GPU is not a licence)
    peak_gb = torch.cuda.max_memory_allocated() / 1e9
    print("cfg2 step peak memory: %.1f GB" % peak_gb)
    assert peak_gb < CFG2_PEAK_GB_MAX, peak_gb
    assert tuple(out["mrcnn_mask_logits"].shape) == (4, 192, 192, 192, 8) and tuple(out["mrcnn_class_logits"].shape) == (12, 2)
    assert all(np.isfinite(v) and v > 0 for v in l1), l1
    trainable = [k for k, p in net.named_parameters() if p.requires_grad]
    assert len(trainable) == 95 and sorted(g1) == sorted(trainable)
    for k, v in g1.items():
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0, k
    del out
    _, l2, g2 = run()
    assert l1 == l2                                                       # bit-identical losses
    # every gradient repeats bit for bit -- since round 5 also those that pass through RoIAlign's backward (a gather over the
    # RoIs in index order; rounds 1-4 scattered with fp32 atomics and were held to 1e-5 here)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    del g2
    # NOT a self-comparison: the product's gradients at the benchmarked size against the mask head's fp64
    # gradients of exactly this step (tests/golden/grad_fp64_cfg2.npz: same seed-0 weights, volume, RoIs, seed-1 Dropout3d masks;
    # generated through the oracle on the host) under the measured bound 3 x (the reference fp32 arithmetic's own deviation) + 2e-5
    import sys
    sys.path.insert(0, ROOT)
    import bench
    ref64 = bench.load_grad_fp64(net, cfg, "cfg2")
    assert ref64 is not None, "tests/golden/grad_fp64_cfg2.npz does not belong to these weights (another torch build?)"
    assert len(ref64) == 27                 # every U-Net conv weight (round 6; rounds 4-5: four of them)
    for k, ref in ref64.items():
        e, floor = bench.grad_fp64_error(g1[k], ref), ref[2]
        bound = bench.GRAD_FP64_FACTOR * floor + bench.GRAD_FP64_FLOOR
        assert e <= bound, "%s: relL2(GPU, fp64) %.3e > 3 x %.3e + 2e-5" % (k, e, floor)
    monkeypatch.setenv("CFUN_CONV_ALGO", "direct")
    _, l3, g3 = run()
    for a, r in zip(l1, l3):
        assert abs(a - r) <= 1e-4 * abs(r), (l1, l3)
    # gradients: tight wherever no InstanceNorm + LeakyReLU lies downstream; the U-Net tensors above the last norm carry
    # the configuration's own fp32 noise floor (the reference's fp32 gradients are 2e-4 .. 7e-3 off its fp64 ones at
    # these shapes, measured per tensor by test_training_step_finetune_b20_vs_oracle) -- two fp32 evaluation orders
    # (MFMA tiles vs the direct kernel) differ by that much, so those are held to 5x that floor
    for k, tol in (("mask.modified_u_net.conv3d_l4.weight", 1e-4), ("mask.modified_u_net.out_upscale_conv.1.weight", 1e-4),
                   ("mask.modified_u_net.ds3_1x1_conv3d.weight", 1e-4), ("fpn.C1.0.weight", 1e-4),
                   ("rpn.conv_shared.weight", 1e-4), ("classifier.conv1.weight", 1e-4),
                   ("mask.modified_u_net.conv_norm_lrelu_l4.0.weight", 3e-3), ("mask.modified_u_net.conv3d_c1_1.weight", 3e-2),
                   ("mask.modified_u_net.norm_lrelu_conv_c5.2.weight", 3e-2)):
        e = float((g1[k] - g3[k]).norm() / g3[k].norm())
        assert e < tol, "%s: MFMA vs direct rel L2 %.3e" % (k, e)


def test_training_step_lits_shapes(gpu):
    """BASELINE.json configs[4] shapes (shrunk): P3D35, (5,7,7) stem, 3 classes, no dropout, non-cubic crops."""
    mc.check_training_step_vs_oracle(gpu, mc.tiny_lits_config())


def test_cfg1_forward_vs_oracle(gpu):
    """BASELINE.json configs[1]: 128x128x64 volume, P3D backbone + FPN + RPN + mask head forward ('beginning',
    b = 20, 96^3 crops, 2 RoIs) against the oracle."""
    from cfun_amd import config, step
    from oracle import cfun_oracle as orc
    cfg = config.heart_config("beginning", 128, 128, 64)
    torch.manual_seed(0)
    net = step.CFUNHotPath(cfg).to(gpu).eval()
    s = step.synthetic_inputs(cfg, gpu, 0)
    with torch.no_grad():
        p2, p3, logits, probs, bbox = net.backbone_rpn(s["image"])
        rois = net.proposals(probs, bbox, "inference")
        ml, mp = net.mask.forward_ndhwc(s["image"][0].permute(1, 2, 3, 0).contiguous(), s["p_rois"][:2])
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    img = s["image"].cpu()
    with torch.no_grad():
        rp2, rp3 = orc.fpn(img, sd)
        r2, r3 = orc.rpn(rp2, sd), orc.rpn(rp3, sd)
        rprobs = torch.cat([r2[1], r3[1]], dim=1)
        rbbox = torch.cat([r2[2], r3[2]], dim=1)
        rrois, _, _ = orc.proposal_layer(rprobs[0], rbbox[0], net.anchors.cpu(), cfg.POST_NMS_ROIS_INFERENCE, 0.7,
                                         cfg.image_dhw, cfg.PRE_NMS_LIMIT)
        rl, rp = orc.mask_head(img[0], s["p_rois"][:2].cpu(), sd, cfg.MASK_POOL_SIZE, "beginning")
    np.testing.assert_allclose(p2.cpu().permute(0, 4, 1, 2, 3).numpy(), rp2.numpy(), rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(bbox.cpu().numpy(), rbbox.numpy(), rtol=1e-4, atol=2e-5)
    assert rois.shape[1] == rrois.shape[0]
    np.testing.assert_allclose(rois[0].cpu().numpy(), rrois.numpy(), rtol=0, atol=1e-5)
    assert np.abs(ml.cpu().permute(0, 4, 1, 2, 3).numpy() - rl.numpy()).max() < 1e-3
    assert float((mp.cpu().permute(0, 4, 1, 2, 3).numpy().argmax(1) != rp.numpy().argmax(1)).mean()) <= 1e-4


def test_unet_b20_96_forward_properties(gpu):
    """Full-size mask head (b = 20, 96^3 -> 192^3, 'finetune'): size-independent properties --
    softmax rows sum to 1, eval is deterministic, batch entries are independent (InstanceNorm is per sample)."""
    from cfun_amd.mask_branch import Modified3DUNet
    torch.manual_seed(0)
    net = Modified3DUNet(1, 8, "finetune", 20).to(gpu).eval()
    x = torch.randn(2, 1, 96, 96, 96, device=gpu)
    with torch.no_grad():
        y = net(x)
        y1 = net(x[1:2])
        y_again = net(x)
    assert tuple(y.shape) == (2, 8, 192, 192, 192)
    assert torch.equal(y, y_again)
    assert float((y[1:2] - y1).abs().max()) < 1e-4
    from cfun_amd import ops
    p = ops.softmax_channels(y.permute(0, 2, 3, 4, 1))
    assert float((p.sum(-1) - 1).abs().max()) < 1e-5


def test_state_dict_contract(gpu):
    """220 entries with the reference's key names and shapes; strict load round-trip."""
    from cfun_amd import config, step
    g = load_golden("predict_cfg0")
    net = step.CFUNHotPath(config.heart_config("beginning", 64, 64, 32))
    sd = net.state_dict()
    ref = {str(k): tuple(int(v) for v in str(s).split(",") if v != "") for k, s in zip(g["sd_keys"], g["sd_shapes"])}
    assert set(sd) == set(ref)
    assert len(sd) == 220
    for k, v in sd.items():
        assert tuple(v.shape) == ref[k], k


def test_refine_detections_golden(gpu):
    mc.check_refine_detections_golden(gpu)


@pytest.mark.parametrize("stage", ["beginning", "finetune"])
def test_inference_vs_oracle(gpu, stage):
    r = mc.check_inference_vs_oracle(gpu, mc.tiny_config(stage), max_instances=3)
    assert r["n_det"] >= 1


def test_inference_lits_overlap_tile(gpu):
    """LiTS fork inference: P3D35 + 3-class heads, several detections un-molded with the overlap-tile average."""
    # 64x64x32: on the 32x32x16 volume the clipped proposals coincide and their class scores tie exactly
    r = mc.check_inference_vs_oracle(gpu, mc.tiny_lits_config("together", max_dim=64, min_dim=32), max_instances=3)
    assert r["n_det"] >= 2


def test_inference_cfg0(gpu):
    """predict('inference') at BASELINE configs[0] size (64x64x32, real channel counts) vs the oracle."""
    from cfun_amd import config
    # one instance: at this size several clipped proposals coincide, so lower-ranked scores tie exactly
    mc.check_inference_vs_oracle(gpu, config.heart_config("beginning", 64, 64, 32), max_instances=1)


def test_predict_cfg0_reference_golden(gpu):
    """Un-injected training step vs the reference's own cfg0 outputs (detection_target_layer on device included)."""
    mc.check_predict_cfg0_golden(gpu)


def test_detection_target_layer(gpu):
    mc.check_detection_target_layer(gpu)
    mc.check_detection_target_layer(gpu, lits=True)


def test_gradient_reducer_streams(gpu):
    """cfun_amd.dist.GradientReducer on the GPU (single-rank RCCL group): bucket views, hooks and the side-stream
    all-reduce leave exactly the gradients of a plain backward."""
    import os
    import torch.distributed as dist
    from cfun_amd import dist as cdist
    from cfun_amd import step
    import socket
    with socket.socket() as sock:               # a free port (a fixed one clashes on a shared box and fails the tier under -x)
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        cfg = mc.tiny_config("finetune")
        torch.manual_seed(0)
        net = step.CFUNHotPath(cfg).to(gpu)
        s = step.synthetic_inputs(cfg, gpu, 0)
        b = cfg.UNET_MASK_BRANCH_CHANNEL
        gen = torch.Generator().manual_seed(1)
        net.mask.modified_u_net.dropout_masks = [torch.empty(4, c).bernoulli_(0.4, generator=gen) / 0.4
                                                 for c in (b, 2 * b, 4 * b, 8 * b, 16 * b)]
        net.zero_grad(set_to_none=True)
        step.training_step(net, s)
        ref = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
        red = cdist.GradientReducer(net.parameters(), bucket_bytes=16 << 10, always_reduce=True)
        assert len(red.buckets) > 3
        from cfun_amd import ops
        for it in range(3):
            red.zero_grad()
            if it == 2:
                # third pass: the weight-gradient streams asleep while the step is enqueued -- the accumulation into the
                # buckets and the hooks' all-reduces (RCCL, on the communication stream) must still come out in order
                for (d, name), st in list(ops._SIDE_STREAMS.items()):
                    if name.startswith("wgrad"):
                        with torch.cuda.stream(st):
                            torch.cuda._sleep(int(2e8))
            step.training_step(net, s)
            red.finish()
            torch.cuda.synchronize()
            for k, p in net.named_parameters():
                if k in ref:
                    # bit-equal: the reducer (one rank) only routes the gradients through its buckets, and since round 5 no
                    # kernel on the path accumulates with atomics (RoIAlign's backward is a gather)
                    assert torch.equal(p.grad, ref[k]), (it, k)
        red.remove()
    finally:
        dist.destroy_process_group()


def test_flat_sgd_vs_torch(gpu):
    mc.check_flat_sgd(gpu)


def test_conv_bn_bias_fold(gpu):
    mc.check_conv_bn_bias_fold(gpu)


def test_train_epoch_accumulate(gpu):
    mc.check_train_epoch_accumulate(gpu)


def test_train_epoch_reference_golden(gpu):
    """train.train_epoch + train.make_optimizer vs the reference's own train_epoch / train_model optimizer, 3 steps at cfg0."""
    r = mc.check_train_epoch_golden(gpu)
    print("train_epoch golden:", r)


def test_train_loop_flat_sgd(gpu):
    """A short train_epoch-style loop (model.py:1600-1650) on the tiny config: hot path forward/backward, global
    clip to 5.0 and SGD(momentum, weight decay) on the flat arenas; the loss goes down on the fixed sample."""
    from cfun_amd import optim, step
    cfg = mc.tiny_config("finetune")
    torch.manual_seed(0)
    net = step.CFUNHotPath(cfg).to(gpu)
    s = step.synthetic_inputs(cfg, gpu, 0)
    b = cfg.UNET_MASK_BRANCH_CHANNEL
    gen = torch.Generator().manual_seed(1)
    net.mask.modified_u_net.dropout_masks = [torch.empty(4, c).bernoulli_(0.4, generator=gen) / 0.4
                                             for c in (b, 2 * b, 4 * b, 8 * b, 16 * b)]
    opt = optim.FlatSGD(net.named_parameters(), lr=cfg.LEARNING_RATE, momentum=cfg.LEARNING_MOMENTUM,
                        weight_decay=cfg.WEIGHT_DECAY, clip_norm=5.0)
    sd_keys = set(net.state_dict())
    totals = []
    for _ in range(6):
        opt.zero_grad()
        _, losses, total = step.training_step(net, s)
        opt.step()
        totals.append(float(total.detach()))
        assert float(opt.grad_norm[0]) > 0
    assert all(t == t for t in totals) and totals[-1] < totals[0], totals
    assert set(net.state_dict()) == sd_keys                 # parameters moved into arenas, the module is unchanged


def test_cfg3_volume_forward_properties(gpu):
    """BASELINE.json configs[3] size on ONE GPU (512x512x256, 268 MB input): FPN + RPN + proposals run, shapes follow
    SURVEY.md section 8(a) (147 456 anchors), outputs are finite, RPN probabilities are distributions and the
    proposals are inside the unit cube -- size-independent properties, the oracle would need minutes here."""
    from cfun_amd import config, step
    cfg = config.heart_config("beginning", 512, 512, 256)
    torch.manual_seed(0)
    net = step.CFUNHotPath(cfg).to(gpu).eval()
    image = torch.randn(1, 1, 256, 512, 512, device=gpu)
    with torch.no_grad():
        p2, p3, logits, probs, bbox = net.backbone_rpn(image)
        rois = net.proposals(probs, bbox, "inference")
    assert tuple(p2.shape) == (1, 32, 64, 64, 128) and tuple(p3.shape) == (1, 16, 32, 32, 128)
    assert logits.shape[1] == 147456 == net.anchors.shape[0]
    assert bool(torch.isfinite(p2).all()) and bool(torch.isfinite(bbox).all())
    assert float((probs.sum(-1) - 1).abs().max()) < 1e-5
    assert 1 <= rois.shape[1] <= cfg.POST_NMS_ROIS_INFERENCE
    assert float(rois.min()) >= 0.0 and float(rois.max()) <= 1.0


def test_cfg3_full_step_properties(gpu):
    """BASELINE.json configs[3]'s volume (512x512x256, 147 456 anchors) through the FULL 'finetune' step on one GPU --
    FPN / RPN / proposals on 8x the voxels of cfg2, classifier on 12 RoIs, the U-Net on 4 positive RoIs (96^3 -> 192^3),
    six losses incl. the edge loss, backward (cfg3 had only been run forward).  Size-independent
    properties: the heads are not skipped, every one of the 95 trainable tensors receives a finite non-zero gradient,
    the proposals lie in the unit cube, and with fixed Dropout3d masks the losses and every gradient repeat bit for bit."""
    from cfun_amd import config, step
    cfg = config.heart_config("finetune", 512, 512, 256)
    torch.manual_seed(0)
    net = step.CFUNHotPath(cfg).to(gpu)
    s = step.synthetic_inputs(cfg, gpu, 0)
    assert s["p_rois"].shape[0] == 4 and s["n_rois"].shape[0] == 8 and tuple(s["image"].shape) == (1, 1, 256, 512, 512)
    b = cfg.UNET_MASK_BRANCH_CHANNEL
    gen = torch.Generator().manual_seed(1)
    net.mask.modified_u_net.dropout_masks = [torch.empty(4, c).bernoulli_(0.4, generator=gen) / 0.4
                                             for c in (b, 2 * b, 4 * b, 8 * b, 16 * b)]

    def run():
        net.zero_grad(set_to_none=True)
        out, losses, _ = step.training_step(net, s)
        torch.cuda.synchronize()
        return out, [float(l.detach()) for l in losses], {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
    out, l1, g1 = run()
    assert out["rpn_class_logits"].shape[1] == 147456 == net.anchors.shape[0]
    assert tuple(out["mrcnn_mask_logits"].shape) == (4, 192, 192, 192, 8) and tuple(out["mrcnn_class_logits"].shape) == (12, 2)
    rois = out["rpn_rois"]
    assert 1 <= rois.shape[1] <= cfg.POST_NMS_ROIS_TRAINING and float(rois.min()) >= 0.0 and float(rois.max()) <= 1.0
    assert all(np.isfinite(v) and v > 0 for v in l1), l1
    trainable = [k for k, p in net.named_parameters() if p.requires_grad]
    assert len(trainable) == 95 and sorted(g1) == sorted(trainable)
    for k, v in g1.items():
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0, k
    del out
    _, l2, g2 = run()
    assert l1 == l2
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    del g1, g2
    torch.cuda.empty_cache()


def test_lits_full_size_step_properties(gpu):
    """BASELINE.json configs[4] at the fork's real sizes (320x320x256 volume, P3D35, (5,7,7) stem, b = 32, 3 classes,
    32x80x80 crops), both training phases of the fork: 'beginning' trains the detector only (no mask head), 'together'
    the mask branch only (everything else frozen, no classifier head).  The step runs, the losses are finite, exactly
    the phase's trainable tensors receive finite gradients.  (Value parity for these shapes:
    test_training_step_lits_shapes / _finetune and the unet_lits_eval golden.)"""
    from cfun_amd import config, step
    for stage in ("beginning", "together"):
        cfg = config.LiTSConfig(stage)
        torch.manual_seed(0)
        net = step.CFUNHotPath(cfg).to(gpu)
        s = step.synthetic_inputs(cfg, gpu, 0)
        assert tuple(s["image"].shape) == (1, 1, 256, 320, 320)
        net.zero_grad(set_to_none=True)
        out, losses, total = step.training_step(net, s)
        assert all(bool(torch.isfinite(l)) for l in losses)
        if stage == "beginning":
            assert out["mrcnn_mask_logits"] is None and tuple(out["mrcnn_class_logits"].shape) == (12, 2)
            assert float(losses[4]) == 0.0 and float(losses[5]) == 0.0 and float(losses[0]) > 0.0
        else:
            assert out["mrcnn_class_logits"] is None and tuple(out["mrcnn_mask_logits"].shape) == (4, 32, 80, 80, 3)
            assert float(losses[0]) == 0.0 and float(losses[2]) == 0.0 and float(losses[4]) > 0.0
        for k, p in net.named_parameters():
            in_mask = k.startswith("mask.")
            if stage == "beginning":
                assert (p.grad is None) == (in_mask or not p.requires_grad), k
            else:
                assert p.requires_grad == (in_mask or (k.startswith("classifier.") and ".bn" not in k)), k
                if in_mask and "out_upscale_conv" not in k:     # ('finetune'-only conv, mask_branch.py:118-122)
                    assert p.grad is not None, k
            if p.grad is not None:
                assert bool(torch.isfinite(p.grad).all()), k
        del net, out, losses, total
        torch.cuda.empty_cache()

def test_unmold_golden(gpu):
    mc.check_unmold_golden(gpu)


def test_unmold_lits_golden(gpu):
    mc.check_unmold_lits_golden(gpu)


def test_mask_head_side_stream(gpu):
    """The optional two-stream step (mask head beside FPN / RPN / classifier, step.OVERLAP_MASK_HEAD) runs the same
    kernels on the same data: losses and EVERY gradient equal the single-stream step bit for bit (RoIAlign's backward is a
    gather since round 5: no order-dependent sum is left on the path)."""
    from cfun_amd import step
    cfg = mc.tiny_config("finetune")
    torch.manual_seed(0)
    net = step.CFUNHotPath(cfg).to(gpu)
    s = step.synthetic_inputs(cfg, gpu, 0)
    results = []
    old = step.OVERLAP_MASK_HEAD
    try:
        for flag in (False, True, True):
            step.OVERLAP_MASK_HEAD = flag
            torch.manual_seed(5)                      # the same host-drawn Dropout3d masks every time
            net.zero_grad(set_to_none=True)
            _, losses, total = step.training_step(net, s)
            torch.cuda.synchronize()
            results.append(([float(l) for l in losses],
                            {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}))
    finally:
        step.OVERLAP_MASK_HEAD = old
    for losses, grads in results[1:]:
        assert losses == results[0][0]
        assert grads.keys() == results[0][1].keys()
        for k, g in grads.items():
            assert torch.equal(g, results[0][1][k]), k


def test_rccl_self_exchange_on_side_stream(gpu):
    """The `nccl` (= RCCL) branch of ``dist._exchange`` has never met a peer (the test boxes have one GPU and RCCL refuses two
    ranks on a device: tools/probe_rccl_one_gpu.py).  What CAN run here: a one-rank RCCL group whose ring neighbours are the
    rank itself -- ``dist._exchange_async`` then hands DEVICE buffers straight to ``batch_isend_irecv`` on the side HIP stream
    (no host staging), RCCL pairs the two self-sends with the two self-receives in order, and the main stream picks the planes
    up after ``wait()``: the stream hand-over, the record_stream bookkeeping and the RCCL point-to-point calls of the halo
    exchange, with real data, minus the xGMI link."""
    import socket
    import torch.distributed as dist
    from cfun_amd import dist as cdist
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        class SelfRing:                       # a ShardContext whose previous AND next rank are this rank
            group, rank, world, prev, next = None, 0, 1, 0, 0
        gen = torch.Generator().manual_seed(0)
        for it in range(3):
            a = torch.randn(1, 2, 24, 24, 16, generator=gen).to(gpu)
            b = torch.randn(1, 1, 24, 24, 16, generator=gen).to(gpu)
            busy = torch.randn(2048, 2048, device=gpu)
            busy = busy @ busy                                  # the main stream is still working when the transfer starts
            sa, sb = a * 2.0, b * 3.0                           # produced on the main stream right before the exchange
            fp, fn, wait = cdist._exchange_async(SelfRing, sa, sb, tuple(sa.shape), tuple(sb.shape), sa)
            wait()
            got_p, got_n = fp + 0.0, fn + 0.0                   # consumed on the main stream
            torch.cuda.synchronize()
            assert torch.equal(got_p, a * 2.0) and torch.equal(got_n, b * 3.0), it
    finally:
        dist.destroy_process_group()


def test_preflight_over_single_rank_rccl(gpu):
    """bench.py's communication pre-flight (cfun_amd.dist_selftest) on a one-rank RCCL group: every collective call it makes --
    int64 all-gather, fp64 MAX all-reduce, the reducer's own communicator and stream -- goes through RCCL with device tensors
    (the exchanges degenerate to zero padding at world size 1; the two self-ring tests below cover the point-to-point path)."""
    import socket
    import torch.distributed as dist
    from cfun_amd import dist_selftest
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        pf = dist_selftest.preflight(torch.device(gpu))
        assert pf["ok"] and pf["backend"] == "nccl" and pf["rccl_ranks_seen"] == 1 and pf["devices_seen"] == 1, pf
    finally:
        dist.destroy_process_group()


def test_rccl_self_ring_halo_conv(gpu):
    """... and the whole depth-coupled conv of the sharded layout over RCCL: ``layers.sharded_conv`` -> ``dist.halo_conv``
    (interior planes enqueued while the halo planes travel on the side stream, edge planes after ``_HaloFinish``, the gradient
    planes travelling back in the backward) on a one-rank RCCL group whose neighbours are the rank itself.  A slab whose both
    halos come from itself is a convolution with REPLICATE depth padding (RCCL pairs a rank's self-sends with its
    self-receives in issue order: the planes sent "to the previous rank" -- the slab's first -- come back as the low halo) --
    checked against exactly that, forward, input gradient and weight gradient; plus the thin-slab fall-back
    (``_HaloExchange``) the same way."""
    import socket
    import torch.distributed as dist
    import torch.nn.functional as F
    from cfun_amd import dist as cdist
    from cfun_amd.layers import Conv3dParams
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        class SelfRing:                       # claims two ranks so that the sharded code paths engage; both neighbours = self
            group, rank, world, prev, next = None, 0, 2, 0, 0
        gen = torch.Generator().manual_seed(1)
        for planes, ci, co in ((8, 16, 32), (1, 8, 8)):            # interior / edge split; slab thinner than the kernel (padded slab)
            torch.manual_seed(3)
            conv = Conv3dParams(ci, co, 3, padding=1).to(gpu)
            x = torch.randn(1, planes, 8, 16, ci, generator=gen).to(gpu)
            gy = torch.randn(1, planes, 8, 16, co, generator=gen).to(gpu)
            xs = x.clone().requires_grad_(True)
            with cdist.depth_sharded_as(SelfRing):
                y = conv(xs)
                (y * gy).sum().backward()
            torch.cuda.synchronize()
            got = (y.detach(), xs.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone())
            conv.weight.grad = conv.bias.grad = None
            # reference: replicate padding along depth, zero padding in (y, x), torch fp32
            xr = x.clone().requires_grad_(True)
            xp = torch.cat([xr[:, :1], xr, xr[:, -1:]], dim=1).permute(0, 4, 1, 2, 3)
            yr = F.conv3d(xp, conv.weight, conv.bias, padding=(0, 1, 1)).permute(0, 2, 3, 4, 1)
            (yr * gy).sum().backward()
            ref = (yr.detach(), xr.grad, conv.weight.grad, conv.bias.grad)
            for a, b, nm in zip(got, ref, ("y", "dx", "dw", "db")):
                err = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-12)
                assert err < 2e-5, (planes, nm, err)
            conv.weight.grad = conv.bias.grad = None
    finally:
        dist.destroy_process_group()


def test_wgrad_stream_bitwise(gpu):
    """the weight gradients on their own HIP stream (ops.WGRAD_STREAM) depend on the autograd engine replaying
    _OnWgradStream / AccumulateGrad on the right stream and joining the leaf streams at the end of backward() -- behaviour of the
    torch build.  Same kernels, same data: every gradient with the stream on equals the single-stream step's bit for bit, on the
    real channel counts (b = 20, 'finetune', 96^3 -> 192^3: every weight-gradient kernel family of the bench step)."""
    from cfun_amd import config, ops, step
    cfg = config.heart_config("finetune", 64, 64, 32)
    torch.manual_seed(0)
    net = step.CFUNHotPath(cfg).to(gpu)
    s = step.synthetic_inputs(cfg, gpu, 0)
    b = cfg.UNET_MASK_BRANCH_CHANNEL
    gen = torch.Generator().manual_seed(3)
    net.mask.modified_u_net.dropout_masks = [torch.empty(4, c).bernoulli_(0.4, generator=gen) / 0.4
                                             for c in (b, 2 * b, 4 * b, 8 * b, 16 * b)]
    results = []
    old = ops.WGRAD_STREAM
    try:
        for flag in (False, True, True):
            ops.WGRAD_STREAM = flag
            net.zero_grad(set_to_none=True)
            _, losses, _ = step.training_step(net, s)
            torch.cuda.synchronize()
            results.append(([float(l) for l in losses],
                            {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}))
    finally:
        ops.WGRAD_STREAM = old
    assert len(results[0][1]) == 95
    for losses, grads in results[1:]:
        assert losses == results[0][0]
        for k, g in grads.items():
            assert torch.equal(g, results[0][1][k]), k


def test_training_step_lits_finetune(gpu):
    """LiTS fork 'finetune': class-weighted mask CE + raw-Sobel edge loss through the whole step vs the oracle."""
    mc.check_training_step_vs_oracle(gpu, mc.tiny_lits_config("finetune"))


def test_fpn_rpn_lits_golden(gpu):
    mc.check_fpn_rpn_lits_golden(gpu)


def test_unet_lits_noncubic_golden(gpu):
    mc.check_unet_golden(gpu, "unet_lits_noncubic")


def test_detection_target_layer_lits_golden(gpu):
    mc.check_detection_target_layer_lits_golden(gpu)


@pytest.mark.parametrize("stage", ["beginning", "together"])
def test_predict_lits_golden(gpu, stage):
    mc.check_predict_lits_golden(gpu, stage)


def test_input_pipeline(gpu):
    mc.check_input_pipeline(gpu)


def test_async_scalar_ring_keeps_every_deferred_value(gpu):
    """AsyncScalar's 16 pinned buffers are a ring -- an instance whose buffer is handed to a newer one must
    keep ITS value (40 scalars deferred, read back afterwards in creation order and in reverse)."""
    import torch
    from cfun_amd import hostio
    vals = [torch.full((3,), float(i), device=gpu) + torch.arange(3, device=gpu) for i in range(40)]
    pend = [hostio.AsyncScalar(v) for v in vals]
    for i in list(range(0, 40, 2)) + list(range(39, 0, -2)):
        assert pend[i].get().tolist() == [float(i), float(i) + 1, float(i) + 2], i


def test_resize_known_answers_device(gpu):
    """cfun_resize3d against the hand-derived known answers of skimage.transform.resize (tests/golden/resize_kat.json)."""
    mc.check_resize_kat_device(gpu)


@pytest.mark.parametrize("which", ["tiny", "cfg0_real_channels"])
def test_wgrad_stream_lagging_far_behind_is_bit_identical(gpu, which):
    """The weight-gradient stream (cfun_amd.ops.WGRAD_STREAM) reads tensors the backward chain allocated and
    autograd frees the moment a node's backward returns.  Here the weight-gradient streams are put to sleep before
    ``backward()`` so that the WHOLE chain -- and every free -- runs ahead of them, while the host keeps allocating and
    freeing on the chain's streams: any tensor missing its ``record_stream`` is overwritten before the sleeping stream reads
    it (the round-5 bug: the Dropout3d index lists -> a memory fault on an interior rank of the 4-rank test).  Every
    gradient must equal the single-stream step bit for bit."""
    from cfun_amd import config, ops, step
    # tiny: 32^3 crops, b = 4 (direct kernels, per-RoI Dropout3d slices); cfg0_real_channels: 64x64x32 volume, b = 20, 96^3 -> 192^3
    # (Winograd kernels, the fused norm prologue's statistics, folded up-convs, the 113 MB classifier weight)
    cfg = mc.tiny_config("finetune") if which == "tiny" else config.heart_config("finetune", 64, 64, 32)
    torch.manual_seed(0)
    net = step.CFUNHotPath(cfg).to(gpu)
    s = step.synthetic_inputs(cfg, gpu, 0)
    dev = torch.device(gpu)

    def run(lag):
        torch.manual_seed(5)                      # the same host-drawn Dropout3d masks every time
        net.zero_grad(set_to_none=True)
        out = net.predict_training(s["image"], s["p_rois"], s["n_rois"], lazy_rois=True)
        losses = net.compute_losses(out, s["rpn_match"], s["rpn_bbox_t"], s["target_class_ids"], s["target_deltas"], s["mask_labels"])
        total = net.total_loss(losses)
        if lag:
            for (d, name), st in list(ops._SIDE_STREAMS.items()):
                if name.startswith("wgrad"):
                    with torch.cuda.stream(st):
                        torch.cuda._sleep(int(3e8))          # ~0.15 s: the chain's backward takes a few ms
        total.backward()
        if lag:       # churn: the chain's allocator hands freed blocks out again while the weight-gradient streams sleep
            junk = []
            for (d, name), st in list(ops._SIDE_STREAMS.items()) + [((0, "main"), torch.cuda.current_stream(dev))]:
                if name.startswith("wgrad"):
                    continue
                with torch.cuda.stream(st):
                    for k in range(40):
                        junk.append(torch.full((1 << (10 + k % 12),), float("nan"), device=dev))
                    junk.clear()
        torch.cuda.synchronize()
        return [float(l) for l in losses], {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}

    old = ops.WGRAD_STREAM
    try:
        ops.WGRAD_STREAM = False
        l0, g0 = run(False)
        ops.WGRAD_STREAM = True
        run(False)                                   # creates the weight-gradient streams
        assert any(name.startswith("wgrad") for (_, name) in ops._SIDE_STREAMS)
        for _ in range(3 if which == "tiny" else 2):
            l1, g1 = run(True)
            assert l1 == l0
            assert g1.keys() == g0.keys()
            for k in g0:
                assert torch.equal(g1[k], g0[k]), k
    finally:
        ops.WGRAD_STREAM = old
