#!/usr/bin/env python3
"""The training-sample path (cfun_amd/sample.py) at the product sizes, HIP-event timed:

  * cfun_sample_rotate_bbox -- rotate + re-lay + label cast + box, the C entry with preallocated buffers, and its bytes
    (13 B / voxel: two 4-byte reads, a 4-byte and a 1-byte write) as TB/s;
  * cfun_resize3d(order = 0) to the same [D,H,W] output from the same [H,W,D] source (8 B / voxel): the existing gather is the
    yardstick, compared as time per byte moved;
  * the whole load_image_gt (Python wrappers, mold_image, RPN targets) beside one training step of the same configuration;
  * tests/sample_ref.py, the numpy restatement, on 16 threads: a stated host baseline, not credit.

    python tools/bench_sample.py [--no-step] [--out profiles/sample_pipeline.txt]
"""
import argparse
import ctypes as C
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cfun_amd import _lib, config, sample, step  # noqa: E402
from cfun_amd._lib import ptr  # noqa: E402
from cfun_amd.ops import ptr_raw  # noqa: E402


def events(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters          # ms


def bench_config(name, cfg, lines, with_step):
    dev = torch.device("cuda:0")
    lib = _lib.load()
    h, w, d = [int(v) for v in cfg.IMAGE_SHAPE[:3]]
    n = h * w * d
    g = torch.Generator().manual_seed(0)
    image = torch.randn((h, w, d), generator=g).to(dev)
    mask = torch.zeros((h, w, d), dtype=torch.int32)
    mask[h // 5:4 * h // 5, w // 4:3 * w // 4, d // 6:5 * d // 6] = torch.randint(1, cfg.NUM_CLASSES, (4 * h // 5 - h // 5, 3 * w // 4 - w // 4, 5 * d // 6 - d // 6), generator=g, dtype=torch.int32)
    mask = mask.to(dev)
    lits = isinstance(cfg, config.LiTSConfig)
    angle = None if lits else 13.0
    rad = math.radians(angle or 0.0)

    out = torch.empty((d, h, w), dtype=torch.float32, device=dev)
    lab = torch.empty((d, h, w), dtype=torch.uint8, device=dev)
    small = torch.empty(16, dtype=torch.int32, device=dev)
    ws = _lib.workspace(lib.cfun_sample_workspace_bytes(h, w, d, 0, 0), image)
    i64, i32 = C.c_int64 * 3, C.c_int32 * 3
    st = _lib.stream(image)

    def rotate():
        _lib.check(lib.cfun_sample_rotate_bbox(ptr_raw(image), i64(*image.stride()), ptr_raw(mask), i64(*mask.stride()), i32(h, w, d),
                                               math.cos(rad), math.sin(rad), int(angle is not None), ptr(out), ptr(lab), ptr(small[0:6]),
                                               ptr(small[6:12]), ptr(small[12:13]), ptr(ws), ws.numel(), st), "rotate")

    src = image.permute(2, 0, 1)

    def gather():
        _lib.check(lib.cfun_resize3d(ptr_raw(src), i64(*src.stride()), i32(d, h, w), None, None, ptr(out), i32(d, h, w), 0, None, st),
                   "resize3d")

    # alternate the two so that both see the same machine state
    t_rot, t_gat = [], []
    for _ in range(3):
        t_rot.append(events(rotate, 50))
        t_gat.append(events(gather, 50))
    t_rot, t_gat = min(t_rot), min(t_gat)
    pb_rot, pb_gat = t_rot / (13.0 * n), t_gat / (8.0 * n)
    lines.append("%s  [H,W,D] = %dx%dx%d  (%.1f M voxels), angle %s" % (name, h, w, d, n / 1e6, angle))
    lines.append("  cfun_sample_rotate_bbox      %8.1f us   %6.1f MB  %5.2f TB/s   %.3f ps/B" % (t_rot * 1e3, 13.0 * n / 1e6, 13.0 * n / t_rot / 1e9, pb_rot * 1e9))
    lines.append("  cfun_resize3d(order=0)       %8.1f us   %6.1f MB  %5.2f TB/s   %.3f ps/B" % (t_gat * 1e3, 8.0 * n / 1e6, 8.0 * n / t_gat / 1e9, pb_gat * 1e9))
    lines.append("  time per byte, rotate / gather: %.2fx   (the margin to hold: 1.5x)" % (pb_rot / pb_gat))

    net = step.CFUNHotPath(cfg).to(dev) if with_step else None
    if net is not None:
        anchors = net.anchors.to(dev)
    else:
        from cfun_amd import utils
        anchors = torch.from_numpy(utils.generate_pyramid_anchors(cfg.RPN_ANCHOR_SCALES, cfg.RPN_ANCHOR_RATIOS,
                                                                  utils.compute_backbone_shapes(cfg, cfg.IMAGE_SHAPE), cfg.BACKBONE_STRIDES,
                                                                  cfg.RPN_ANCHOR_STRIDE)).float().to(dev)
    keys = torch.randint(0, 1 << 32, (anchors.shape[0],), generator=g, dtype=torch.int64).to(dev)
    boxf = small[6:12].float()[None].clone()
    t_rpn = events(lambda: sample.build_rpn_targets(anchors, boxf, cfg, keys), 20)
    t_all = events(lambda: sample.load_image_gt(image, mask, angle, cfg, anchors, keys), 20)
    s = sample.load_image_gt(image, mask, angle, cfg, anchors, keys)
    lines.append("  build_rpn_targets (A = %d)  %8.1f us   positives / negatives kept: %s" % (anchors.shape[0], t_rpn * 1e3, s["rpn_counts"].tolist()))
    lines.append("  load_image_gt, whole         %8.1f us   (wrappers, mold_image, targets; box %s)" % (t_all * 1e3, s["raw_box"].tolist()))

    if net is not None:
        smp = step.synthetic_inputs(cfg, dev, seed=0)

        def one():
            net.zero_grad(set_to_none=True)
            step.training_step(net, smp)
        t_step = events(one, 5, warmup=2)
        lines.append("  one training step            %8.1f us   load_image_gt = %.2f %% of it" % (t_step * 1e3, 100 * t_all / t_step))
        del net, smp
        torch.cuda.empty_cache()

    import sample_ref as sr
    torch.set_num_threads(16)
    img_np, mask_np, a_np, k_np = image.cpu().numpy(), mask.cpu().numpy(), anchors.cpu().numpy(), keys.cpu().numpy()
    t0 = time.perf_counter()
    sr.load_image_gt(img_np, mask_np, angle, cfg.NUM_CLASSES, a_np, cfg.RPN_TRAIN_ANCHORS_PER_IMAGE, cfg.RPN_BBOX_STD_DEV, k_np)
    t_host = time.perf_counter() - t0
    lines.append("  sample_ref on the host       %8.1f ms   (numpy, 16 threads allowed: a stated baseline, not credit)" % (t_host * 1e3))
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-step", action="store_true", help="skip the training step beside load_image_gt")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sample needs a GPU: nothing here is measured on the host"
    lines = ["training-sample path on %s, HIP events, best of 3 x 50 calls for the two kernels (alternated)" % torch.cuda.get_device_name(0), ""]
    bench_config("main (HeartConfig 320x320x192)", config.heart_config("beginning", 320, 320, 192), lines, not args.no_step)
    lcfg = config.LiTSConfig("beginning")
    bench_config("LiTS (LiTSConfig)", lcfg, lines, not args.no_step)
    txt = "\n".join(lines)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
