#!/usr/bin/env python3
"""The warp pass (cfun_amd.sample.warp_and_box, ``augment=`` on the sample routes) at the product shapes, HIP-event timed: the
heart sample [D,H,W] = 192x320x320 and the LiTS sample 256x320x320, each with a 5^3 control grid, a 13-degree in-plane map and an
x flip, image order 0 and order 1.

  * cfun_sample_warp -- the C entry with preallocated buffers; its bytes are counted as if every voxel were fetched once: 4 + 1 B
    read and 4 + 1 B written per voxel;
  * a ``copy_`` that moves the same number of bytes, and ``cfun_resize3d(order=0)`` at the same shape (the generic gather: 4 B
    read, 4 B written per voxel): yardsticks, reported as ratios, no threshold;
  * scipy.ndimage.map_coordinates on the host, on the restatement's coordinate stack: a baseline, not credit;
  * the output against tests/sample_warp_ref.py on three z slabs only -- the first, a middle one and the last;
  * make_sample_heart / make_sample_lits with and without ``augment`` (device tensors in), as shares of the training steps of
    profiles/sample_pipeline.txt.

    python tools/bench_sample_warp.py [--out profiles/sample_warp_pipeline.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cfun_amd import _lib, config, ops, sample, utils  # noqa: E402
from cfun_amd._lib import ptr  # noqa: E402

HEART_STEP_MS = 41.0986         # profiles/sample_pipeline.txt: one training step of HeartConfig at 320x320x192
LITS_STEP_MS = 14.0798          # ... of LiTSConfig at 320x320x256
ANGLE = 13.0
GRID = (5, 5, 5)
SLAB = 4                        # z planes per verified slab


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


def one_shape(name, shape, iters, lines, host):
    import sample_warp_ref as wr
    from scipy import ndimage
    dev = torch.device("cuda:0")
    lib = _lib.load()
    d, h, w = shape
    n = d * h * w
    g = torch.Generator().manual_seed(0)
    image = torch.randn(shape, generator=g).mul_(350.0).add_(100.0).to(dev)
    labels = torch.zeros(shape, dtype=torch.uint8)
    labels[d // 5:d - d // 5, h // 4:h - h // 4, w // 4:w - w // 4] = torch.randint(0, 3, (d - 2 * (d // 5), h - 2 * (h // 4), w - 2 * (w // 4)),
                                                                                  generator=g, dtype=torch.uint8)
    labels = labels.to(dev)
    warp = sample.draw_warp(shape, torch.Generator().manual_seed(1), grid=GRID, sigma=(3.0, 6.0, 6.0), angle=ANGLE, flip_p=(0, 0, 1))
    grid = warp.grid.to(dev).contiguous()
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    lab = torch.empty(shape, dtype=torch.uint8, device=dev)
    small = torch.empty(16, dtype=torch.int32, device=dev)
    i32 = C.c_int32 * 3
    ws = _lib.workspace(lib.cfun_sample_warp_workspace_bytes(i32(*shape)), image)
    st = _lib.stream(image)
    amap = (C.c_double * 6)(*warp.map)
    flips = sum(1 << k for k in range(3) if warp.flips[k])

    def the_pass(order):
        _lib.check(lib.cfun_sample_warp(ptr(image), ptr(labels), i32(*shape), ptr(grid), i32(*GRID), amap, flips, order, ptr(out),
                                        ptr(lab), ptr(small[0:6]), ptr(small[6:12]), ptr(small[12:13]), ptr(ws), ws.numel(), st),
                   "sample_warp")

    # the output against the restatement on three z slabs: the first, a middle one, the last
    slabs = [list(range(0, SLAB)), list(range(d // 2, d // 2 + SLAB)), list(range(d - SLAB, d))]
    img_np, lab_np, grid_np = image.cpu().numpy(), labels.cpu().numpy(), warp.grid.numpy()
    verified = True
    for order in (0, 1):
        the_pass(order)
        torch.cuda.synchronize()
        for planes in slabs:
            r_img, r_lab = wr.warp(img_np, lab_np, grid_np, warp.map, warp.flips, order, planes=planes)[:2]
            verified &= bool(torch.equal(out[planes].cpu().view(torch.int32), torch.from_numpy(r_img).view(torch.int32)))
            verified &= bool(torch.equal(lab[planes].cpu(), torch.from_numpy(r_lab)))
    box, changed = small[0:6].tolist(), float((lab != labels).float().mean())

    nbytes = 10 * n
    c_src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev).fill_(1)
    c_dst = torch.empty_like(c_src)
    t = {"o0": [], "o1": [], "copy": [], "resize": []}
    for _ in range(3):                          # alternated: all of them see the same machine state
        t["o0"].append(events(lambda: the_pass(0), iters))
        t["copy"].append(events(lambda: c_dst.copy_(c_src), iters))
        t["o1"].append(events(lambda: the_pass(1), iters))
        t["resize"].append(events(lambda: ops.resize3d(image, shape, order=0), iters))
    t = {k: min(v) for k, v in t.items()}

    t_host = {}
    if host:
        s = wr.coords(shape, grid_np, warp.map, warp.flips)
        for order in (0, 1):
            t0 = time.perf_counter()
            ndimage.map_coordinates(img_np, s, order=order, mode="constant")
            t_host[order] = time.perf_counter() - t0

    mb = 1e6
    row = "  %-44s %8.1f us   %6.1f MB  %5.2f TB/s"
    per_byte = {k: t[k] / nbytes for k in ("o0", "o1")}
    rs_per_byte = t["resize"] / (8 * n)
    lines += ["%s: [D,H,W] = %dx%dx%d (%.1f M voxels), control grid %dx%dx%d (scaled by %.3f), %g degrees, flips %s; %.0f %% of the"
              " labels changed, raw box %s" % (name, d, h, w, n / 1e6, GRID[0], GRID[1], GRID[2], warp.factor, ANGLE, warp.flips,
                                               100 * changed, box),
              row % ("cfun_sample_warp, image order 0", t["o0"] * 1e3, nbytes / mb, nbytes / t["o0"] / 1e9),
              row % ("cfun_sample_warp, image order 1", t["o1"] * 1e3, nbytes / mb, nbytes / t["o1"] / 1e9),
              row % ("copy_ of the same bytes", t["copy"] * 1e3, nbytes / mb, nbytes / t["copy"] / 1e9),
              row % ("cfun_resize3d(order=0), same shape", t["resize"] * 1e3, 8 * n / mb, 8 * n / t["resize"] / 1e9),
              "  pass / copy_: %.2fx order 0, %.2fx order 1;  order 1 / order 0: %.2fx (yardsticks, no threshold)"
              % (t["o0"] / t["copy"], t["o1"] / t["copy"], t["o1"] / t["o0"]),
              "  time per byte against the generic gather: %.2fx order 0, %.2fx order 1" % (per_byte["o0"] / rs_per_byte, per_byte["o1"] / rs_per_byte),
              "  working set: sources %.0f MB + outputs %.0f MB = %.0f MB per call, near the 256 MiB (268 MB) Infinity Cache: back-to-back"
              " calls find much of it resident, a training loop that touches other data in between does not"
              % (5 * n / mb, 5 * n / mb, 10 * n / mb),
              "  equal to tests/sample_warp_ref.py on z slabs %s, both orders: %s" % ([p[0] for p in slabs], verified)]
    if host:
        lines.append("  scipy.ndimage.map_coordinates on the host (a baseline, not credit; coordinates given): order 0 %.0f ms, order 1 %.0f ms"
                     % (t_host[0] * 1e3, t_host[1] * 1e3))
    lines.append("")
    return warp


def routes(lines):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(2)

    def anchors_of(cfg):
        return torch.from_numpy(utils.generate_pyramid_anchors(cfg.RPN_ANCHOR_SCALES, cfg.RPN_ANCHOR_RATIOS,
                                                               utils.compute_backbone_shapes(cfg, cfg.IMAGE_SHAPE), cfg.BACKBONE_STRIDES,
                                                               cfg.RPN_ANCHOR_STRIDE)).float().to(dev)

    cfg = config.HeartConfig("beginning")
    mx, mn = int(cfg.IMAGE_MAX_DIM), int(cfg.IMAGE_MIN_DIM)
    sh, sw, sd = 512, 512, 224
    image = torch.randint(-1024, 1500, (sd, sw, sh), generator=g, dtype=torch.int16).to(dev).permute(2, 1, 0)
    mask = torch.zeros((sd, sw, sh), dtype=torch.int16)
    mask[40:170, 120:380, 100:400] = torch.randint(0, 3, (130, 260, 300), generator=g, dtype=torch.int16)
    mask = mask.to(dev).permute(2, 1, 0)
    anchors = anchors_of(cfg)
    keys = torch.randint(0, 1 << 32, (anchors.shape[0],), generator=g, dtype=torch.int64).to(dev)
    warp = sample.draw_warp((mn, mx, mx), torch.Generator().manual_seed(1), grid=GRID, sigma=(3.0, 6.0, 6.0), angle=ANGLE, flip_p=(0, 0, 1))
    warp.grid = warp.grid.to(dev)
    t_w, t_p = [], []
    for _ in range(3):
        t_w.append(events(lambda: sample.make_sample_heart(image, mask, ANGLE, cfg, anchors, keys, augment=warp), 20))
        t_p.append(events(lambda: sample.make_sample_heart(image, mask, ANGLE, cfg, anchors, keys), 20))
    t_w, t_p = min(t_w), min(t_p)
    lines += ["routes, whole (wrappers, RPN targets; device tensors in), image order 1:",
              "  %-44s %8.1f us   = %.2f %% of the %.1f ms heart step" % ("make_sample_heart(augment=Warp)", t_w * 1e3, 100 * t_w / HEART_STEP_MS, HEART_STEP_MS),
              "  %-44s %8.1f us   = %.2f %% of it (z-score inside the pass; with a Warp torch's mold_image follows the warp)"
              % ("make_sample_heart(augment=None)", t_p * 1e3, 100 * t_p / HEART_STEP_MS)]
    del image, mask

    cfg = config.LiTSConfig("beginning")
    h, w, d = [int(v) for v in cfg.IMAGE_SHAPE[:3]]
    src = (512, 512, 200)
    image = torch.randn(src, generator=g).mul_(250.0).to(dev)
    mask = torch.zeros(src, dtype=torch.int8)
    mask[120:400, 100:380, 40:160] = torch.randint(0, 3, (280, 280, 120), generator=g, dtype=torch.int8)
    mask = mask.to(dev)
    anchors = anchors_of(cfg)
    keys = torch.randint(0, 1 << 32, (anchors.shape[0],), generator=g, dtype=torch.int64).to(dev)
    warp = sample.draw_warp((d, h, w), torch.Generator().manual_seed(1), grid=GRID, sigma=(3.0, 6.0, 6.0), angle=ANGLE, flip_p=(0, 0, 1))
    warp.grid = warp.grid.to(dev)
    t_w, t_p = [], []
    for _ in range(3):
        t_w.append(events(lambda: sample.make_sample_lits(image, mask, 17, cfg, anchors, keys, augment=warp), 20))
        t_p.append(events(lambda: sample.make_sample_lits(image, mask, 17, cfg, anchors, keys), 20))
    t_w, t_p = min(t_w), min(t_p)
    lines += ["  %-44s %8.1f us   = %.2f %% of the %.1f ms LiTS step" % ("make_sample_lits(augment=Warp)", t_w * 1e3, 100 * t_w / LITS_STEP_MS, LITS_STEP_MS),
              "  %-44s %8.1f us   = %.2f %% of it" % ("make_sample_lits(augment=None)", t_p * 1e3, 100 * t_p / LITS_STEP_MS), ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--no-host", action="store_true", help="skip the scipy baseline (about a minute of host time)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sample_warp needs a GPU: nothing but the scipy baseline is measured on the host"
    lines = ["warp pass on %s, HIP events, best of 3 x %d calls (alternated with the yardsticks)" % (torch.cuda.get_device_name(0), args.iters), ""]
    one_shape("heart", (192, 320, 320), args.iters, lines, not args.no_host)
    one_shape("LiTS", (256, 320, 320), args.iters, lines, not args.no_host)
    routes(lines)
    txt = "\n".join(lines)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
