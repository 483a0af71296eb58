#!/usr/bin/env python3
"""The heart sample from the loader's grid (cfun_amd.sample.resize_rotate_box / make_sample_heart) at the product shape, HIP-event
timed: a 512x512x224 int16 volume in NIfTI (Fortran) order with int16 labels -> [192,320,320].

  * cfun_sample_heart -- the C entry with preallocated buffers: without rotation and z-score, with the rotation (13 degrees), and
    with both (the training form); its bytes are counted per OUTPUT voxel as if every tap were fetched once: nothing more than
    the output's 5 B (+ 8 B for the z-score's flat pass) and the source's 2 + 2 B per SOURCE voxel;
  * a ``copy_`` that moves the same number of bytes: a yardstick, reported as a ratio, no threshold;
  * the composed route the library had before this pass: utils.resize_image + utils.resize_mask + rotate_and_box + mold_image;
  * make_sample_heart whole against make_sample whole (wrappers, RPN targets; device tensors in), each as a share of the 41.1 ms
    heart step of profiles/sample_pipeline.txt.

    python tools/bench_sample_heart.py [--out profiles/sample_heart_pipeline.txt]
"""
import argparse
import ctypes as C
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cfun_amd import _lib, config, sample, utils  # noqa: E402
from cfun_amd._lib import ptr  # noqa: E402
from cfun_amd.ops import ptr_raw  # noqa: E402

HEART_STEP_MS = 41.0986         # profiles/sample_pipeline.txt: one training step of HeartConfig at 320x320x192
ANGLE = 13.0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sample_heart needs a GPU: nothing here is measured on the host"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    cfg = config.HeartConfig("beginning")
    mx, mn = int(cfg.IMAGE_MAX_DIM), int(cfg.IMAGE_MIN_DIM)
    h, w, d = mx, mx, mn
    sh, sw, sd = 512, 512, 224
    n, ns = h * w * d, sh * sw * sd
    g = torch.Generator().manual_seed(0)
    # NIfTI order: H fastest
    image = torch.randint(-1024, 1500, (sd, sw, sh), generator=g, dtype=torch.int16).to(dev).permute(2, 1, 0)
    mask = torch.zeros((sd, sw, sh), dtype=torch.int16)
    mask[40:170, 120:380, 100:400] = torch.randint(0, 3, (130, 260, 300), generator=g, dtype=torch.int16)
    mask = mask.to(dev).permute(2, 1, 0)
    assert image.stride() == (1, sh, sh * sw)

    out = torch.empty((d, h, w), dtype=torch.float32, device=dev)
    lab = torch.empty((d, h, w), dtype=torch.uint8, device=dev)
    small = torch.empty(16, dtype=torch.int32, device=dev)
    stats = torch.empty(2, dtype=torch.float64, device=dev)
    lo, hi = torch.aminmax(image)
    clip = torch.stack([lo, hi]).to(torch.float64).contiguous()
    i64, i32 = C.c_int64 * 3, C.c_int32 * 3
    ws = _lib.workspace(lib.cfun_sample_heart_workspace_bytes(i32(h, w, d)), image)
    st = _lib.stream(image)
    rad = math.radians(ANGLE)

    def the_pass(rotate, zscore):
        _lib.check(lib.cfun_sample_heart(ptr_raw(image), i64(*image.stride()), _lib.ELEM_INT16, ptr_raw(mask), i64(*mask.stride()),
                                         _lib.LABEL_INT16, i32(sh, sw, sd), i32(h, w, d), ptr(clip), 1, math.cos(rad), math.sin(rad),
                                         int(rotate), int(zscore), ptr(out), ptr(lab), ptr(small[0:6]), ptr(small[6:12]),
                                         ptr(small[12:13]), ptr(stats), ptr(ws), ws.numel(), st), "sample_heart")

    nbytes = 5 * n + 4 * ns                      # the gather: 4 + 1 B written per output voxel, 2 + 2 B read per source voxel
    zbytes = nbytes + 8 * n                      # ... plus the flat pass: 4 B read, 4 B written
    c_src = torch.empty(zbytes // 2, dtype=torch.uint8, device=dev).fill_(1)
    c_dst = torch.empty_like(c_src)
    c_half = nbytes // 2

    def composed():
        img = utils.resize_image(image[..., None], min_dim=mn, max_dim=mx, mode="self", device=dev)[0]
        lbl = utils.resize_mask(mask, None, None, max_dim=mx, min_dim=mn, mode="self", device=dev)
        o = sample.rotate_and_box(img[..., 0], lbl, ANGLE)
        return (utils.mold_image(o[0]),) + tuple(o[1:])

    a = composed()
    the_pass(1, 1)
    torch.cuda.synchronize()
    same = bool(torch.equal(a[1], lab)) and a[3].tolist() == small[6:12].tolist()
    worst = float((a[0] - out).abs().max())

    t = {"plain": [], "rot": [], "full": [], "copy": [], "zcopy": [], "composed": []}
    for _ in range(3):                          # alternated: all of them see the same machine state
        t["plain"].append(events(lambda: the_pass(0, 0), args.iters))
        t["rot"].append(events(lambda: the_pass(1, 0), args.iters))
        t["full"].append(events(lambda: the_pass(1, 1), args.iters))
        t["copy"].append(events(lambda: c_dst[:c_half].copy_(c_src[:c_half]), args.iters))
        t["zcopy"].append(events(lambda: c_dst.copy_(c_src), args.iters))
        t["composed"].append(events(composed, max(args.iters // 5, 5)))
    t = {k: min(v) for k, v in t.items()}

    anchors = torch.from_numpy(utils.generate_pyramid_anchors(cfg.RPN_ANCHOR_SCALES, cfg.RPN_ANCHOR_RATIOS,
                                                              utils.compute_backbone_shapes(cfg, cfg.IMAGE_SHAPE), cfg.BACKBONE_STRIDES,
                                                              cfg.RPN_ANCHOR_STRIDE)).float().to(dev)
    keys = torch.randint(0, 1 << 32, (anchors.shape[0],), generator=g, dtype=torch.int64).to(dev)
    t_new, t_old = [], []
    for _ in range(3):
        t_new.append(events(lambda: sample.make_sample_heart(image, mask, ANGLE, cfg, anchors, keys), 20))
        t_old.append(events(lambda: sample.make_sample(image, mask, ANGLE, cfg, anchors, keys), 10))
    t_new, t_old = min(t_new), min(t_old)
    s = sample.make_sample_heart(image, mask, ANGLE, cfg, anchors, keys)

    mb = 1e6
    row = "  %-40s %8.1f us   %6.1f MB  %5.2f TB/s"
    lines = ["heart sample path on %s, HIP events, best of 3 x %d calls (alternated)" % (torch.cuda.get_device_name(0), args.iters), "",
             "source [H,W,D] = %dx%dx%d int16 (Fortran order) + int16 labels -> [D',H',W'] = %dx%dx%d (%.1f M voxels), truncate, clip"
             % (sh, sw, sd, d, h, w, n / 1e6),
             row % ("cfun_sample_heart, no rotation, no z-score", t["plain"] * 1e3, nbytes / mb, nbytes / t["plain"] / 1e9),
             row % ("cfun_sample_heart, %g degrees, no z-score" % ANGLE, t["rot"] * 1e3, nbytes / mb, nbytes / t["rot"] / 1e9),
             row % ("cfun_sample_heart, %g degrees, z-score" % ANGLE, t["full"] * 1e3, zbytes / mb, zbytes / t["full"] / 1e9),
             row % ("copy_ of the gather's bytes", t["copy"] * 1e3, nbytes / mb, nbytes / t["copy"] / 1e9),
             row % ("copy_ of the gather's + flat pass's bytes", t["zcopy"] * 1e3, zbytes / mb, zbytes / t["zcopy"] / 1e9),
             "  pass / copy_: %.2fx without rotation and z-score, %.2fx rotated, %.2fx rotated and z-scored (a yardstick, no threshold)"
             % (t["plain"] / t["copy"], t["rot"] / t["copy"], t["full"] / t["zcopy"]),
             "  working sets: source %.0f MB + labels %.0f MB + outputs %.0f MB = %.0f MB per call: more than the 256 MiB (268 MB)"
             " Infinity Cache, so back-to-back calls do not find the whole set resident; the %.0f MB the two sources make do fit it,"
             " as do the copies' halves"
             % (2 * ns / mb, 2 * ns / mb, 5 * n / mb, (4 * ns + 5 * n) / mb, 4 * ns / mb),
             "  %-40s %8.1f us   (resize_image + resize_mask + rotate_and_box + mold_image)" % ("composed route, %g degrees" % ANGLE,
                                                                                              t["composed"] * 1e3),
             "  composed / pass (rotated, z-scored): %.2fx   labels and box equal: %s; worst |image difference| %.3g"
             " (z-score units; the composed route resizes in float32, so its cast back lands one integer away at some voxels)"
             % (t["composed"] / t["full"], same, worst),
             "  %-40s %8.1f us   = %.2f %% of the %.1f ms heart step (device tensors in; box %s, kept %s)"
             % ("make_sample_heart, whole", t_new * 1e3, 100 * t_new / HEART_STEP_MS, HEART_STEP_MS, s["raw_box"].tolist(),
                s["rpn_counts"].tolist()),
             "  %-40s %8.1f us   = %.2f %% of it;  make_sample / make_sample_heart: %.2fx"
             % ("make_sample, whole", t_old * 1e3, 100 * t_old / HEART_STEP_MS, t_old / t_new), ""]
    txt = "\n".join(lines)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
