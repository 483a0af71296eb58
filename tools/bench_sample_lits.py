#!/usr/bin/env python3
"""The LiTS fork's training sample on the device (cfun_amd.sample.frame_rotate_resize / make_sample_lits) at the product shape,
HIP-event timed: a 512x512x200 HU volume with int8 labels -> the virtual 646x646x536 frame -> [256,320,320].

  * cfun_sample_lits -- the C entry with preallocated buffers, at angle None and at 17 degrees, and its bytes: 10 B per output
    voxel (a 4-byte and a 1-byte read, a 4-byte and a 1-byte write), counted as if every output voxel had a source voxel; the
    z stride of about 2.1 elements makes the sectors actually fetched about twice the bytes used, by construction;
  * a ``copy_`` that moves the same number of bytes: a yardstick, reported as a ratio, no threshold;
  * at angle None, the route a user can compose from the pieces the library had before this pass: preprocess_image_lits, two
    resize3d(order=0, frame, offset), the label casts either side, then rotate_and_box(None);
  * the whole make_sample_lits (wrappers, RPN targets, window and meta; device tensors in) as a share of the 14.1 ms LiTS step
    of profiles/sample_pipeline.txt.

    python tools/bench_sample_lits.py [--out profiles/sample_lits_pipeline.txt]
"""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cfun_amd import _lib, config, ops, sample, utils  # noqa: E402
from cfun_amd._lib import ptr  # noqa: E402
from cfun_amd.ops import ptr_raw  # noqa: E402

LITS_STEP_MS = 14.0798          # profiles/sample_pipeline.txt: one training step of LiTSConfig at 320x320x256
ANGLE = 17


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
    assert torch.cuda.is_available(), "bench_sample_lits needs a GPU: nothing here is measured on the host"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    cfg = config.LiTSConfig("beginning")
    frame = [int(v) for v in cfg.PAD_IMAGE_SHAPE]
    h, w, d = [int(v) for v in cfg.IMAGE_SHAPE[:3]]
    sh, sw, sd = 512, 512, 200
    off = [int((p - k) / 2.0) for p, k in zip(frame, (sh, sw, sd))]
    n = h * w * d
    g = torch.Generator().manual_seed(0)
    image = (torch.randn((sh, sw, sd), generator=g) * 250.0).to(dev)
    mask = torch.zeros((sh, sw, sd), dtype=torch.int8)
    mask[100:400, 120:380, 40:170] = torch.randint(0, 3, (300, 260, 130), generator=g, dtype=torch.int8)
    mask = mask.to(dev)

    out = torch.empty((d, h, w), dtype=torch.float32, device=dev)
    lab = torch.empty((d, h, w), dtype=torch.uint8, device=dev)
    small = torch.empty(16, dtype=torch.int32, device=dev)
    i64, i32 = C.c_int64 * 3, C.c_int32 * 3
    ws = _lib.workspace(lib.cfun_sample_lits_workspace_bytes(i32(h, w, d)), image)
    st = _lib.stream(image)
    amap = (C.c_double * 6)(*sample.rotation_map(ANGLE, frame[0], frame[1]))

    def the_pass(m):
        _lib.check(lib.cfun_sample_lits(ptr_raw(image), i64(*image.stride()), ptr_raw(mask), i64(*mask.stride()), 1, i32(sh, sw, sd),
                                        i32(*frame), i32(*off), i32(h, w, d), m, 1, ptr(out), ptr(lab), ptr(small[0:6]),
                                        ptr(small[6:12]), ptr(small[12:13]), ptr(ws), ws.numel(), st), "sample_lits")

    nbytes = 10 * n
    c_src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev).fill_(1)
    c_dst = torch.empty_like(c_src)

    def composed():
        img = ops.resize3d(utils.preprocess_image_lits(image), (h, w, d), order=0, frame=frame, offset=off)
        lbl = ops.resize3d(mask.to(torch.float32), (h, w, d), order=0, frame=frame, offset=off).to(torch.int32)
        return sample.rotate_and_box(img, lbl, None)

    a = composed()
    the_pass(None)
    torch.cuda.synchronize()
    same = bool(torch.equal(a[1], lab)) and a[3].tolist() == small[6:12].tolist()
    # (the composed route's image goes through torch's device division: see DESIGN.md section 7 on its last bit)
    img_diff = int((a[0] != out).sum())

    t = {"none": [], "rot": [], "copy": [], "composed": []}
    for _ in range(3):                          # alternated: all four see the same machine state
        t["none"].append(events(lambda: the_pass(None), args.iters))
        t["rot"].append(events(lambda: the_pass(amap), args.iters))
        t["copy"].append(events(lambda: c_dst.copy_(c_src), args.iters))
        t["composed"].append(events(composed, max(args.iters // 5, 5)))
    t = {k: min(v) for k, v in t.items()}

    anchors = torch.from_numpy(utils.generate_pyramid_anchors(cfg.RPN_ANCHOR_SCALES, cfg.RPN_ANCHOR_RATIOS,
                                                              utils.compute_backbone_shapes(cfg, cfg.IMAGE_SHAPE), cfg.BACKBONE_STRIDES,
                                                              cfg.RPN_ANCHOR_STRIDE)).float().to(dev)
    keys = torch.randint(0, 1 << 32, (anchors.shape[0],), generator=g, dtype=torch.int64).to(dev)
    t_all = min(events(lambda: sample.make_sample_lits(image, mask, ANGLE, cfg, anchors, keys), 20) for _ in range(3))
    s = sample.make_sample_lits(image, mask, ANGLE, cfg, anchors, keys)

    row = "  %-34s %8.1f us   %6.1f MB  %5.2f TB/s"
    lines = ["LiTS sample path on %s, HIP events, best of 3 x %d calls (alternated)" % (torch.cuda.get_device_name(0), args.iters), "",
             "source [H,W,D] = %dx%dx%d float32 HU + int8 labels -> frame %dx%dx%d -> [D',H',W'] = %dx%dx%d (%.1f M voxels)"
             % (sh, sw, sd, frame[0], frame[1], frame[2], d, h, w, n / 1e6),
             row % ("cfun_sample_lits, angle None", t["none"] * 1e3, nbytes / 1e6, nbytes / t["none"] / 1e9),
             row % ("cfun_sample_lits, angle %d" % ANGLE, t["rot"] * 1e3, nbytes / 1e6, nbytes / t["rot"] / 1e9),
             row % ("copy_ of the same bytes", t["copy"] * 1e3, nbytes / 1e6, nbytes / t["copy"] / 1e9),
             "  pass / copy_: %.2fx at angle None, %.2fx at %d degrees   (a yardstick: the z stride wastes sectors by construction)"
             % (t["none"] / t["copy"], t["rot"] / t["copy"], ANGLE),
             "  %-34s %8.1f us   (preprocess_image_lits, 2 x resize3d(order=0, frame, offset), label casts, rotate_and_box(None))"
             % ("composed route, angle None", t["composed"] * 1e3),
             "  composed / pass at angle None: %.2fx   labels and box equal: %s; image voxels that differ: %d of %d"
             % (t["composed"] / t["none"], same, img_diff, n),
             "  %-34s %8.1f us   = %.2f %% of the %.1f ms LiTS step (device tensors in; box %s, kept %s)"
             % ("make_sample_lits, whole, angle %d" % ANGLE, t_all * 1e3, 100 * t_all / LITS_STEP_MS, LITS_STEP_MS,
                s["raw_box"].tolist(), s["rpn_counts"].tolist()), ""]
    txt = "\n".join(lines)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
