#!/usr/bin/env python3
"""The native-grid tier (cfun_amd.native) at a LiTS shape, HIP-event timed: a 512x512x129 int16 volume in NIfTI (Fortran) order
at spacing (0.70, 0.70, 2.5) mm -> resampled 452x452x214 (never built) -> frame 646x646x536 (never built) -> [256,320,320];
and the way back, a 214x452x452 uint8 class map -> a Fortran 512x512x129 volume.

  (a) cfun_mold_native -- the C entry with preallocated buffers and the clip range already on the device;
  (b) the route it replaces, composed from what the library had: to(float32), resize3d(order=1, clip=True) to the resampled
      shape (its min / max inside), utils.mold_inputs_lits; and the order-1 pass of it alone (no min / max, no clip);
  (c) a ``copy_`` of (a)'s bytes: the source once plus the output once;
  (d) cfun_map_resize;
  (e) run_test's save path: to(float32), resize3d(order=0), round, to(uint8);
  (f) a ``copy_`` of (d)'s bytes.
Acceptance is against routes measured in the same run: (a) < the order-1 pass of (b) alone, (d) < (e).  The ratios to the copies
are yardsticks, no threshold: (a) reads eight taps per output voxel through L2, so the bytes it MOVES are not the bytes it
fetches from HBM, and every buffer here fits the 256 MiB Infinity Cache (DESIGN.md section 7 on reading such rates).

    python tools/bench_native.py [--out profiles/native_pipeline.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cfun_amd import _lib, config, native, ops, utils  # noqa: E402
from cfun_amd._lib import ptr  # noqa: E402
from cfun_amd.ops import ptr_raw  # noqa: E402

SPACING = (0.70, 0.70, 2.5)


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
    assert torch.cuda.is_available(), "bench_native needs a GPU: nothing here is measured on the host"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    cfg = config.LiTSConfig("together")
    frame = [int(v) for v in cfg.PAD_IMAGE_SHAPE]
    h, w, d = [int(v) for v in cfg.IMAGE_SHAPE[:3]]
    shape = (512, 512, 129)
    rs = [int(v) for v in native.resampled_shape(shape, SPACING, cfg.MEAN_SPACING)]
    off = [int((p - k) / 2.0) for p, k in zip(frame, rs)]
    rng = np.random.default_rng(0)
    src = native._upload(np.asfortranarray(rng.integers(-1024, 1500, shape, dtype=np.int16)), dev)
    assert src.dtype == torch.int16 and src.stride() == (1, 512, 512 * 512)

    out = torch.empty((d, h, w), dtype=torch.float32, device=dev)
    lo, hi = torch.aminmax(src)
    clip = torch.stack([lo, hi]).to(torch.float64).contiguous()
    i64, i32 = C.c_int64 * 3, C.c_int32 * 3
    st = _lib.stream(src)

    def mold_pass():
        _lib.check(lib.cfun_mold_native(ptr_raw(src), i64(*src.stride()), _lib.ELEM_INT16, i32(*shape), i32(*rs), i32(*frame), i32(*off),
                                        i32(h, w, d), ptr(clip), 1, ptr(out), st), "mold_native")

    def order1_alone():
        return ops.resize3d(src_f32, rs, order=1)

    def composed():
        stored = ops.resize3d(src.to(torch.float32), rs, order=1, clip=True)
        return utils.mold_inputs_lits(cfg, [stored], device=dev)[0]

    src_f32 = src.to(torch.float32)
    mold_bytes = src.numel() * 2 + out.numel() * 4
    c_src = torch.empty(mold_bytes // 2, dtype=torch.uint8, device=dev).fill_(1)
    c_dst = torch.empty_like(c_src)

    cmap = torch.from_numpy(rng.integers(0, 3, (rs[2], rs[0], rs[1]), dtype=np.uint8)).to(dev)
    back_base = torch.empty((shape[2], shape[1], shape[0]), dtype=torch.uint8, device=dev)
    back = back_base.permute(2, 1, 0)
    cview = cmap.permute(1, 2, 0)

    def byte_pass():
        _lib.check(lib.cfun_map_resize(ptr_raw(cmap), i64(*cview.stride()), i32(*cview.shape), ptr(back_base), i64(*back.stride()),
                                       i32(*shape), st), "map_resize")

    def save_route():
        return torch.round(ops.resize3d(cview.to(torch.float32), shape, order=0)).to(torch.uint8)

    map_bytes = cmap.numel() + back.numel()
    m_src = torch.empty(map_bytes // 2, dtype=torch.uint8, device=dev).fill_(1)
    m_dst = torch.empty_like(m_src)

    mold_pass()
    ref = composed()
    byte_pass()
    torch.cuda.synchronize()
    mold_diff = int((ref[0, 0] != out).sum())
    mold_max = float((ref[0, 0] - out).abs().max())
    map_same = bool(torch.equal(save_route(), back))

    t = {k: [] for k in "abcdef"}
    t["b1"] = []
    for _ in range(3):                          # alternated: every row sees the same machine state
        t["a"].append(events(mold_pass, args.iters))
        t["b1"].append(events(order1_alone, max(args.iters // 5, 5)))
        t["b"].append(events(composed, max(args.iters // 5, 5)))
        t["c"].append(events(lambda: c_dst.copy_(c_src), args.iters))
        t["d"].append(events(byte_pass, args.iters))
        t["e"].append(events(save_route, max(args.iters // 5, 5)))
        t["f"].append(events(lambda: m_dst.copy_(m_src), args.iters))
    t = {k: min(v) for k, v in t.items()}

    row = "  %-44s %8.1f us   %6.1f MB  %5.2f TB/s"
    plain = "  %-44s %8.1f us"
    ok_a, ok_d = t["a"] < t["b1"], t["d"] < t["e"]
    lines = ["Native-grid tier on %s, HIP events, best of 3 x %d calls (alternated)" % (torch.cuda.get_device_name(0), args.iters), "",
             "source [H,W,D] = %dx%dx%d int16, Fortran order, spacing %s -> resampled %dx%dx%d -> frame %dx%dx%d -> [D',H',W'] = %dx%dx%d"
             % (shape + (SPACING,) + tuple(rs) + tuple(frame) + (d, h, w)),
             row % ("(a) cfun_mold_native", t["a"] * 1e3, mold_bytes / 1e6, mold_bytes / t["a"] / 1e9),
             plain % ("(b) composed: to(float32), resize3d(order=1, clip), mold_inputs_lits", t["b"] * 1e3),
             plain % ("    its order-1 pass alone (no min/max, no clip)", t["b1"] * 1e3),
             row % ("(c) copy_ of (a)'s bytes", t["c"] * 1e3, mold_bytes / 1e6, mold_bytes / t["c"] / 1e9),
             "  (a) / order-1 pass alone: %.2fx   (a) / (b): %.2fx   (a) / (c): %.2fx   acceptance (a) < order-1 pass: %s"
             % (t["a"] / t["b1"], t["a"] / t["b"], t["a"] / t["c"], "PASS" if ok_a else "FAIL"),
             "  (a) against (b): %d of %d voxels differ, largest difference %.3g (resize3d blends in its own operation order, and"
             % (mold_diff, out.numel(), mold_max),
             "  torch divides by a reciprocal on the device: DESIGN.md section 7)", "",
             "class map [D,H,W] = %dx%dx%d uint8 -> Fortran [H,W,D] = %dx%dx%d uint8" % (rs[2], rs[0], rs[1], shape[0], shape[1], shape[2]),
             row % ("(d) cfun_map_resize", t["d"] * 1e3, map_bytes / 1e6, map_bytes / t["d"] / 1e9),
             plain % ("(e) to(float32), resize3d(order=0), round, to(uint8)", t["e"] * 1e3),
             row % ("(f) copy_ of (d)'s bytes", t["f"] * 1e3, map_bytes / 1e6, map_bytes / t["f"] / 1e9),
             "  (d) / (e): %.2fx   (d) / (f): %.2fx   maps equal: %s   acceptance (d) < (e): %s"
             % (t["d"] / t["e"], t["d"] / t["f"], map_same, "PASS" if ok_d else "FAIL"), ""]
    txt = "\n".join(lines)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    if not (ok_a and ok_d and map_same):
        sys.exit(1)


if __name__ == "__main__":
    main()
