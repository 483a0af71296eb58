#!/usr/bin/env python3
"""The hole-filling step (cfun_amd/components.py fill_holes, cfun_amd/csrc/fill.hip) at two map sizes, HIP-event timed:

  * cfun_fill_holes -- the C entry with preallocated buffers, back to back: the heart map by class (K = 8: seven labellings of a
    complement), the LiTS map by foreground (one labelling) in 3-D and slice by slice (axis 0), and the kernels one by one
    (torch.profiler, a run of its own);
  * yardstick a: cfun_cc_label + cfun_cc_filter on the same map (26-connectivity, the same grouping, largest only): the step
    that runs just before, built on the same forest, labelling the ~11 % of the voxels that are object where the fill labels
    the ~89 % that are not;
  * yardstick b: a plain copy_ of the bytes ONE labelling must touch at least once -- the uint8 map in, the int32 labels out and
    in, the uint8 map out: 10 B per voxel;
  * yardstick c: the host route this replaces -- device-to-host copy, scipy.ndimage.binary_fill_holes per group, copy back
    (16 threads allowed): a stated baseline, not credit;
  * one detect_original at the heart size (seeded weights), for the share a user feels.

The map is bench_cc's synthetic organ -- an ellipsoid in bands of classes with 3 % of its voxels knocked out at random: every one
of those a cavity -- plus planted ball-shaped cavities and one large cavity with a pinhole to the outside along z, which is no
hole in 3-D and one in nearly every axial slice.  The table states how many cavities each call found.

    python tools/bench_fill.py [--no-host] [--no-detect] [--out profiles/fill_pipeline.txt]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_cc import detect_time, events, organ  # noqa: E402
from cfun_amd import _lib  # noqa: E402
from cfun_amd._lib import ptr  # noqa: E402

KERNELS = ["k_fill_local", "k_fill_seam", "k_fill_flatten", "k_fill_mark", "k_fill_write", "k_fill_finish"]


def planted(d, h, w, k):
    """bench_cc.organ with 24 ball-shaped cavities (radius 2 .. 6) inside the ellipsoid, and one of radius 12 at its centre with a
    one-voxel shaft to the outside along z.  Returns (map, number of balls)."""
    pred = organ(d, h, w, k)
    rng = np.random.default_rng(0)

    def carve(cz, cy, cx, r):
        box = pred[cz - r:cz + r + 1, cy - r:cy + r + 1, cx - r:cx + r + 1]
        assert tuple(box.shape) == (2 * r + 1,) * 3, "the ball leaves the volume"
        o = torch.arange(-r, r + 1)
        box[(o[:, None, None] ** 2 + o[None, :, None] ** 2 + o[None, None, :] ** 2) <= r * r] = 0

    balls = 0
    while balls < 24:
        u = rng.normal(size=3)
        u *= rng.random() ** (1 / 3) * 0.2 / np.linalg.norm(u)                      # within 0.2 of each extent: well inside
        cz, cy, cx, r = int(d / 2 + u[0] * d), int(h / 2 + u[1] * h), int(w / 2 + u[2] * w), int(rng.integers(2, 7))
        if abs(cz - d // 2) < 20 and abs(cy - h // 2) < 20 and abs(cx - w // 2) < 20:
            continue                                                                # (keep clear of the cavity with the shaft)
        carve(cz, cy, cx, r)
        balls += 1
    carve(d // 2, h // 2, w // 2, 12)
    pred[: d // 2, h // 2, w // 2] = 0
    return pred.contiguous(), balls


def host_fill(pred, k, by, conn, axis, value):
    """The host route restated: scipy.ndimage.binary_fill_holes per group, descending, writing where the map is still 0."""
    from scipy import ndimage
    assert axis in (None, 0)
    st = ndimage.generate_binary_structure(3 if axis is None else 2, 1 if conn in (6, 4) else 3)
    out = pred.copy()
    groups = [(pred != 0, value)] if by == "foreground" else [(pred == c, c) for c in range(k - 1, 0, -1)]
    for obj, v in groups:
        if axis is None:
            full = ndimage.binary_fill_holes(obj, structure=st)
        else:
            full = np.stack([ndimage.binary_fill_holes(obj[z], structure=st) for z in range(obj.shape[0])])
        out[full & ~obj & (pred == 0) & (out == 0)] = v
    return out


def kernel_times(fn, iters=10):
    """{kernel name: mean us per call} of the k_fill_* kernels, or None where the profiler gives no device events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            for name in KERNELS:
                if name in ev.key:
                    total = getattr(ev, "device_time_total", None)
                    if total is None:
                        total = getattr(ev, "cuda_time_total", 0.0)
                    out[name] = out.get(name, 0.0) + total / iters
        return out or None
    except Exception as e:                      # a measurement aid: the table says so when it is missing
        sys.stderr.write("bench_fill: no per-kernel times (%s: %s)\n" % (type(e).__name__, e))
        return None


def bench_size(name, d, h, w, k, by, variants, lines, host, detect):
    dev = torch.device("cuda:0")
    lib = _lib.load()
    n = d * h * w
    pred_host, balls = planted(d, h, w, k)
    pred = pred_host.to(dev)
    mode = _lib.CC_FOREGROUND if by == "foreground" else _lib.CC_CLASS
    groups = 1 if by == "foreground" else k - 1
    out = torch.empty_like(pred)
    stats = torch.empty((k, 2), dtype=torch.int64, device=dev)
    nws = lib.cfun_fill_workspace_bytes(d, h, w, k)
    ws = _lib.workspace(nws, pred)
    labels = torch.empty((d, h, w), dtype=torch.int32, device=dev)
    cc_out = torch.empty_like(pred)
    cc_stats = torch.empty((k, 3), dtype=torch.int64, device=dev)
    cc_ws = _lib.workspace(lib.cfun_cc_workspace_bytes(d, h, w, k), pred)
    dims = (C.c_int32 * 3)(d, h, w)
    st = _lib.stream(pred)

    def fill(conn, axis):
        _lib.check(lib.cfun_fill_holes(ptr(pred), dims, k, mode, conn, -1 if axis is None else axis, 1, ptr(out), ptr(stats), ptr(ws),
                                       ws.numel(), st), "fill_holes")

    def cc():
        _lib.check(lib.cfun_cc_label(ptr(pred), dims, 26, mode, ptr(labels), ptr(cc_ws), cc_ws.numel(), st), "cc_label")
        _lib.check(lib.cfun_cc_filter(ptr(pred), ptr(labels), dims, k, mode, 1, 0, ptr(cc_out), ptr(cc_stats), ptr(cc_ws),
                                      cc_ws.numel(), st), "cc_filter")

    nbytes = 10 * n
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(0, 255)
    dst = torch.empty_like(src)

    def copy():
        dst.copy_(src)

    bg = float((pred_host == 0).sum()) / n
    lines.append("%s  [D,H,W] = %dx%dx%d (%.1f M voxels), K = %d, by %s: %d labelling(s) per call; %.1f %% zero voxels; planted: the "
                 "organ's 3 %% knock-outs, %d balls, 1 cavity with a shaft along z"
                 % (name, d, h, w, n / 1e6, k, by, groups, 100 * bg, balls))
    lines.append("  working set: map 2 x %.1f MB + workspace %.1f MB (labels %.1f MB) = %.1f MB"
                 % (n / 1e6, nws / 1e6, 4 * n / 1e6, (2 * n + nws) / 1e6))
    fns = [lambda c=c, a=a: fill(c, a) for c, a in variants]
    for f in fns + [cc, copy]:
        f()
    torch.cuda.synchronize()
    t_fill, t_cc, t_copy = [[] for _ in variants], [], []
    for _ in range(3):                        # alternated, so that all see the same machine state
        for i, f in enumerate(fns):
            t_fill[i].append(events(f, 50))
        t_cc.append(events(cc, 50))
        t_copy.append(events(copy, 50))
    t_fill, t_cc, t_copy = [min(t) for t in t_fill], min(t_cc), min(t_copy)
    t_first = t_fill[0]
    for (conn, axis), f, t in zip(variants, fns, t_fill):
        f()
        torch.cuda.synchronize()
        s = stats.cpu().numpy()
        what = "3-D, %d-neighbourhood" % conn if axis is None else "axis %d, %d-neighbourhood" % (axis, conn)
        lines.append("  cfun_fill_holes  %-24s %9.1f us   %.1f us per labelling; %d enclosed components, %d voxels filled"
                     % (what, t * 1e3, t * 1e3 / groups, int(s[:, 0].sum()), int(s[:, 1].sum())))
        per = kernel_times(f)
        if per:
            lines.append("    per kernel and call (profiler, a run of its own): "
                         + ", ".join("%s %.1f us" % (p[7:], per[p]) for p in KERNELS if p in per))
        else:
            lines.append("    per kernel: not measured (the profiler returned no device events)")
        if host:
            torch.set_num_threads(16)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            back = torch.from_numpy(host_fill(pred.cpu().numpy(), k, by, conn, axis, 1)).to(dev)
            torch.cuda.synchronize()
            t_h = time.perf_counter() - t0
            assert torch.equal(back, out), "the device and the host route disagree"
            lines.append("    c host route, transfers in      %9.1f ms   the device call is %.0fx faster (scipy, 16 threads allowed, one "
                         "run: a stated baseline, not credit)" % (t_h * 1e3, t_h / (t * 1e-3)))
    lines.append("  a cfun_cc_label + cfun_cc_filter         %9.1f us   (26-connectivity, by %s, largest only); the first fill above = %.1fx"
                 % (t_cc * 1e3, by, t_first / t_cc))
    lines.append("  b a copy_ of %6.1f MB                   %9.1f us   %5.2f TB/s read + as much written; one labelling of the first fill "
                 "= %.1fx the copy's" % (nbytes / 1e6, t_copy * 1e3, nbytes / t_copy / 1e9, t_first / groups / t_copy))
    if detect:
        try:
            t_d, found = detect_time(h, w, d)
            lines.append("  one detect_original                      %9.1f ms   (heart configuration, seeded weights, %s); the first fill is "
                         "%.2f %% of it" % (t_d * 1e3, "with detections" if found else "NO detection: the mask branch did not run",
                                            100 * t_first * 1e-3 / t_d))
        except Exception as e:
            lines.append("  one detect_original: not measured (%s: %s)" % (type(e).__name__, str(e)[:200]))
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-host", action="store_true", help="skip the host baseline")
    ap.add_argument("--no-detect", action="store_true", help="skip the detect_original timing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fill needs a GPU: nothing here is measured on the host but the stated baseline"
    lines = ["hole filling on %s, HIP events, back-to-back calls, best of 3 x 50 (alternated with the yardsticks)"
             % torch.cuda.get_device_name(0), ""]
    bench_size("heart", 192, 320, 320, 8, "class", [(6, None)], lines, not args.no_host, not args.no_detect)
    bench_size("lits ", 256, 320, 320, 3, "foreground", [(6, None), (4, 0)], lines, not args.no_host, False)
    txt = "\n".join(lines)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
