#!/usr/bin/env python3
"""The ball morphology (cfun_amd/morphology.py, cfun_amd/csrc/morph.hip) at two map sizes, HIP-event timed:

  * cfun_morph_apply -- the C entry with preallocated buffers, back to back: erode and open at 1, 2 and 3 mm; the heart map by
    class (K = 8: seven groups, unit spacing), the LiTS map by class (K = 3: two groups) at the LiTS mean spacing, and one class
    alone; the kernels one by one (torch.profiler, a run of its own);
  * yardstick a: a plain copy_ of the bytes one group's erosion must touch at least once -- the uint8 map in, the uint8 map out:
    2 B per voxel;
  * yardstick b: cfun_surface_field on the same volume and class: the same three sweeps without a cut-off, through a float32
    field (surface.hip, which this tool only calls);
  * yardstick c: the host route this replaces -- device-to-host copy, scipy.ndimage.binary_erosion / binary_dilation per class
    with the same ball, copy back (16 threads allowed): a stated baseline, not credit.

The map is bench_cc's synthetic organ: an ellipsoid in bands of classes with 3 % of its voxels knocked out at random and one-voxel
specks on the background -- what an opening is for.

    python tools/bench_morph.py [--no-host] [--out profiles/morph_pipeline.txt]
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
from bench_cc import events, organ  # noqa: E402
from cfun_amd import _lib  # noqa: E402
from cfun_amd._lib import ptr  # noqa: E402

KERNELS = ["k_morph_x", "k_morph_y", "k_morph_z", "k_morph_copy"]
LITS = (1.50625819, 0.79272507, 0.79272507)
OPS = {"erode": _lib.MORPH_ERODE, "open": _lib.MORPH_OPEN}


def squares(spacing, radius):
    s2 = [float(np.float32(np.float64(v) * np.float64(v))) for v in spacing]
    return (C.c_float * 3)(*s2), float(np.float32(np.float64(radius) * np.float64(radius)))


def ball(spacing, radius):
    """The structuring element by the float32 rule of include/cfun_morph.h."""
    f = np.float32
    s2 = [f(np.float64(v) * np.float64(v)) for v in spacing]
    r2 = f(np.float64(radius) * np.float64(radius))
    reach = [int(np.floor(radius / v)) + 1 for v in spacing]
    dz, dy, dx = np.meshgrid(*[np.arange(-r, r + 1) for r in reach], indexing="ij")
    t = [(o.astype(np.int64) ** 2).astype(f) * a for o, a in zip((dz, dy, dx), s2)]
    return ((t[2] + t[1]).astype(f) + t[0]).astype(f) <= r2


def host_morph(pred, classes, op, b):
    """The host route restated: scipy per class on the input map, cleared where the result is not."""
    from scipy import ndimage
    out = pred.copy()
    for c in classes:
        obj = pred == c
        res = ndimage.binary_erosion(obj, structure=b, border_value=0)
        if op == "open":
            res = ndimage.binary_dilation(res, structure=b)
        out[obj & ~res] = 0
    return out


def kernel_times(fn, iters=10):
    """{kernel name: mean us per call} of the k_morph_* kernels, or None where the profiler gives no device events."""
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
        sys.stderr.write("bench_morph: no per-kernel times (%s: %s)\n" % (type(e).__name__, e))
        return None


def bench_size(name, d, h, w, k, spacing, one, lines, host):
    dev = torch.device("cuda:0")
    lib = _lib.load()
    n = d * h * w
    pred_host = organ(d, h, w, k)
    pred = pred_host.to(dev)
    out = torch.empty_like(pred)
    stats = torch.empty((k, 2), dtype=torch.int64, device=dev)
    nws = lib.cfun_morph_workspace_bytes(d, h, w, k)
    ws = _lib.workspace(nws, pred)
    surface = torch.empty_like(pred)
    field = torch.empty((d, h, w), dtype=torch.float32, device=dev)
    sws = _lib.workspace(0, pred)
    dims = (C.c_int32 * 3)(d, h, w)
    st = _lib.stream(pred)
    every = (1 << k) - 2

    def morph(op, radius, bits):
        s2, r2 = squares(spacing, radius)
        _lib.check(lib.cfun_morph_apply(ptr(pred), dims, k, _lib.CC_CLASS, OPS[op], bits, s2, r2, 0, 1, ptr(out), ptr(stats), ptr(ws),
                                        ws.numel(), st), "morph_apply")

    s2_field, _ = squares(spacing, 1.0)

    def surface_field():
        _lib.check(lib.cfun_surface_field(ptr(pred), dims, one, s2_field, ptr(surface), ptr(field), ptr(sws), sws.numel(), st),
                   "surface_field")

    src = torch.empty(n, dtype=torch.uint8, device=dev).random_(0, 255)
    dst = torch.empty_like(src)

    def copy():
        dst.copy_(src)

    lines.append("%s  [D,H,W] = %dx%dx%d (%.1f M voxels), K = %d, by class, spacing (%s) mm; class %d alone holds %.1f %% of the voxels"
                 % (name, d, h, w, n / 1e6, k, ", ".join("%g" % v for v in spacing), one, 100.0 * float((pred_host == one).sum()) / n))
    lines.append("  working set: map 2 x %.1f MB + workspace %.1f MB = %.1f MB" % (n / 1e6, nws / 1e6, (2 * n + nws) / 1e6))
    variants = [(op, r, bits) for bits in (every, 1 << one) for op in ("erode", "open") for r in (1.0, 2.0, 3.0)]
    fns = [lambda v=v: morph(*v) for v in variants]
    for f in fns + [surface_field, copy]:
        f()
    torch.cuda.synchronize()
    t_m, t_s, t_c = [[] for _ in variants], [], []
    for _ in range(3):                          # alternated, so that all see the same machine state
        for i, f in enumerate(fns):
            t_m[i].append(events(f, 20))
        t_s.append(events(surface_field, 20))
        t_c.append(events(copy, 20))
    t_m, t_s, t_c = [min(t) for t in t_m], min(t_s), min(t_c)
    lines.append("  a a copy_ of %5.1f MB (2 B per voxel moved)        %9.1f us   %5.2f TB/s read + as much written" % (n / 1e6, t_c * 1e3, n / t_c / 1e9))
    lines.append("  b cfun_surface_field, class %d                      %9.1f us   (surface pass + three unbounded sweeps, float32 field)" % (one, t_s * 1e3))
    for (op, r, bits), f, t in zip(variants, fns, t_m):
        groups = bin(bits).count("1")
        b = ball(spacing, r)
        f()
        torch.cuda.synchronize()
        s = stats.cpu().numpy()
        lines.append("  cfun_morph_apply  %-5s %g mm (%3d offsets) %-13s %9.1f us   %8.1f us per group = %5.2fx b, %5.1fx a; %d voxels cleared"
                     % (op, r, int(b.sum()), "every class" if bits == every else "class %d alone" % one, t * 1e3, t * 1e3 / groups,
                        t / groups / t_s, t / groups / t_c, int(s[:, 0].sum())))
        sys.stderr.write(lines[-1] + "\n")
        sys.stderr.flush()
        if bits != every:
            per = kernel_times(f)
            if per:
                lines.append("      per kernel and call (profiler, a run of its own): " + ", ".join("%s %.1f us" % (p[8:], per[p]) for p in KERNELS if p in per))
            else:
                lines.append("      per kernel: not measured (the profiler returned no device events)")
        if host and bits != every and r in (1.0, 3.0):
            torch.set_num_threads(16)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            back = torch.from_numpy(host_morph(pred.cpu().numpy(), [one], op, b)).to(dev)
            torch.cuda.synchronize()
            t_h = time.perf_counter() - t0
            assert torch.equal(back, out), "the device and the host route disagree"
            lines.append("      c host route, transfers in                   %9.1f ms   the device call is %.0fx faster (scipy, one run: a stated "
                         "baseline, not credit)" % (t_h * 1e3, t_h / (t * 1e-3)))
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-host", action="store_true", help="skip the host baseline")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_morph needs a GPU: nothing here is measured on the host but the stated baseline"
    lines = ["ball morphology on %s, HIP events, back-to-back calls, best of 3 x 20 (alternated with the yardsticks)"
             % torch.cuda.get_device_name(0), ""]
    bench_size("heart", 192, 320, 320, 8, (1.0, 1.0, 1.0), 4, lines, not args.no_host)
    bench_size("lits ", 256, 320, 320, 3, LITS, 1, lines, not args.no_host)
    txt = "\n".join(lines)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
