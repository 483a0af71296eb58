#!/usr/bin/env python3
"""The surface-distance step (cfun_amd/evaluate.py: surface_distances; cfun_amd/csrc/surface.hip) at two map sizes, HIP-event
timed:

  * cfun_surface_stats -- the C entry with a preallocated workspace, back to back, all classes; and the kernels one by one
    (torch.profiler, a run of its own);
  * yardstick a: a plain copy_ of the bytes the passes of one class touch -- the surface pass 4 B per voxel, the x sweep 10, the
    y and z sweeps 16 each, the gather 10, two selection passes 10 each: 76 B per voxel, a copy_ of 38 -- times the classes;
  * yardstick b: the host route this replaces -- the map to the host, per class and direction the erosion surface and
    scipy.ndimage.distance_transform_edt, the gathers, the percentile (16 threads allowed): a stated baseline, not credit;
  * one detect_original at the same size (heart configuration, seeded weights), for the share a user feels;
  * the data-dependent ends of the pruned scan, one class each: a class that is absent (every line +inf: skipped), and one
    surface voxel in a corner (every line finite and far: the farthest scans there are); and the same maps after
    clean_components, without their specks.

The prediction is bench_cc's synthetic organ; the label is the same organ moved by (2, 3, -4) voxels.

    python tools/bench_surface.py [--no-host] [--no-detect] [--iters 50] [--out profiles/surface_pipeline.txt]
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
from cfun_amd import _lib, evaluate  # noqa: E402
from cfun_amd._lib import ptr  # noqa: E402

BYTES_PER_VOXEL = 76          # read + written per class, see above
# (label, the spellings a profiler may give the kernel: demangled or mangled)
KERNELS = [("surface", ("k_surface",)), ("sweep x", ("k_sweep_x",)), ("sweep y", ("k_sweep<1>", "k_sweepILi1")),
           ("sweep z", ("k_sweep<2>", "k_sweepILi2")), ("gather", ("k_gather",)), ("finish", ("k_finish",)), ("hist", ("k_hist",)),
           ("pick", ("k_pick",))]


def host_scores(pred, label, k, spacing, q):
    """The host route restated: per class both erosion surfaces, both exact EDTs, the gathers and the scores."""
    from scipy import ndimage
    st = ndimage.generate_binary_structure(3, 1)
    out = np.full((k - 1, 3), np.nan)
    for c in range(1, k):
        a, b = pred == c, label == c
        sa, sb = a & ~ndimage.binary_erosion(a, st), b & ~ndimage.binary_erosion(b, st)
        if not sa.any() or not sb.any():
            continue
        dl = ndimage.distance_transform_edt(~sb, sampling=spacing)[sa]
        dp = ndimage.distance_transform_edt(~sa, sampling=spacing)[sb]
        out[c - 1] = max(dl.max(), dp.max()), np.percentile(np.concatenate([dl, dp]), q), 0.5 * (dl.mean() + dp.mean())
    return out


def kernel_times(fn, iters):
    """{kernel: mean us per call of fn} over ``iters`` calls, or None where the profiler gives no device events."""
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
            for label, spellings in KERNELS:
                if any(sp in ev.key for sp in spellings):          # (only cfun_surface_stats runs under the profiler)
                    total = getattr(ev, "device_time_total", None)
                    if total is None:
                        total = getattr(ev, "cuda_time_total", 0.0)
                    out[label] = out.get(label, 0.0) + total / iters
        return out or None
    except Exception as e:                      # a measurement aid: the table says so when it is missing
        sys.stderr.write("bench_surface: no per-kernel times (%s: %s)\n" % (type(e).__name__, e))
        return None


def bench_size(name, d, h, w, k, spacing, lines, host, detect, iters):
    dev = torch.device("cuda:0")
    lib = _lib.load()
    n = d * h * w
    pred_host = organ(d, h, w, k)
    label_host = torch.roll(pred_host, shifts=(2, 3, -4), dims=(0, 1, 2)).contiguous()
    pred, label = pred_host.to(dev), label_host.to(dev)
    nws = lib.cfun_surface_workspace_bytes(d, h, w, k)
    ws = _lib.workspace(nws, pred)
    dims = (C.c_int32 * 3)(d, h, w)
    s2 = evaluate._spacing2("bench_surface", spacing)
    st = _lib.stream(pred)
    stats = torch.empty((k, _lib.SURFACE_STATS_FIELDS), dtype=torch.int64, device=dev)

    def run(p=pred, lab=label, kk=k, out=stats):
        _lib.check(lib.cfun_surface_stats(ptr(p), ptr(lab), dims, kk, s2, 0.95, ptr(out), ptr(ws), ws.numel(), st), "surface_stats")

    nbytes = (BYTES_PER_VOXEL // 2) * n
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(0, 255)
    dst = torch.empty_like(src)

    def copy():
        dst.copy_(src)

    run()
    torch.cuda.synchronize()
    sc = evaluate.SurfaceScores(stats)
    t_s, t_c = [], []
    for _ in range(3):                        # alternated, so that both see the same machine state
        t_s.append(events(run, iters))
        t_c.append(events(copy, iters))
    t_s, t_c = min(t_s), min(t_c)
    lines.append("%s  [D,H,W] = %dx%dx%d (%.1f M voxels), K = %d, spacing %s mm; surface voxels per class (pred): %s"
                 % (name, d, h, w, n / 1e6, k, spacing, sc.n_pred.tolist()))
    lines.append("  scores: hausdorff %s, hd95 %s, assd %s" % tuple(np.array2string(v, precision=3) for v in (sc.hausdorff, sc.hd_percentile,
                                                                                                               sc.assd)))
    lines.append("  working set per class: 2 maps %.1f MB + workspace %.1f MB (2 byte surfaces, 2 float32 fields) = %.1f MB"
                 % (2 * n / 1e6, nws / 1e6, (2 * n + nws) / 1e6))
    lines.append("  cfun_surface_stats, %d classes  %9.1f us   %.1f us per class" % (k - 1, t_s * 1e3, t_s * 1e3 / (k - 1)))
    per = kernel_times(run, 5)
    if per:
        lines.append("  per kernel and call (profiler, a run of its own): " + ", ".join("%s %.1f us" % (p, per[p]) for p, _ in KERNELS if p in per))
    else:
        lines.append("  per kernel: not measured (the profiler returned no device events)")
    lines.append("  a copy_ of %6.1f MB x %d       %9.1f us   %5.2f TB/s read + as much written; pipeline time = %.1fx the copies'"
                 % (nbytes / 1e6, k - 1, t_c * 1e3 * (k - 1), nbytes / t_c / 1e9, t_s / (t_c * (k - 1))))
    # the two data-dependent ends, one class (K = 2)
    one = torch.empty((2, _lib.SURFACE_STATS_FIELDS), dtype=torch.int64, device=dev)
    zeros = torch.zeros_like(pred)
    corner = torch.zeros_like(pred)
    corner[0, 0, 0] = 1
    t_abs = min(events(lambda: run(zeros, zeros, 2, one), max(iters // 5, 3)) for _ in range(3))
    t_cor = min(events(lambda: run(corner, corner, 2, one), max(iters // 5, 3)) for _ in range(3))
    lines.append("  one class, absent (all lines +inf)   %9.1f us;   one surface voxel in a corner (longest scans) %9.1f us"
                 % (t_abs * 1e3, t_cor * 1e3))
    # the same maps without the specks (the largest component of every class, as a Postprocess leaves them): the scans are
    # as long as the in-plane distance to the organ, not to the nearest speck
    from cfun_amd import components
    cp, cl = components.clean_components(pred, k)[0], components.clean_components(label, k)[0]
    two = torch.empty_like(stats)
    t_cln = min(events(lambda: run(cp, cl, k, two), max(iters // 2, 3)) for _ in range(3))
    lines.append("  the same maps cleaned (largest component per class, no specks), %d classes  %9.1f us   %.1f us per class"
                 % (k - 1, t_cln * 1e3, t_cln * 1e3 / (k - 1)))
    if host:
        torch.set_num_threads(16)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = host_scores(pred.cpu().numpy(), label.cpu().numpy(), k, spacing, 95.0)
        t_h = time.perf_counter() - t0
        want = np.stack([sc.hausdorff, sc.hd_percentile, sc.assd], axis=1)
        assert np.allclose(got, want, rtol=1e-5, equal_nan=True), "the device and the host route disagree:\n%s\n%s" % (got, want)
        lines.append("  b host route, transfers in      %9.1f ms   device pipeline is %.0fx faster (scipy, 16 threads allowed: a stated "
                     "baseline, not credit)" % (t_h * 1e3, t_h / (t_s * 1e-3)))
    if detect:
        try:
            t_d, found = detect_time(h, w, d)
            lines.append("  one detect_original             %9.1f ms   (heart configuration, seeded weights, %s); the step is %.2f %% of it"
                         % (t_d * 1e3, "with detections" if found else "NO detection: the mask branch did not run", 100 * t_s * 1e-3 / t_d))
        except Exception as e:
            lines.append("  one detect_original: not measured (%s: %s)" % (type(e).__name__, str(e)[:200]))
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-host", action="store_true", help="skip the host baseline")
    ap.add_argument("--no-detect", action="store_true", help="skip the detect_original timing")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_surface needs a GPU: nothing here is measured on the host but the stated baseline"
    lines = ["surface distances on %s, HIP events, back-to-back calls, best of 3 x %d (alternated with the copy)"
             % (torch.cuda.get_device_name(0), args.iters), ""]
    bench_size("heart", 192, 320, 320, 8, (1.0, 1.0, 1.0), lines, not args.no_host, not args.no_detect, args.iters)
    bench_size("lits ", 256, 320, 320, 3, (2.5, 0.78, 0.78), lines, not args.no_host, False, args.iters)
    txt = "\n".join(lines)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
