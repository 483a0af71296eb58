#!/usr/bin/env python3
"""The connected-component step (cfun_amd/components.py, cfun_amd/csrc/cc.hip) at two map sizes, HIP-event timed:

  * cfun_cc_label + cfun_cc_filter -- the C entries with preallocated buffers, back to back (26-connectivity, per class, largest
    component only), together and each alone, and the kernels one by one (torch.profiler, a run of its own);
  * yardstick a: a plain copy_ of the bytes the passes must touch at least once -- the uint8 map in, the int32 labels out and in,
    the uint8 map out: 10 B per voxel;
  * yardstick b: the host route this replaces -- device-to-host copy, scipy.ndimage.label per class + bincount + filter
    (16 threads allowed), copy back: a stated baseline, not credit;
  * one detect_original at the same size (heart configuration, seeded weights), for the share a user feels.

The map is a synthetic organ: one ellipsoid in bands of classes 1 .. K-1 plus scattered one-voxel specks, ~90 % background.

    python tools/bench_cc.py [--no-host] [--no-detect] [--out profiles/cc_pipeline.txt]
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
from cfun_amd import _lib  # noqa: E402
from cfun_amd._lib import ptr  # noqa: E402

CONN, MODE = 26, _lib.CC_CLASS


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


def organ(d, h, w, k):
    """uint8 [D,H,W]: an ellipsoid (semi-axes 0.3 of each extent: ~11 % of the box) in k-1 bands of classes along y, minus 3 % of
    its voxels knocked out at random, plus one-voxel specks of a random class on 0.3 % of the background."""
    g = torch.Generator().manual_seed(0)
    z = (torch.arange(d, dtype=torch.float32) - d / 2) / (0.3 * d)
    y = (torch.arange(h, dtype=torch.float32) - h / 2) / (0.3 * h)
    x = (torch.arange(w, dtype=torch.float32) - w / 2) / (0.3 * w)
    inside = (z[:, None, None] ** 2 + y[None, :, None] ** 2 + x[None, None, :] ** 2) < 1.0
    band = ((torch.arange(h) * (k - 1)) // h + 1).to(torch.uint8)[None, :, None].expand(d, h, w)
    pred = torch.where(inside, band, torch.zeros((), dtype=torch.uint8))
    r = torch.rand((d, h, w), generator=g)
    pred[inside & (r < 0.03)] = 0
    speck = ~inside & (r < 0.003)
    pred[speck] = torch.randint(1, k, (int(speck.sum()),), generator=g, dtype=torch.uint8)
    return pred.contiguous()


def host_clean(pred, k):
    """The host route restated: per class scipy.ndimage.label (26-connectivity), bincount, keep the largest (first of equals)."""
    from scipy import ndimage
    st = ndimage.generate_binary_structure(3, 3)
    out = np.zeros_like(pred)
    for c in range(1, k):
        lab, n = ndimage.label(pred == c, structure=st)
        if n == 0:
            continue
        sizes = np.bincount(lab.reshape(-1))
        sizes[0] = 0
        out[lab == int(np.argmax(sizes))] = c
    return out


def kernel_times(fn, iters=10):
    """{kernel name: mean us} of the k_cc_* kernels over ``iters`` calls, or None where the profiler gives no device events."""
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
            if "k_cc_" in ev.key:
                name = ev.key[ev.key.index("k_cc_"):].split("(")[0].split("E")[0]
                total = getattr(ev, "device_time_total", None)
                if total is None:
                    total = getattr(ev, "cuda_time_total", 0.0)
                out[name] = out.get(name, 0.0) + total / iters
        return out or None
    except Exception as e:                      # a measurement aid: the table says so when it is missing
        sys.stderr.write("bench_cc: no per-kernel times (%s: %s)\n" % (type(e).__name__, e))
        return None


def detect_time(h, w, d):
    """Seconds of one detect_original on a seeded heart network at this volume size (best of 3), and whether it detected."""
    from cfun_amd import config, evaluate, step
    cfg = config.heart_config("finetune", h, w, d)
    cfg.DETECTION_MIN_CONFIDENCE = 0.0
    torch.manual_seed(0)
    net = step.CFUNHotPath(cfg).to("cuda:0")
    image = torch.randn((h, w, d, 1), generator=torch.Generator().manual_seed(1)) * 300.0 + 100.0
    best, res = None, None
    with torch.no_grad():
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = evaluate.detect_original(net, image)
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            best = t if best is None else min(best, t)
    return best, not res["empty"]


def bench_size(name, d, h, w, k, lines, host, detect):
    dev = torch.device("cuda:0")
    lib = _lib.load()
    n = d * h * w
    pred_host = organ(d, h, w, k)
    pred = pred_host.to(dev)
    labels = torch.empty((d, h, w), dtype=torch.int32, device=dev)
    out = torch.empty_like(pred)
    stats = torch.empty((k, 3), dtype=torch.int64, device=dev)
    nws = lib.cfun_cc_workspace_bytes(d, h, w, k)
    ws = _lib.workspace(nws, pred)
    dims = (C.c_int32 * 3)(d, h, w)
    st = _lib.stream(pred)

    def label():
        _lib.check(lib.cfun_cc_label(ptr(pred), dims, CONN, MODE, ptr(labels), ptr(ws), ws.numel(), st), "cc_label")

    def filt():
        _lib.check(lib.cfun_cc_filter(ptr(pred), ptr(labels), dims, k, MODE, 1, 0, ptr(out), ptr(stats), ptr(ws), ws.numel(), st),
                   "cc_filter")

    def both():
        label()
        filt()

    nbytes = 10 * n
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(0, 255)
    dst = torch.empty_like(src)

    def copy():
        dst.copy_(src)

    both()
    torch.cuda.synchronize()
    s = stats.cpu().numpy()
    t_b, t_l, t_f, t_c = [], [], [], []
    for _ in range(3):                        # alternated, so that all see the same machine state
        t_b.append(events(both, 50))
        t_c.append(events(copy, 50))
        t_l.append(events(label, 50))
        t_f.append(events(filt, 50))
    t_b, t_l, t_f, t_c = min(t_b), min(t_l), min(t_f), min(t_c)
    bg = float((pred_host == 0).sum()) / n
    lines.append("%s  [D,H,W] = %dx%dx%d (%.1f M voxels), K = %d, 26-connectivity, per class, largest only; %.1f %% background, "
                 "%d components, %d voxels removed" % (name, d, h, w, n / 1e6, k, 100 * bg, int(s[:, 0].sum()), int(s[:, 2].sum())))
    lines.append("  working set: map 2 x %.1f MB + labels %.1f MB + workspace %.1f MB = %.1f MB"
                 % (n / 1e6, 4 * n / 1e6, nws / 1e6, (6 * n + nws) / 1e6))
    lines.append("  cfun_cc_label + cfun_cc_filter %8.1f us   (alone: label %.1f us, filter %.1f us)" % (t_b * 1e3, t_l * 1e3, t_f * 1e3))
    per = kernel_times(both)
    if per:
        order = ["k_cc_local", "k_cc_seam", "k_cc_flatten", "k_cc_size", "k_cc_select", "k_cc_finish", "k_cc_write"]
        lines.append("  per kernel (profiler, a run of its own): " + ", ".join("%s %.1f us" % (p[5:], per[p]) for p in order if p in per))
        lines.append("  (the size workspace's memset is the rest of the filter)")
    else:
        lines.append("  per kernel: not measured (the profiler returned no device events)")
    lines.append("  a copy_ of %6.1f MB           %8.1f us   %5.2f TB/s read + as much written; pipeline time = %.1fx the copy's"
                 % (nbytes / 1e6, t_c * 1e3, nbytes / t_c / 1e9, t_b / t_c))
    if host:
        torch.set_num_threads(16)
        t_h = None
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            back = torch.from_numpy(host_clean(pred.cpu().numpy(), k)).to(dev)
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            t_h = t if t_h is None else min(t_h, t)
        assert torch.equal(back, out), "the device and the host route disagree"
        lines.append("  b host route, transfers in     %8.1f ms   device pipeline is %.0fx faster (scipy, 16 threads allowed: a stated "
                     "baseline, not credit)" % (t_h * 1e3, t_h / (t_b * 1e-3)))
    if detect:
        try:
            t_d, found = detect_time(h, w, d)
            lines.append("  one detect_original            %8.1f ms   (heart configuration, seeded weights, %s); the step is %.2f %% of it"
                         % (t_d * 1e3, "with detections" if found else "NO detection: the mask branch did not run", 100 * t_b * 1e-3 / t_d))
        except Exception as e:
            lines.append("  one detect_original: not measured (%s: %s)" % (type(e).__name__, str(e)[:200]))
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-host", action="store_true", help="skip the host baseline")
    ap.add_argument("--no-detect", action="store_true", help="skip the detect_original timing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_cc needs a GPU: nothing here is measured on the host but the stated baseline"
    lines = ["connected components on %s, HIP events, back-to-back calls, best of 3 x 50 (alternated with the copy)"
             % torch.cuda.get_device_name(0), ""]
    bench_size("heart", 192, 320, 320, 8, lines, not args.no_host, not args.no_detect)
    bench_size("lits ", 256, 320, 320, 3, lines, not args.no_host, False)
    txt = "\n".join(lines)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
