#!/usr/bin/env python3
"""The lesion-scoring step (cfun_amd/lesions.py, cfun_amd/csrc/lesion.hip) at two map sizes, HIP-event timed:

  * cfun_rank_overlap -- the C entry with preallocated buffers, back to back, against yardstick a: a plain copy_ of the bytes
    it reads (two int32 volumes: 8 B per voxel);
  * cfun_cc_rank alone (its kernels one by one: torch.profiler, a run of its own);
  * lesions.lesion_scores as a user calls it: both sides reduced to a lesion map, labelled, ranked, overlapped, packed;
  * yardstick b: the host route this replaces -- two device-to-host copies, scipy.ndimage.label twice, a numpy count over the
    pairs of labels (16 threads allowed): a stated baseline, not credit.

The maps are synthetic: an ellipsoid liver (class 1) with about 50 ball-shaped lesions (class 2) of 2 .. 14 voxels radius; the
prediction has every lesion one voxel off along x, every fifth one missing, and one-voxel specks of class 2 on 0.3 % of the
volume.

    python tools/bench_lesion.py [--no-host] [--out profiles/lesion_pipeline.txt]
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
from cfun_amd import _lib, components, lesions  # noqa: E402
from cfun_amd._lib import ptr  # noqa: E402

CAP = 1023


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


def liver_maps(d, h, w, lesions_n=50):
    """-> (pred, label) uint8 [D,H,W] on the host."""
    rng = np.random.default_rng(0)
    z = (np.arange(d, dtype=np.float32) - d / 2) / (0.3 * d)
    y = (np.arange(h, dtype=np.float32) - h / 2) / (0.3 * h)
    x = (np.arange(w, dtype=np.float32) - w / 2) / (0.3 * w)
    label = ((z[:, None, None] ** 2 + y[None, :, None] ** 2 + x[None, None, :] ** 2) < 1.0).astype(np.uint8)
    pred = label.copy()
    for i in range(lesions_n):
        r = int(rng.integers(2, 15))
        c = [int(rng.integers(int(0.3 * n), int(0.7 * n))) for n in (d, h, w)]
        zz, yy, xx = np.ogrid[-r:r + 1, -r:r + 1, -r:r + 1]
        ball = (zz * zz + yy * yy + xx * xx) <= r * r
        sl = tuple(slice(ci - r, ci + r + 1) for ci in c)
        label[sl][ball] = 2
        if i % 5:
            sl = sl[:2] + (slice(c[2] - r + 1, c[2] + r + 2),)
            pred[sl][ball] = 2
    pred[rng.random((d, h, w), dtype=np.float32) < 0.003] = 2
    return torch.from_numpy(pred), torch.from_numpy(label)


def host_route(pred, label):
    """The host route restated: both maps down, scipy.ndimage.label twice, the distinct label pairs and their counts."""
    from scipy import ndimage
    st = ndimage.generate_binary_structure(3, 3)
    p, g = pred.cpu().numpy() == 2, label.cpu().numpy() == 2
    lp, n_pred = ndimage.label(p, structure=st)
    lg, n_ref = ndimage.label(g, structure=st)
    pairs, counts = np.unique(lg.reshape(-1).astype(np.int64) * (n_pred + 1) + lp.reshape(-1), return_counts=True)
    return n_ref, n_pred, pairs, counts


def kernel_times(fn, iters=10):
    """{kernel name: mean us} of the k_rank_* kernels over ``iters`` calls, or None where the profiler gives no device events."""
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
            if "k_rank_" in ev.key:
                name = ev.key[ev.key.index("k_rank_"):].split("(")[0].split("E")[0]
                total = getattr(ev, "device_time_total", None)
                if total is None:
                    total = getattr(ev, "cuda_time_total", 0.0)
                out[name] = out.get(name, 0.0) + total / iters
        return out or None
    except (ImportError, RuntimeError) as e:    # no profiler here: a measurement aid, the table says so when it is missing
        sys.stderr.write("bench_lesion: no per-kernel times (%s: %s)\n" % (type(e).__name__, e))
        return None


def bench_size(name, d, h, w, lines, host):
    dev = torch.device("cuda:0")
    lib = _lib.load()
    n = d * h * w
    pred_host, label_host = liver_maps(d, h, w)
    pred, label = pred_host.to(dev), label_host.to(dev)
    mp, mg = (pred == 2).to(torch.uint8), (label == 2).to(torch.uint8)
    rp, _, cp = lesions.rank_components(mp, 26, "foreground", CAP)
    rg, _, cg = lesions.rank_components(mg, 26, "foreground", CAP)
    labels_p = components.label_components(mp, 26, "foreground")
    ranks = torch.empty_like(rp)
    count = torch.empty((2,), dtype=torch.int64, device=dev)
    table = torch.empty((CAP + 2, _lib.LESION_FIELDS), dtype=torch.int64, device=dev)
    overlap = torch.empty((CAP + 2, CAP + 2), dtype=torch.int64, device=dev)
    nws = lib.cfun_lesion_workspace_bytes(d, h, w, CAP)
    ws = _lib.workspace(nws, pred)
    dims = (C.c_int32 * 3)(d, h, w)
    st = _lib.stream(pred)

    def over():
        _lib.check(lib.cfun_rank_overlap(ptr(rg), ptr(rp), dims, CAP, CAP, ptr(overlap), ptr(ws), ws.numel(), st), "rank_overlap")

    def rank():
        _lib.check(lib.cfun_cc_rank(ptr(mp), ptr(labels_p), dims, CAP, ptr(ranks), ptr(count), ptr(table), ptr(ws), ws.numel(), st),
                   "cc_rank")

    def pipeline():
        return lesions.lesion_scores(pred, label, 2, 26, (0.0, 0.5), CAP)

    src = torch.empty(8 * n, dtype=torch.uint8, device=dev).random_(0, 255)
    dst = torch.empty_like(src)

    def copy():
        dst.copy_(src)

    over()
    rank()
    torch.cuda.synchronize()
    assert int(overlap.sum()) == n and torch.equal(ranks, rp)
    t_o, t_c, t_r, t_p = [], [], [], []
    for _ in range(3):                        # alternated, so that all see the same machine state
        t_o.append(events(over, 50))
        t_c.append(events(copy, 50))
        t_r.append(events(rank, 50))
        t_p.append(events(pipeline, 10))
    t_o, t_c, t_r, t_p = min(t_o), min(t_c), min(t_r), min(t_p)
    s = lesions.LesionScores(pipeline())
    pairs = int((torch.as_tensor(s.overlap) != 0).sum())
    lines.append("%s  [D,H,W] = %dx%dx%d (%.1f M voxels), 26-connectivity, cap %d; %d reference and %d predicted lesions (%d of them "
                 "beyond cap), %d distinct pairs, %.2f %% of the voxels in a lesion of either side"
                 % (name, d, h, w, n / 1e6, CAP, int(cg[0]), int(cp[0]), int(cp[1]), pairs, 100.0 * (1.0 - float(overlap[0, 0]) / n)))
    lines.append("  working set: overlap reads 2 x %.1f MB of ranks; rank reads map %.1f MB + labels %.1f MB, writes ranks %.1f MB; "
                 "the whole pipeline holds 2 x (map + labels + ranks) = %.1f MB"
                 % (4 * n / 1e6, n / 1e6, 4 * n / 1e6, 4 * n / 1e6, 18 * n / 1e6))
    lines.append("  cfun_rank_overlap              %8.1f us   %5.2f TB/s read" % (t_o * 1e3, 8 * n / t_o / 1e9))
    lines.append("  a copy_ of %6.1f MB           %8.1f us   %5.2f TB/s read + as much written; overlap time = %.2fx the copy's"
                 % (8 * n / 1e6, t_c * 1e3, 8 * n / t_c / 1e9, t_o / t_c))
    lines.append("  cfun_cc_rank                   %8.1f us" % (t_r * 1e3))
    per = kernel_times(lambda: (rank(), over()))
    if per:
        order = ["k_rank_count", "k_rank_scan", "k_rank_roots", "k_rank_assign", "k_rank_overlap"]
        lines.append("  per kernel (profiler, a run of its own): " + ", ".join("%s %.1f us" % (p[7:], per[p]) for p in order if p in per))
    else:
        lines.append("  per kernel: not measured (the profiler returned no device events)")
    lines.append("  lesion_scores, both sides      %8.1f us   (2 x map, label, rank; overlap; pack) = %.1fx the copy's"
                 % (t_p * 1e3, t_p / t_c))
    if host:
        torch.set_num_threads(16)
        t_h = None
        for _ in range(2 if n < 3e7 else 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n_ref, n_pred, hp, hc = host_route(pred, label)
            t = time.perf_counter() - t0
            t_h = t if t_h is None else min(t_h, t)
        assert (n_ref, n_pred) == (s.n_ref, s.n_pred) and int(hc.sum()) == n, "the device and the host route disagree"
        lines.append("  b host route, transfers in     %8.1f ms   device pipeline is %.0fx faster (scipy + numpy, 16 threads allowed: a "
                     "stated baseline, not credit)" % (t_h * 1e3, t_h / (t_p * 1e-3)))
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-host", action="store_true", help="skip the host baseline")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lesion needs a GPU: nothing here is measured on the host but the stated baseline"
    lines = ["lesion scoring on %s, HIP events, back-to-back calls, best of 3 x 50 (alternated with the copy; lesion_scores 3 x 10)"
             % torch.cuda.get_device_name(0), ""]
    bench_size("lits 320", 192, 320, 320, lines, not args.no_host)
    bench_size("lits 512", 256, 512, 512, lines, not args.no_host)
    txt = "\n".join(lines)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
