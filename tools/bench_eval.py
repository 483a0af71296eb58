#!/usr/bin/env python3
"""The scoring pass (cfun_amd/evaluate.py) at two label sizes, HIP-event timed:

  * cfun_seg_confusion -- the C entry with preallocated buffers, back to back, and its bytes (label + 1 B of pred per voxel);
  * yardstick 1: the same counts by torch on the same device -- the label made contiguous in pred's order, then
    torch.bincount(label.long() * (K+1) + pred.long(), minlength=(K+1)**2);
  * yardstick 2: a plain copy_ of the same number of bytes (it reads them and writes them again);
  * yardstick 3 (first size only): the reference's way on the host -- two float64 one-hot arrays [H,W,D,K-1], cast to float32,
    the diagonal of their [K-1,V] x [V,K-1] product -- in numpy on 16 threads: a stated baseline, not credit.

    python tools/bench_eval.py [--no-host] [--out profiles/eval_pipeline.txt]
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
from cfun_amd import _lib, evaluate  # noqa: E402
from cfun_amd._lib import ptr  # noqa: E402
from cfun_amd.ops import ptr_raw  # noqa: E402

K = 8


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


def volumes(h, w, d, dtype, dev):
    """An [H,W,D] label (z fastest) that is ~92 % background with a blob of classes 1 .. K-1, and a [D,H,W] prediction that agrees
    with it on most of the blob."""
    g = torch.Generator().manual_seed(0)
    label = torch.zeros((h, w, d), dtype=torch.uint8)
    ys, xs, zs = slice(h // 4, 3 * h // 4), slice(w // 4, 3 * w // 4), slice(d // 3, 2 * d // 3)
    label[ys, xs, zs] = (torch.arange(h // 2)[:, None, None] * (K - 1) // (h // 2) + 1).to(torch.uint8)      # bands of classes
    pred = label.permute(2, 0, 1).contiguous().clone()
    flip = torch.rand(pred.shape, generator=g) < 0.02
    pred[flip] = torch.randint(0, K, (int(flip.sum()),), generator=g, dtype=torch.uint8)
    return label.to(dtype).to(dev), pred.to(dev)


def host_onehot_iou(label, pred, k):
    """The reference's route (heart_main.py:321-330 + utils.compute_per_class_mask_iou), restated: float64 one-hots, float32 cast,
    the diagonal of a matrix product."""
    gt = np.zeros(label.shape + (k - 1,))
    pm = np.zeros(label.shape + (k - 1,))
    for j in range(k - 1):
        gt[..., j][label == j + 1] = 1
        pm[..., j][pred == j + 1] = 1
    gt = (gt > .5).reshape(-1, k - 1).astype(np.float32)
    pm = (pm > .5).reshape(-1, k - 1).astype(np.float32)
    a1, a2 = gt.sum(axis=0), pm.sum(axis=0)
    inter = np.diagonal(gt.T @ pm)
    return inter / (a1 + a2 - inter + 1e-6)


def bench_size(name, h, w, d, dtype, lines, host):
    dev = torch.device("cuda:0")
    lib = _lib.load()
    n = h * w * d
    label, pred = volumes(h, w, d, dtype, dev)
    view = label.permute(2, 0, 1)
    assert view.stride(0) == 1
    nbytes = n * (label.element_size() + 1)
    counts = torch.empty((K + 1, K + 1), dtype=torch.int64, device=dev)
    ws = _lib.workspace(lib.cfun_seg_confusion_workspace_bytes(d, h, w, K), pred)
    i64, i32 = C.c_int64 * 3, C.c_int32 * 3
    st = _lib.stream(pred)
    code = 0 if dtype == torch.uint8 else 1

    def kernel():
        _lib.check(lib.cfun_seg_confusion(ptr(pred), ptr_raw(view), code, i64(*view.stride()), i32(d, h, w), K, ptr(counts), ptr(ws),
                                          ws.numel(), st), "seg_confusion")

    def by_torch():
        return torch.bincount((view.contiguous().long() * (K + 1) + pred.long()).reshape(-1), minlength=(K + 1) ** 2)

    src = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(0, 255)
    dst = torch.empty_like(src)

    def copy():
        dst.copy_(src)

    kernel()
    want = by_torch().view(K + 1, K + 1)
    assert torch.equal(counts, want), "the kernel and torch.bincount disagree"
    bg = float(counts[0, 0]) / n
    t_k, t_t, t_c = [], [], []
    for _ in range(3):                        # alternated, so that all three see the same machine state
        t_k.append(events(kernel, 50))
        t_t.append(events(by_torch, 50 if n < 3e7 else 10))
        t_c.append(events(copy, 50))
    t_k, t_t, t_c = min(t_k), min(t_t), min(t_c)
    lines.append("%s  [H,W,D] = %dx%dx%d (%.1f M voxels), %s label with z fastest, K = %d, %.1f %% of the voxels are (0,0)"
                 % (name, h, w, d, n / 1e6, str(dtype).replace("torch.", ""), K, 100 * bg))
    lines.append("  cfun_seg_confusion           %8.1f us   %6.1f MB read      %5.2f TB/s" % (t_k * 1e3, nbytes / 1e6, nbytes / t_k / 1e9))
    lines.append("  1 torch contiguous+bincount  %8.1f us   kernel is %.1fx faster" % (t_t * 1e3, t_t / t_k))
    lines.append("  2 copy_ of %6.1f MB         %8.1f us   %5.2f TB/s read + as much written; kernel time = %.2fx the copy's"
                 % (nbytes / 1e6, t_c * 1e3, nbytes / t_c / 1e9, t_k / t_c))
    if host:
        torch.set_num_threads(16)
        ln, pn = label.cpu().numpy(), pred.permute(1, 2, 0).cpu().numpy()
        t0 = time.perf_counter()
        ref = host_onehot_iou(ln, pn, K)
        t_h = time.perf_counter() - t0
        got = evaluate.SegScores(counts).per_class_iou
        np.testing.assert_allclose(got, ref, rtol=2.0 ** -20 if n >= 2 ** 24 else 2.0 ** -22, atol=0)
        lines.append("  3 one-hot + dot on the host  %8.1f ms   (numpy, 16 threads allowed: a stated baseline, not credit)" % (t_h * 1e3))
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-host", action="store_true", help="skip the host baseline")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_eval needs a GPU: nothing here is measured on the host but the stated baseline"
    lines = ["scoring pass on %s, HIP events, back-to-back calls, best of 3 x 50 (alternated with the yardsticks)" % torch.cuda.get_device_name(0), ""]
    bench_size("heart", 320, 320, 192, torch.int32, lines, not args.no_host)
    bench_size("large", 512, 512, 256, torch.uint8, lines, False)
    txt = "\n".join(lines)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
