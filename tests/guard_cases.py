"""Cases of the guard tier shared by test_guard_emu.py and test_guard_gpu.py: the zero-size contract of the wrappers, small
cases for C entries no other kernel case reaches (plain torch references, in the style of kernel_cases.py; the plain conv
entries against the fused ones the wrappers call), and the
accounting of the entries that ran under guard against ``_lib.EXPORTS``."""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

import guard
from cfun_amd import _lib, ops
from cfun_amd._lib import ACT_LRELU, ALGO_DIRECT, ALGO_MFMA
from kernel_cases import _gen, assert_close, py_bounds, randn, ref_conv
from oracle import cfun_oracle as orc

# Entries that need no run under guard, one reason each.  Everything else in _lib.EXPORTS launches work and must have been
# called under guarded_memory() by the tier's own file.
_HOST = "host-side query: launches nothing, touches no device memory"
EXEMPT = {name: _HOST for name in guard.NO_LAUNCH}
EXEMPT_EMU = dict(EXEMPT)
EXEMPT_GPU = dict(EXEMPT)


def check_coverage(exempt, tier):
    exports, seen = set(_lib.EXPORTS), guard.SEEN[tier]
    assert set(exempt) <= exports, "exempt entries that the library does not export: %s" % sorted(set(exempt) - exports)
    missed = sorted(exports - set(exempt) - seen)
    print("guard tier (%s): %d allocations guarded, %d input shadows, %d verify() calls, %d payload bytes; %d of %d entries seen, "
          "%d exempt" % (tier, guard.COUNTS["allocations"], guard.COUNTS["shadows"], guard.COUNTS["verifies"], guard.COUNTS["bytes"],
                         len(seen & exports), len(exports), len(exempt)))
    assert not missed, "entries that launch work but never ran under guard (add a case, not an exemption): %s" % missed


def check_all(device):
    check_instnorm_bwd_entries(device)
    check_roi_align_whole_map_entries(device)
    check_mask_losses_bwd_entry(device)
    check_concat_lrelu(device)
    check_plain_conv_entries(device)


def check_concat_lrelu(device, seed=64):
    """Two LeakyReLUs written into the channel ranges of a ConcatBuffer and joined without a copy against torch.cat: the
    backward hands each its channel range of the gradient as a strided view (cfun_lrelu_fwd_strided / _bwd_strided)."""
    gen = _gen(seed)
    for shape, ca, cb in (((2, 3, 4, 5), 8, 12), ((1, 2, 2, 3), 4, 4)):
        a, b, g = randn(gen, *shape, ca), randn(gen, *shape, cb), randn(gen, *shape, ca + cb)
        ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        yr = torch.cat([F.leaky_relu(ar, 0.01), F.leaky_relu(br, 0.01)], dim=-1)
        yr.backward(g)
        ad, bd = a.clone().to(device).requires_grad_(True), b.clone().to(device).requires_grad_(True)
        buf = ops.ConcatBuffer(ad, ca + cb)
        y = buf.join(ops.lrelu(ad, out=buf.slot(0, ca)), ops.lrelu(bd, out=buf.slot(ca, ca + cb)))
        y.backward(g.to(device))
        assert_close(y, yr, "concat lrelu y")
        assert_close(ad.grad, ar.grad, "concat lrelu da")
        assert_close(bd.grad, br.grad, "concat lrelu db")


def check_instnorm_bwd_entries(device, seed=61):
    """The InstanceNorm + LeakyReLU backward entries the wrappers do not call on one rank -- cfun_instnorm_lrelu_bwd, its
    _strided form (the gradient is a channel range of a wider buffer) and the depth-sharded pair cfun_instnorm_bwd_means /
    cfun_instnorm_lrelu_bwd_apply with the single rank's means -- through the C ABI against torch autograd in fp64 (the
    dx bound of kernel_cases.check_instnorm_lrelu).  The channel range sits at either end of the wide rows, so a read past a
    row's range at the buffer's start or end leaves the buffer."""
    lib = _lib.load()
    gen = _gen(seed)
    for n, v, c, ct in ((2, 60, 8, 20), (1, 18, 4, 12), (3, 343, 20, 40)):
        x = randn(gen, n, v, c) * 1.5 + randn(gen, 1, 1, c)
        gy = randn(gen, n, v, c)
        x64 = x.double().requires_grad_(True)
        mean, var = x64.mean(1, keepdim=True), x64.var(1, unbiased=False, keepdim=True)
        F.leaky_relu((x64 - mean) / torch.sqrt(var + 1e-5), 0.01).backward(gy.double())
        ref = x64.grad.float()
        stats = torch.stack([mean.detach()[:, 0], torch.rsqrt(var.detach() + 1e-5)[:, 0]], dim=-1).float().contiguous().to(device)
        xd, dy = x.to(device), gy.to(device)
        nb = lib.cfun_instnorm_workspace_bytes(n, v, c)
        dx = torch.empty_like(xd)
        ws = _lib.workspace(nb, xd)
        _lib.check(lib.cfun_instnorm_lrelu_bwd(ops.ptr(xd), ops.ptr(stats), ops.ptr(dy), ops.ptr(dx), n, v, c, 0.01, ops.ptr(ws),
                                               ws.numel(), ops.stream(xd)), "instnorm_lrelu_bwd")
        assert_close(dx, ref, "instnorm_lrelu_bwd dx (c=%d)" % c, 1e-4)
        for c0 in (0, ct - c):
            wide = torch.empty((n, v, ct), dtype=torch.float32, device=device)
            wide.copy_(randn(gen, n, v, ct))
            wide[..., c0:c0 + c] = dy
            dyv = wide[..., c0:c0 + c]
            dx = torch.empty_like(xd)
            ws = _lib.workspace(nb, xd)
            _lib.check(lib.cfun_instnorm_lrelu_bwd_strided(ops.ptr(xd), ops.ptr(stats), ops.ptr_raw(dyv), ops.ptr(dx), n, v, c, ct,
                                                           0.01, ops.ptr(ws), ws.numel(), ops.stream(xd)), "instnorm_lrelu_bwd_strided")
            assert_close(dx, ref, "instnorm_lrelu_bwd_strided dx (c=%d, c0=%d)" % (c, c0), 1e-4)
            means = torch.empty((n, c, 2), dtype=torch.float32, device=device)
            dx = torch.empty_like(xd)
            ws = _lib.workspace(nb, xd)
            _lib.check(lib.cfun_instnorm_bwd_means(ops.ptr(xd), ops.ptr(stats), ops.ptr_raw(dyv), ops.ptr(means), n, v, c, ct, 0.01,
                                                   ops.ptr(ws), ws.numel(), ops.stream(xd)), "instnorm_bwd_means")
            _lib.check(lib.cfun_instnorm_lrelu_bwd_apply(ops.ptr(xd), ops.ptr(stats), ops.ptr(means), ops.ptr_raw(dyv), ops.ptr(dx),
                                                         n, v, c, ct, 0.01, ops.stream(xd)), "instnorm_lrelu_bwd_apply")
            assert_close(dx, ref, "instnorm_bwd_means + _bwd_apply dx (c=%d, c0=%d)" % (c, c0), 1e-4)


def check_roi_align_whole_map_entries(device, seed=62):
    """cfun_roi_align3d_fwd / _bwd (the whole-map entries; the wrappers call the depth-slab forms) through the C ABI against the
    oracle, at kernel_cases.check_roi_align's bounds: integer crop bit-exact, values to 2e-6, gradient to 1e-5 of its scale."""
    lib = _lib.load()
    gen = _gen(seed)
    c, d, h, w = 4, 5, 6, 7
    pd, ph, pw = 3, 2, 4
    fm = randn(gen, c, d, h, w)
    boxes = torch.tensor([[0.0, 0.0, 0.0, 1.0, 1.0, 1.0], [0.1, 0.2, 0.3, 0.6, 0.9, 0.8], [0.4, 0.0, 0.5, 0.45, 0.3, 0.55],
                          [-0.2, -0.1, 0.0, 0.5, 1.2, 0.7], [0.5, 0.5, 0.5, 0.5, 0.5, 0.5], [0.9, 0.9, 0.9, 1.0, 1.0, 1.0]])
    r = boxes.shape[0]
    gy = randn(gen, r, c, pd, ph, pw)
    fr = fm.clone().requires_grad_(True)
    ref = orc.roi_align(fr, [pd, ph, pw], boxes)
    (ref * gy).sum().backward()
    fd, bx = fm.permute(1, 2, 3, 0).contiguous().to(device), boxes.to(device)
    out = torch.empty((r, pd, ph, pw, c), dtype=torch.float32, device=device)
    bounds = torch.empty((r, 6), dtype=torch.int32, device=device)
    _lib.check(lib.cfun_roi_align3d_fwd(ops.ptr(fd), ops.ptr(bx), ops.ptr(out), ops.ptr(bounds), r, d, h, w, c, pd, ph, pw,
                                        ops.stream(fd)), "roi_align3d_fwd")
    np.testing.assert_array_equal(bounds.cpu().numpy(), py_bounds(boxes, (d, h, w)))
    assert float((out.permute(0, 4, 1, 2, 3).cpu() - ref.detach()).abs().max()) < 2e-6
    dout = gy.permute(0, 2, 3, 4, 1).contiguous().to(device)
    dfm = torch.empty((d, h, w, c), dtype=torch.float32, device=device)
    _lib.check(lib.cfun_roi_align3d_bwd(ops.ptr(dout), ops.ptr(bounds), ops.ptr(dfm), r, d, h, w, c, pd, ph, pw, ops.stream(fd)),
               "roi_align3d_bwd")
    assert float((dfm.permute(3, 0, 1, 2).cpu() - fr.grad).abs().max()) < 1e-5 * max(1.0, float(fr.grad.abs().max()))


def check_mask_losses_bwd_entry(device, seed=63):
    """cfun_mask_losses_bwd (both mask losses' backward in one pass WITHOUT the forward's saved coefficient field; the
    wrappers take it only for volumes thinner than 3) through the C ABI against the oracle's autograd, at the bound
    kernel_cases.check_mask_losses holds the fused backward to (1e-3 of max-abs)."""
    lib = _lib.load()
    rng = np.random.default_rng(seed)
    for n, c, dhw in ((1, 8, (5, 6, 7)), (2, 3, (21, 4, 9))):
        lg = torch.from_numpy(rng.normal(size=(n, c) + dhw).astype(np.float32))
        labels = rng.integers(0, c, size=(n,) + dhw).astype(np.uint8)
        lab = torch.from_numpy(labels.astype(np.int64))
        onehot = torch.stack([(lab == k) for k in range(c)], dim=1).double()
        lr = lg.clone().requires_grad_(True)
        (0.7 * orc.mask_ce_loss(onehot, lr) + 1.3 * orc.edge_loss(onehot, torch.softmax(lr, dim=1))[0]).backward()
        ld = lg.permute(0, 2, 3, 4, 1).contiguous().to(device)
        labd = torch.from_numpy(labels).to(device)
        probs = ops.softmax_channels(ld)
        g = torch.tensor([0.7, 1.3], dtype=torch.float32).to(device)
        dl = torch.empty_like(ld)
        d, h, w = dhw
        ws = _lib.workspace(lib.cfun_edge_loss_bwd_workspace_bytes(n, d, h, w, c), ld)
        _lib.check(lib.cfun_mask_losses_bwd(ops.ptr(probs), ops.ptr(labd), ops.ptr(g), ops.ptr(g[1:]), ops.ptr(dl), n, d, h, w, c,
                                            ops.ptr(ws), ws.numel(), ops.stream(ld)), "mask_losses_bwd")
        assert_close(dl.permute(0, 4, 1, 2, 3), lr.grad, "cfun_mask_losses_bwd vs oracle (C=%d)" % c, 1e-3)


def check_plain_conv_entries(device, seed=65):
    """cfun_conv3d_fwd, cfun_conv3d_bwd_weight and cfun_conv3d_bwd_weight_oidhw (the plain entries of the C ABI; the wrappers
    call cfun_conv3d_fwd_fused / cfun_conv3d_bwd_weight_fused for every conv, with a null fusion for a plain one) through the
    C ABI: equal BIT FOR BIT to the fused entry with a null fusion on the same inputs, on an MFMA shape and a direct one; y and
    the OIDHW gradient also against torch at kernel_cases.check_conv's bound."""
    lib = _lib.load()
    gen = _gen(seed)
    for n, dhw, ci, co, algo in ((2, (4, 5, 7), 16, 16, ALGO_MFMA), (1, (4, 5, 6), 3, 8, ALGO_DIRECT)):
        spec = ops.ConvSpec(k=(3, 3, 3), co=co, pad=(1, 1, 1), act=ACT_LRELU, algo=algo)
        x, w = randn(gen, n, *dhw, ci), randn(gen, co, ci, 3, 3, 3) / float(27 * ci) ** 0.5
        shift, g = randn(gen, co), randn(gen, n, *dhw, co)          # g: the gradient w.r.t. the conv sum
        wr = w.clone().requires_grad_(True)
        F.conv3d(x.permute(0, 4, 1, 2, 3), wr, padding=1).backward(g.permute(0, 4, 1, 2, 3))
        xd, sd, gd = x.to(device), shift.to(device), g.to(device)
        wp = ops.pack_weight(w.to(device))
        p = ops._params(spec, xd.shape, False, True, False)
        bp, st = C.byref(p), ops.stream(xd)
        y = [torch.empty((n,) + dhw + (co,), dtype=torch.float32, device=device) for _ in range(2)]
        ws = _lib.workspace(lib.cfun_conv3d_fwd_workspace_bytes(bp), xd)
        _lib.check(lib.cfun_conv3d_fwd(ops.ptr(xd), ops.ptr(wp), None, ops.ptr(sd), None, ops.ptr(y[0]), bp, ops.ptr(ws),
                                       ws.numel(), st), "conv3d_fwd")
        ws = _lib.workspace(lib.cfun_conv3d_fwd_fused_workspace_bytes(bp, None), xd)
        _lib.check(lib.cfun_conv3d_fwd_fused(ops.ptr(xd), ops.ptr(wp), None, ops.ptr(sd), None, ops.ptr(y[1]), bp, None,
                                             ops.ptr(ws), ws.numel(), st), "conv3d_fwd_fused(null)")
        assert torch.equal(y[0], y[1]), "cfun_conv3d_fwd differs from cfun_conv3d_fwd_fused with a null fusion (algo %d)" % algo
        assert_close(y[0], ref_conv(x, w, spec, None, shift, None), "cfun_conv3d_fwd y (algo %d)" % algo)
        for oidhw, plain in ((0, lib.cfun_conv3d_bwd_weight), (1, lib.cfun_conv3d_bwd_weight_oidhw)):
            dw = [torch.empty(tuple(w.shape) if oidhw else tuple(wp.shape), dtype=torch.float32, device=device) for _ in range(2)]
            ws = _lib.workspace(lib.cfun_conv3d_bwd_weight_workspace_bytes(bp), xd)
            _lib.check(plain(ops.ptr(xd), ops.ptr(gd), ops.ptr(dw[0]), bp, ops.ptr(ws), ws.numel(), st), "conv3d_bwd_weight")
            ws = _lib.workspace(lib.cfun_conv3d_bwd_weight_workspace_bytes(bp), xd)
            _lib.check(lib.cfun_conv3d_bwd_weight_fused(ops.ptr(xd), ops.ptr(gd), ops.ptr(dw[1]), oidhw, bp, None, ops.ptr(ws),
                                                        ws.numel(), st), "conv3d_bwd_weight_fused(null)")
            assert torch.equal(dw[0], dw[1]), ("the plain weight-gradient entry differs from cfun_conv3d_bwd_weight_fused with a "
                                               "null fusion (oidhw %d, algo %d)" % (oidhw, algo))
            if oidhw:
                assert_close(dw[0], wr.grad, "cfun_conv3d_bwd_weight_oidhw dw (algo %d)" % algo)


def check_zero_size(device):
    """Every wrapper with an empty leading dimension: a correctly shaped result (empty, or zeros where the math says
    zero), no error, and -- under guard -- no byte written anywhere."""
    gen = _gen(51)
    fm = randn(gen, 4, 5, 6, 8).to(device).requires_grad_(True)
    out, bounds = ops.roi_align(fm, torch.zeros(0, 6, device=device), (2, 3, 4))
    assert tuple(out.shape) == (0, 2, 3, 4, 8) and bounds.dtype == torch.int32
    out.sum().backward()
    assert tuple(fm.grad.shape) == (4, 5, 6, 8) and float(fm.grad.abs().max()) == 0.0      # no RoI: a zero gradient
    keep, count = ops.nms3d(torch.zeros(0, 6, device=device), torch.zeros(0, device=device), 0.5, 10)
    assert int(count.item()) == 0 and keep.dtype == torch.int32
    x = torch.zeros(0, 16, device=device, requires_grad=True)
    w = randn(gen, 12, 16).to(device).requires_grad_(True)
    y = ops.fc(x, w, None, torch.ones(12, device=device))
    assert tuple(y.shape) == (0, 12)
    y.sum().backward()
    assert float(w.grad.abs().max()) == 0.0
    lab = torch.randint(0, 5, (6, 7, 8), generator=gen, dtype=torch.int64).to(torch.uint8).to(device)
    t = ops.mask_target_labels(lab, torch.zeros(0, 6, device=device), (4, 4, 4))
    assert tuple(t.shape) == (0, 4, 4, 4) and t.dtype == torch.uint8
    labels, full = ops.unmold_overlap(torch.zeros(0, 4, 4, 4, 3, device=device), [], (5, 6, 7), want_full=True)
    assert tuple(labels.shape) == (5, 6, 7) and tuple(full.shape) == (5, 6, 7, 3)
    assert int(labels.max()) == 0 and float(full.abs().max()) == 0.0           # no detection: background everywhere
    s = ops.channel_sum(torch.zeros(0, 16, device=device))
    assert tuple(s.shape) == (16,) and float(s.abs().max()) == 0.0             # an empty sum
