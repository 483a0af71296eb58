"""Cases of the voxel-tile geometry (G16 = TD x 4 x 16, G8 = TD x 8 x 8; TD = 2, or 1 at stride 2) of the weight-gradient conv
kernels -- k_wgrad_mfma, k_wgrad_fused and k_wgrad_wino -- shared by test_wgrad_tile_emu.py (HIP emulator) and
test_wgrad_tile_gpu.py (real library).

Every case runs once per geometry through the per-call override (``TILE_G16`` / ``TILE_G8`` OR-ed into the algo):
  * dw against the fp32 CPU reference of kernel_cases.check_conv (torch's conv3d backward on the same seeded operands) at its
    tolerance (kc.RTOL of the reference's max-abs), in the packed and the OIDHW delivery and -- where the conv takes it -- with
    the input prologue (InstanceNorm + LeakyReLU, then LeakyReLU alone), through cfun_conv3d_bwd_weight / _oidhw / _fused
    directly: only the weight gradient depends on this geometry, and the emulator tier stays short.  The folded up-conv runs
    kernel_cases.check_fold_up2_conv3 unchanged (its reference goes through the differentiable fold).
    G8 and G16 sum the voxels in a different order, so nothing is asserted between the geometries;
  * the query entry cfun_conv3d_wgrad_tile must report the forced tile (G16 where no G8 instantiation exists);
  * two calls of cfun_conv3d_bwd_weight on the same operands are bit-equal (no atomics, a fixed reduction order);
  * every call runs under tests/guard.py with a workspace of exactly cfun_conv3d_bwd_weight_workspace_bytes bytes, all
    of it poison, and x and g shadowed between guard bands: a partial slot the plan counts but no workgroup writes, or a read
    outside x or g, is a NaN in dw; a write past a size is a band hit.
The process-wide knobs CFUN_TILE_GEOM and CFUN_WINO_WGRAD_WGS are read once by the library; the module refuses to run with
either set (the rule's table and the "more tiles than chunks" cases would test something else).
The shapes are the smallest at which each path can go wrong: ragged on every axis, exactly one G8 tile with a sample seam, the
product's 6^3, several x tiles, both tap packings (C_in 8 and 4), stride 2 with an even and an odd output, 1x1x1 (the
compact tile), more tiles than workgroups, the fused C_in 20 / 40 kernels, the folded up-conv (live taps only) and, for the
Winograd kernel, every remainder of C_in mod 16 beside a full subtile, one and two output-channel tiles."""
import ctypes as C
import os

import torch
import torch.nn.functional as F

import guard
import kernel_cases as kc
from cfun_amd import _lib, ops
from cfun_amd._lib import ACT_LRELU, ALGO_AUTO, ALGO_MFMA, ALGO_WINO, ALGO_WINO2, TILE_G8, TILE_G16, check

_KNOBS_AT_IMPORT = {k: os.environ[k] for k in ("CFUN_TILE_GEOM", "CFUN_WINO_WGRAD_WGS") if k in os.environ}


def require_default_knobs():
    assert not _KNOBS_AT_IMPORT, "unset %s: the library reads them once per process" % sorted(_KNOBS_AT_IMPORT)


G16, G8 = (4, 16), (8, 8)          # (y, x) of the tile; z is 2, or 1 at stride 2
FLAG = {G16: TILE_G16, G8: TILE_G8}
K3, K1 = (3, 3, 3), (1, 1, 1)

# name: (n, dhw, ci, co, k, kwargs of check_conv)
DIRECT_CASES = {
    "ragged_pack2": (1, (5, 9, 10), 8, 20, K3, {}),
    "one_tile_sample_seam": (2, (4, 8, 8), 32, 16, K3, {}),
    "product_6cube": (2, (6, 6, 6), 16, 32, K3, {}),
    "three_x_tiles": (1, (4, 8, 24), 8, 48, K3, {}),
    "pack4": (1, (5, 9, 10), 4, 16, K3, {}),
    "stride2_even": (1, (8, 12, 12), 4, 40, K3, dict(stride=2)),
    "stride2_odd": (1, (7, 11, 13), 8, 16, K3, dict(stride=2)),
    "pointwise": (2, (6, 6, 6), 16, 8, K1, {}),
    "tiles_81": (3, (6, 24, 24), 16, 16, K3, {}),
}
# C_in = 20 / 40: k_wgrad_fused; check_conv runs their weight gradient with and without the input prologue
FUSED_CASES = {
    "fused_20_8": (1, (5, 9, 10), 20, 8, K3, {}),
    "fused_20_20": (1, (5, 9, 10), 20, 20, K3, {}),
    "fused_40_16": (2, (6, 6, 6), 40, 16, K3, {}),
}
# (ci, co, dhw, n) of check_fold_up2_conv3: the folded up-conv (TSKIP), tiled on the low-resolution grid
FOLD_CASES = {
    "fold_12_40": (12, 40, (3, 6, 6), 2),
    "fold_16_16_6cube": (16, 16, (6, 6, 6), 2),
}
WINO_CASES = {
    "ragged": (1, (5, 9, 10), 16, 48, K3, {}),
    "odd_w_seam": (2, (4, 7, 7), 32, 40, K3, {}),
    "product_6cube": (2, (6, 6, 6), 16, 32, K3, {}),
    "two_cotiles": (2, (4, 8, 8), 32, 96, K3, {}),
    "tiles_81": (3, (6, 24, 24), 16, 16, K3, {}),
    # a remainder ci subtile beside full ones: 8, 8 (tile count 2 * 3 * 3 * 2 / 2 * 3 * 2 * 3 divides no chunk count), 8, 4, 12
    # live rows; no full subtile; two output-channel subtiles
    "rem8_40_40": (2, (5, 9, 10), 40, 40, K3, {}),
    "rem8_40_40_odd_tiles": (2, (6, 12, 20), 40, 40, K3, {}),
    "rem8_24_48": (2, (5, 9, 10), 24, 48, K3, {}),
    "rem4_36_40": (2, (5, 9, 10), 36, 40, K3, {}),
    "rem12_44_40": (2, (5, 9, 10), 44, 40, K3, {}),
    "one_subtile_8_40": (2, (5, 9, 10), 8, 40, K3, {}),
    "rem8_40_20": (2, (5, 9, 10), 40, 20, K3, {}),
    # depth-to-space convs reach this kernel through ALGO_WINO alone: k_wgrad_wino<2, true> and <3, true>
    "d2s_16_64": (2, (5, 9, 10), 16, 64, K3, dict(d2s=True)),
    "d2s_16_96": (1, (4, 7, 7), 16, 96, K3, dict(d2s=True)),
}


def wgrad_tile(spec, x_shape):
    """(z, y, x) of the voxel tile cfun_conv3d_bwd_weight runs the conv with, or None where it is not on the MFMA / Winograd
    weight-gradient kernels."""
    p = ops._params(spec, tuple(x_shape), False, False, False)
    out = (C.c_int32 * 3)()
    rc = int(_lib.load().cfun_conv3d_wgrad_tile(C.byref(p), out))
    return tuple(int(v) for v in out) if rc == 0 else None


def _wgrad_calls(device, spec, x, g, w_shape, stats):
    """Under guard (x and g shadowed through _lib.ptr, every workspace exactly as large as the query says and poisoned):
    the packed gradient twice, the OIDHW gradient, and with ``stats`` = (mean, rstd) table or False the prologue's OIDHW
    gradients (norm + LeakyReLU, LeakyReLU alone)."""
    co, ci, kd, kh, kw = w_shape
    out = {}
    with guard.guarded_memory():
        lib = _lib.load()
        xd, gd = x.to(device), g.to(device)
        p = ops._params(spec, tuple(x.shape), False, False, False)
        bp, st = C.byref(p), _lib.stream(xd)

        def run(fn, shape, *mid):
            dw = torch.empty(shape, dtype=torch.float32, device=device)
            ws = _lib.workspace(lib.cfun_conv3d_bwd_weight_workspace_bytes(bp), xd)
            check(fn(_lib.ptr(xd), _lib.ptr(gd), _lib.ptr(dw), *mid, _lib.ptr(ws), ws.numel(), st), "conv3d_bwd_weight")
            return dw

        packed = (kd * kh * kw, ci, (p.Co + 15) // 16 * 16)
        dws = [run(lib.cfun_conv3d_bwd_weight, packed, bp), run(lib.cfun_conv3d_bwd_weight, packed, bp),
               run(lib.cfun_conv3d_bwd_weight_oidhw, tuple(w_shape), bp)]
        if stats is not None:
            sd = stats.to(device)
            for key, sp in (("norm", sd.data_ptr()), ("lrelu", None)):
                fz = _lib.ConvFusion(sp, ACT_LRELU, 0.01, None, 0.0)
                dws.append(run(lib.cfun_conv3d_bwd_weight_fused, tuple(w_shape), 1, bp, C.byref(fz)))
        guard.verify()
        out["packed"], out["packed2"], out["oidhw"] = (t.cpu() for t in dws[:3])
        if stats is not None:
            out["norm"], out["lrelu"] = dws[3].cpu(), dws[4].cpu()
    return out


def _ref_dw(x, g, w_shape, stride, pad, d2s):
    """torch's conv3d weight gradient (fp32, CPU) -- what kernel_cases.check_conv compares dw with."""
    n = x.shape[0]
    if d2s:      # y = depth_to_space(conv): the conv's output gradient is g gathered per parity, channel (pz, py, px, o)
        d, h, w, cq = g.shape[1] // 2, g.shape[2] // 2, g.shape[3] // 2, g.shape[4]
        gc = g.view(n, d, 2, h, 2, w, 2, cq).permute(0, 2, 4, 6, 7, 1, 3, 5).reshape(n, 8 * cq, d, h, w)
    else:
        gc = g.permute(0, 4, 1, 2, 3)
    wr = torch.zeros(w_shape, requires_grad=True)
    F.conv3d(x.permute(0, 4, 1, 2, 3), wr, None, stride=stride, padding=pad).backward(gc)
    return wr.grad


def check_conv_both(device, n, dhw, ci, co, k, base_algo, kw, want_g8=G8):
    require_default_knobs()
    stride, d2s = kw.get("stride", 1), bool(kw.get("d2s"))
    pad = tuple(kk // 2 for kk in k)
    gen = kc._gen(3)
    x = kc.randn(gen, n, *dhw, ci)
    so = [(d + 2 * q - kk) // stride + 1 for d, q, kk in zip(dhw, pad, k)]
    g = kc.randn(gen, n, *[2 * s for s in so], co // 8) if d2s else kc.randn(gen, n, *so, co)
    ist = torch.stack([kc.randn(gen, n, ci) * 0.5, torch.rand(n, ci, generator=gen) + 0.5], dim=-1)
    w_shape = (co, ci) + tuple(k)
    ref = {"plain": _ref_dw(x, g, w_shape, stride, pad, d2s)}
    xn = (x - ist[..., 0].view(n, 1, 1, 1, ci)) * ist[..., 1].view(n, 1, 1, 1, ci)
    ref["norm"] = _ref_dw(F.leaky_relu(xn, 0.01), g, w_shape, stride, pad, d2s)
    ref["lrelu"] = _ref_dw(F.leaky_relu(x, 0.01), g, w_shape, stride, pad, d2s)
    for geom in (G16, G8):
        algo = base_algo | FLAG[geom]
        spec = ops.ConvSpec(k=k, co=co, stride=stride, pad=pad, algo=algo, d2s=d2s)
        want = geom if geom == G16 else want_g8
        got = wgrad_tile(spec, (n, *dhw, ci))
        assert got == (2 if stride == 1 else 1,) + want, "forced %s, the query reports %s" % (geom, got)
        p = ops._params(spec, tuple(x.shape), False, False, False)
        pro = bool(int(_lib.load().cfun_conv3d_fused_support(C.byref(p))) & _lib.FUSE_IN_NORM_WGRAD)
        if base_algo == ALGO_MFMA:
            assert pro, "the direct weight-gradient kernels take the input prologue"
        what = "%s %s" % (geom, (n, dhw, ci, co))
        got = _wgrad_calls(device, spec, x, g, w_shape, ist if pro else None)
        for key, t in got.items():
            assert bool(torch.isfinite(t).all()), "%s: dw (%s) holds a value nobody wrote or read out of range (poison)" % (what, key)
        assert torch.equal(got["packed"], got["packed2"]), what + ": two runs of the same call differ"
        kc.assert_close(got["oidhw"], ref["plain"], what + " dw (OIDHW)")
        unpacked = got["packed"][:, :, :co].permute(2, 1, 0).reshape(co, ci, *k)
        kc.assert_close(unpacked, ref["plain"], what + " dw (packed)")
        if got["packed"].shape[2] > co:
            assert float(got["packed"][:, :, co:].abs().max()) == 0.0, what + ": the padded columns of the packed dw are not zero"
        for key in ("norm", "lrelu"):
            if key in got:
                kc.assert_close(got[key], ref[key], "%s dw, prologue(%s)" % (what, key))


def _twice_under_guard(device, spec, x, g, dw_shape, what):
    """cfun_conv3d_bwd_weight twice, each with a fresh poisoned workspace of exactly the size the query reports."""
    with guard.guarded_memory():
        lib = _lib.load()
        xd, gd = x.to(device), g.to(device)
        p = ops._params(spec, tuple(x.shape), False, False, False)
        dws = []
        for _ in range(2):
            dw = torch.empty(dw_shape, dtype=torch.float32, device=device)
            ws = _lib.workspace(lib.cfun_conv3d_bwd_weight_workspace_bytes(C.byref(p)), xd)
            check(lib.cfun_conv3d_bwd_weight(_lib.ptr(xd), _lib.ptr(gd), _lib.ptr(dw), C.byref(p), _lib.ptr(ws), ws.numel(),
                                             _lib.stream(xd)), "conv3d_bwd_weight")
            dws.append(dw)
        guard.verify()
        a, b = dws[0].cpu(), dws[1].cpu()
    assert bool(torch.isfinite(a).all()), what + ": dw holds a value nobody wrote (poison)"
    assert torch.equal(a, b), what + ": two runs of the same call differ"
    return a


def check_fold_both(device, ci, co, dhw, n):
    require_default_knobs()
    gen = kc._gen(4)
    cqp = (co + 15) // 16 * 16
    x = kc.randn(gen, n, *dhw, ci)
    g = kc.randn(gen, n, 2 * dhw[0], 2 * dhw[1], 2 * dhw[2], co)
    for geom in (G16, G8):
        algo = ALGO_MFMA | FLAG[geom]
        spec = ops.ConvSpec(k=K3, co=8 * cqp, pad=(1, 1, 1), d2s=True, d2s_cq=co, tap_skip=True, algo=algo)
        got = wgrad_tile(spec, (n, *dhw, ci))
        assert got == (2,) + geom, "forced %s, the query reports %s" % (geom, got)
        kc.check_fold_up2_conv3(device, ci, co, dhw, algo, n=n)
        _twice_under_guard(device, spec, x, g, (27, ci, 8 * cqp), "fold %s %s" % (geom, (n, dhw, ci, co)))


def check_no_g8_instantiation():
    """Forced G8 where no 8 x 8 weight-gradient instantiation exists: the query reports G16 (and the launch runs G16)."""
    assert wgrad_tile(ops.ConvSpec(k=K3, co=32, pad=(1, 1, 1), algo=ALGO_WINO2 | TILE_G8), (1, 6, 6, 6, 16)) == (2, 4, 16)
    assert wgrad_tile(ops.ConvSpec(k=(1, 3, 3), co=16, pad=(0, 1, 1), algo=ALGO_MFMA | TILE_G8), (1, 6, 6, 6, 16)) == (2, 4, 16)
    assert wgrad_tile(ops.ConvSpec(k=K1, co=64, stride=2, pad=(0, 0, 0), algo=ALGO_MFMA | TILE_G8), (1, 12, 12, 12, 16)) == (1, 4, 16)
    # C_in = 1 runs the stem weight-gradient kernel: no tile to report
    assert wgrad_tile(ops.ConvSpec(k=K3, co=20, pad=(1, 1, 1), algo=ALGO_AUTO), (1, 6, 6, 6, 1)) is None


# AUTO: the forward's rule on the grid the weight gradient tiles -- G8 exactly where it strictly raises the filled fraction
AUTO_TABLE = [((6, 6, 6), G8), ((12, 12, 12), G16), ((16, 16, 16), G16), ((24, 24, 24), G8), ((32, 32, 32), G16),
              ((48, 48, 48), G16), ((96, 96, 96), G16), ((16, 32, 32), G16)]


def check_auto_table():
    """The rule's choice through the query entry, for the Winograd weight gradient (AUTO: C_in = 16, C_out = 32), the direct
    kernels (ALGO_MFMA) and the stride-2 weight gradient on ITS output grid."""
    require_default_knobs()
    for dhw, want in AUTO_TABLE:      # (4 samples, as the step's 4 RoIs)
        for algo in (ALGO_AUTO, ALGO_MFMA):
            got = wgrad_tile(ops.ConvSpec(k=K3, co=32, pad=(1, 1, 1), algo=algo), (4, *dhw, 16))
            assert got == (2,) + want, "%s algo %d: %s, the rule says %s" % (dhw, algo, got, want)
        got = wgrad_tile(ops.ConvSpec(k=K3, co=32, stride=2, pad=(1, 1, 1), algo=ALGO_MFMA), (4, *[2 * d for d in dhw], 16))
        assert got == (1,) + want, "stride 2 -> %s: %s, the rule says %s" % (dhw, got, want)
    # the folded up-conv tiles its low-resolution grid
    l23 = dict(k=K3, co=8 * 48, pad=(1, 1, 1), d2s=True, d2s_cq=40, tap_skip=True)
    assert wgrad_tile(ops.ConvSpec(algo=ALGO_AUTO, **l23), (4, 24, 24, 24, 80)) == (2,) + G8
    # the recorded exception: the folded up-conv with 80-column tiles (l0.3, 320 -> 160 per parity @ 6^3) -- its input-prologue
    # instantiation keeps one wave instead of two on G8 (conv3d.hip: wgrad_g8_loses_wave) -- stays G16 unless forced
    l03 = dict(k=K3, co=8 * 160, pad=(1, 1, 1), d2s=True, d2s_cq=160, tap_skip=True)
    assert wgrad_tile(ops.ConvSpec(algo=ALGO_AUTO, **l03), (4, 6, 6, 6, 320)) == (2,) + G16
    assert wgrad_tile(ops.ConvSpec(algo=ALGO_AUTO | TILE_G8, **l03), (4, 6, 6, 6, 320)) == (2,) + G8
    # 1x1x1 follows the rule too (the step's 160 -> 80 @ 24^3); the 2-D Winograd kernel never does
    assert wgrad_tile(ops.ConvSpec(k=K1, co=80, pad=(0, 0, 0), algo=ALGO_AUTO), (4, 24, 24, 24, 160)) == (2,) + G8
    assert wgrad_tile(ops.ConvSpec(k=K3, co=32, pad=(1, 1, 1), algo=ALGO_WINO2), (4, 24, 24, 24, 16)) == (2,) + G16
