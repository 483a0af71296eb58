"""Cases of the output-tile geometry (G16 = 4 x 4 x 16, G8 = 4 x 8 x 8) of the forward / data-gradient conv kernels, shared by
test_tile_geometry_emu.py (HIP emulator) and test_tile_geometry_gpu.py (real library).

Every case runs once per geometry through the per-call override (``TILE_G16`` / ``TILE_G8`` OR-ed into the algo):
  * kernel_cases.check_conv / check_fold_up2_conv3, unchanged, at their own tolerance (2e-5 of the reference's max-abs);
  * the query entry cfun_conv3d_fwd_tile must report the forced tile;
  * the tile shape does not change any output voxel's accumulation order, so wherever neither geometry splits K
    (splitk_factor: fewer than 8 channel chunks, i.e. C_in <= 28) y and dx of the two runs must be bit-equal.
The shapes are the smallest at which G8 can go wrong: ragged on every axis, exactly one tile with a sample seam, the product's
6^3, several x tiles, the split-K path, stride 2 (whose dx is the folded 2x2x2 data gradient), depth-to-space, remainder
quads (C_out = 20), odd widths and a half-filled register pair of the two-waves-per-SIMD Winograd loop."""
import ctypes as C

import torch

import kernel_cases as kc
from cfun_amd import _lib, ops
from cfun_amd._lib import check, ptr
from cfun_amd._lib import ACT_LRELU, ALGO_AUTO, ALGO_MFMA, ALGO_WINO, ALGO_WINO2, TILE_G8, TILE_G16

G16, G8 = (4, 4, 16), (4, 8, 8)
FLAG = {G16: TILE_G16, G8: TILE_G8}
K3 = (3, 3, 3)
FULL = dict(act=ACT_LRELU, scale=True, per_n=True, shift=True, res=True)

# name: (n, dhw, ci, co, kwargs of check_conv)
DIRECT_CASES = {
    "ragged_rem_quad": (1, (5, 9, 10), 8, 20, {}),
    "one_tile_sample_seam": (2, (4, 8, 8), 8, 16, {}),
    "product_6cube": (2, (6, 6, 6), 16, 32, {}),
    "three_x_tiles": (1, (4, 8, 24), 8, 48, {}),
    "splitk_epilogue": (2, (4, 8, 8), 32, 16, FULL),
    "stride2_folded_dgrad": (1, (8, 12, 12), 4, 40, dict(stride=2)),
    "d2s_res": (2, (3, 6, 6), 8, 64, dict(d2s=True, res=True)),
}
# (ci, co, dhw, n) of check_fold_up2_conv3: the folded up-conv (MODE 2) and its data gradient (MODE 3)
FOLD_CASES = {
    "fold_12_40": (12, 40, (3, 6, 6), 2),
    "fold_16_16_6cube": (16, 16, (6, 6, 6), 2),
}
WINO_CASES = {
    "ragged": (1, (5, 9, 10), 8, 48, {}),
    "epilogue_odd_w": (2, (4, 7, 7), 8, 40, FULL),
    "two_cotiles_splitk": (2, (4, 8, 8), 32, 96, {}),
    "product_6cube": (2, (6, 6, 6), 16, 32, {}),
    "odd_chunks": (2, (5, 8, 9), 12, 24, {}),
}
WINO_ALGOS = {"wino": ALGO_WINO, "wino2": ALGO_WINO2}


def fwd_tile(spec, x_shape, has_scale=False, has_shift=False, has_res=False):
    """(z, y, x) of the output tile cfun_conv3d_fwd runs the conv with, or None where it is not on the MFMA / Winograd kernels."""
    p = ops._params(spec, tuple(x_shape), has_scale, has_shift, has_res)
    out = (C.c_int32 * 3)()
    rc = int(_lib.load().cfun_conv3d_fwd_tile(C.byref(p), out))
    return tuple(int(v) for v in out) if rc == 0 else None


def _spec(co, algo, stride=1, act=0, per_n=False, d2s=False, **_):
    return ops.ConvSpec(k=K3, co=co, stride=stride, pad=(1, 1, 1), act=act, scale_per_n=per_n, algo=algo, d2s=d2s)


def _run(device, n, dhw, ci, co, algo, kw, seed=0):
    """y and dx of one conv call (check_conv's inputs, no reference): the operands of the bit-equality check."""
    gen = kc._gen(seed)
    spec = _spec(co, algo, **kw)
    x = kc.randn(gen, n, *dhw, ci)
    w = kc.randn(gen, co, ci, *K3) / float(ci * 27) ** 0.5
    sc = (torch.rand(n, co, generator=gen) + 0.5) if kw.get("scale") else None
    sf = kc.randn(gen, co) if kw.get("shift") else None
    so = [(d + 2 - 3) // spec.stride + 1 for d in dhw]
    cy = co // 8 if spec.d2s else co
    rs = kc.randn(gen, n, *so, cy) if kw.get("res") else None
    gy = kc.randn(gen, n, *[s * (2 if spec.d2s else 1) for s in so], cy)
    xd = x.to(device).requires_grad_(True)
    y = ops.conv3d(xd, ops.pack_weight(w.to(device)), spec, None if sc is None else sc.to(device),
                   None if sf is None else sf.to(device), None if rs is None else rs.to(device))
    y.backward(gy.to(device))
    return y.detach(), xd.grad


def check_conv_both(device, n, dhw, ci, co, base_algo, kw):
    runs = {}
    for geom in (G16, G8):
        algo = base_algo | FLAG[geom]
        got = fwd_tile(_spec(co, algo, **kw), (n, *dhw, ci), bool(kw.get("scale")), bool(kw.get("shift")), bool(kw.get("res")))
        assert got == geom, "forced %s, the query reports %s" % (geom, got)
        kc.check_conv(device, n, dhw, ci, co, K3, algo=algo, **kw)
        runs[geom] = _run(device, n, dhw, ci, co, algo, kw)
    if ci <= 28:      # fewer than 8 channel chunks: splitk_factor never splits, the accumulation order is the tile-free one
        assert torch.equal(runs[G8][0], runs[G16][0]), "y differs between the geometries"
        assert torch.equal(runs[G8][1], runs[G16][1]), "dx differs between the geometries"


def _run_fold(device, ci, co, dhw, n, algo, seed=8):
    gen = kc._gen(seed)
    x = kc.randn(gen, n, *dhw, ci)
    w = kc.randn(gen, co, ci, 3, 3, 3) / float(27 * ci) ** 0.5
    gy = kc.randn(gen, n, 2 * dhw[0], 2 * dhw[1], 2 * dhw[2], co)
    cqp = (co + 15) // 16 * 16
    spec = ops.ConvSpec(k=K3, co=8 * cqp, pad=(1, 1, 1), d2s=True, d2s_cq=co, tap_skip=True, algo=algo)
    xd = x.to(device).requires_grad_(True)
    y = ops.conv3d(xd, ops.pack_weight(ops.fold_up2_weight(w.to(device), cqp)), spec)
    y.backward(gy.to(device))
    # the data gradient (MODE 3) once more through the C entry WITHOUT a workspace: it cannot split K, so its accumulation
    # order is the tile-free one whatever the channel count
    p = ops._params(spec, tuple(x.shape), False, False, False)
    wp = ops.pack_weight(ops.fold_up2_weight(w.to(device), cqp)).detach()
    g, dx, wpT = gy.to(device).contiguous(), torch.empty_like(xd.detach()), ops._transpose_pack(wp, p.Co)
    check(_lib.load().cfun_conv3d_bwd_data(ptr(g), ptr(wpT), ptr(dx), C.byref(p), None, 0, _lib.stream(g)),
          "conv3d_bwd_data without workspace")
    return spec, y.detach(), xd.grad, dx


def check_fold_both(device, ci, co, dhw, n):
    runs = {}
    for geom in (G16, G8):
        algo = ALGO_MFMA | FLAG[geom]
        kc.check_fold_up2_conv3(device, ci, co, dhw, algo, n=n)
        spec, y, dx, dx_nows = _run_fold(device, ci, co, dhw, n, algo)
        got = fwd_tile(spec, (n, *dhw, ci))
        assert got == geom, "forced %s, the query reports %s" % (geom, got)
        kc.assert_close(dx_nows, dx, "dx without workspace vs dx of the autograd path")
        runs[geom] = (y, dx_nows)
    # d2s launches never split K; the autograd path's data gradient (8 * co / 4 >= 8 chunks) may, the workspace-free one cannot
    assert torch.equal(runs[G8][0], runs[G16][0]), "y differs between the geometries"
    assert torch.equal(runs[G8][1], runs[G16][1]), "dx (no split-K) differs between the geometries"


# AUTO: G8 exactly where it strictly raises the filled fraction of the tiled grid -- 6 (8*16 -> 8*8) and 24 (24*32 -> 24*24);
# 12 would get worse (12*16 -> 16*16), the others are equal and stay G16
AUTO_TABLE = [((6, 6, 6), G8), ((12, 12, 12), G16), ((16, 16, 16), G16), ((24, 24, 24), G8), ((32, 32, 32), G16),
              ((48, 48, 48), G16), ((96, 96, 96), G16), ((16, 32, 32), G16)]


def check_auto_table():
    """The rule's choice through the query entry, for the Winograd family (AUTO: C_in = 16, C_out = 32) and the direct MFMA
    family (ALGO_MFMA), plus the stride-2 forward on ITS output grid."""
    for dhw, want in AUTO_TABLE:      # (4 samples, as the step's 4 RoIs)
        for algo in (ALGO_AUTO, ALGO_MFMA):
            got = fwd_tile(ops.ConvSpec(k=K3, co=32, pad=(1, 1, 1), algo=algo), (4, *dhw, 16))
            assert got == want, "%s algo %d: %s, the rule says %s" % (dhw, algo, got, want)
        got = fwd_tile(ops.ConvSpec(k=K3, co=32, stride=2, pad=(1, 1, 1), algo=ALGO_MFMA), (4, *[2 * d for d in dhw], 16))
        assert got == want, "stride 2 -> %s: %s, the rule says %s" % (dhw, got, want)
    # LiTS' 20-wide level falls out of the same rule (20 * 32 -> 24 * 24)
    assert fwd_tile(ops.ConvSpec(k=K3, co=32, pad=(1, 1, 1), algo=ALGO_AUTO), (4, 8, 20, 20, 16)) == G8
    # the step's own launches at these levels: a per-RoI Dropout3d conv (one sample, 80 -> k kept channels) and the folded
    # up-conv l2.3 (80 -> 40 per parity, padded to 48) at 24^3 run G8; the recorded exception -- the folded up-conv's forward
    # at 6^3 measured no faster (conv3d.hip: g8_no_gain) -- stays G16 unless forced
    for k in (32, 44):
        assert fwd_tile(ops.ConvSpec(k=K3, co=k, pad=(1, 1, 1), algo=ALGO_AUTO), (1, 24, 24, 24, 80)) == G8
    l23 = dict(k=K3, co=8 * 48, pad=(1, 1, 1), d2s=True, d2s_cq=40, tap_skip=True)
    assert fwd_tile(ops.ConvSpec(algo=ALGO_AUTO, **l23), (4, 24, 24, 24, 80)) == G8
    l03 = dict(k=K3, co=8 * 160, pad=(1, 1, 1), d2s=True, d2s_cq=160, tap_skip=True)
    assert fwd_tile(ops.ConvSpec(algo=ALGO_AUTO, **l03), (4, 6, 6, 6, 320)) == G16
    assert fwd_tile(ops.ConvSpec(algo=ALGO_AUTO | TILE_G8, **l03), (4, 6, 6, 6, 320)) == G8
    # no G8 instantiation: 1x1x1 stays G16 even when forced
    assert fwd_tile(ops.ConvSpec(k=(1, 1, 1), co=32, pad=(0, 0, 0), algo=ALGO_MFMA | TILE_G8), (1, 6, 6, 6, 16)) == G16

