"""Both sides of every predicate that chooses a conv kernel family (cfun_amd/csrc/conv3d.hip and the *_supported functions it
asks), shared by test_dispatch_emu.py (HIP emulator) and test_dispatch_gpu.py (real library).

The predicates: cfun_conv_pointwise_supported / _in_supported, cfun_conv_stem_supported, mfma_shape, cfun_wino_supported,
use_folded_s2_dgrad, use_mfma_dgrad / make_dgrad_params, cfun_wino_s2d_dgrad_supported, cfun_wgrad_c1_supported,
cfun_wino_wgrad_supported, and the workspace-dependent fallbacks of conv_fwd_impl and cfun_conv3d_bwd_data.  A predicate
that admits a conv its kernel does not implement gives wrong numbers with return code 0, so every case here

  * asserts which side of its boundary it is on through the queries -- cfun_conv3d_fwd_kernel, cfun_weight_prepare_kinds,
    cfun_conv3d_bwd_kernels, cfun_conv3d_wgrad_tile (which refuses exactly the C_in = 1 and direct weight gradients) -- so the
    table cannot go stale when a threshold moves;
  * replays the conv through product_shapes.replay: y and dx on boxes, dw / dshift / dres in full against fp64 under the
    project's rule (product_shapes.bound), prologue runs bit for bit against the materialised input;
  * runs once more inside ops.WeightScope when its operands are not the plain packs: bit-equal results.

The shapes are the smallest at which each predicate can go wrong.  CASES maps a name to (Sig, (forward, data gradient,
weight gradient, data-gradient operand kind or None)).  The C-entry checks below it cover what ``ops`` never does: misaligned
pointers, short or missing workspaces, CFUN_ALGO_MFMA without an MFMA kernel, and empty problems."""
import ctypes as C

import torch

import guard
import product_shapes as ps
from cfun_amd import _lib, ops
from cfun_amd._lib import ALGO_AUTO, ALGO_MFMA, ALGO_WINO, ptr
from membound_cases import _refused
from product_shapes import PRO_LRELU, PRO_NORM, case_sig as S

CFUN_OK, CFUN_EINVAL, CFUN_EWORKSPACE, CFUN_EALIGN = 0, -1, -2, -3
K1, K3, K5, K2 = (1, 1, 1), (3, 3, 3), (5, 5, 5), (2, 2, 2)
P0 = (0, 0, 0)
POINTWISE_MIN_VOXELS = 32768          # cfun_conv_pointwise_supported: N * V_out at and above which the streaming kernel runs

CASES = {}


def _add(name, sig, fwd, dgrad, wgrad, dgrad_op=None):
    assert name not in CASES, name
    CASES[name] = (sig, (fwd, dgrad, wgrad, dgrad_op))


# ---- pointwise 1x1x1 -> 8 (k_conv_pointwise) against the MFMA 1x1x1 kernel
_add("pw_at_threshold", S(1, (32, 32, 32), 8, 8, K1), "pointwise", "mfma", "mfma")                     # N * V = 32768 exactly
_add("pw_one_row_below", S(1, (33, 31, 32), 8, 8, K1), "mfma", "mfma", "mfma")                          # 32768 - 32
# pad 1: the output grid is larger than the input's and the pointwise kernel indexes x by the output voxel
_add("pw_pad1", S(1, (30, 32, 32), 8, 8, K1, pad=(1, 1, 1)), "mfma", "direct", "mfma")
_add("pw_ci12_scalen_resup2", S(2, (16, 32, 34), 12, 8, K1, scale=True, per_n=True, res=True, res_up2=True),
     "pointwise", "mfma", "mfma")
# the input prologue's (mean, rstd) table: N * C_in * 8 bytes = 48 KB exactly (the sample above: check_pointwise_prologue_limit)
_add("pw_prologue_48k", S(96, (4, 8, 11), 64, 8, K1, pro=PRO_NORM), "pointwise", "mfma", "mfma")

# ---- the C_in = 1 stems (k_conv_stem, k_wgrad_c1_mfma)
_add("stem_k333_pad0", S(1, (5, 6, 18), 1, 20, K3, pad=P0), "stem", "direct", "c1")
_add("stem_k377_pad", S(1, (7, 11, 13), 1, 16, (3, 7, 7), stride=2, pad=(0, 2, 3)), "stem", "direct", "c1")
_add("stem_k577_pad", S(1, (7, 9, 9), 1, 24, (5, 7, 7), stride=2, pad=(1, 3, 2)), "stem", "direct", "c1")
_add("stem_k377_odd", S(1, (7, 11, 13), 1, 16, (3, 7, 7), stride=2), "stem", "direct", "c1")
_add("stem_k577_odd", S(1, (7, 9, 9), 1, 24, (5, 7, 7), stride=2), "stem", "direct", "c1")
_add("stem_k333_odd_two_samples", S(2, (5, 7, 19), 1, 20, K3, shift=True, scale=True), "stem", "direct", "c1")
_add("stem_co_off_list", S(1, (5, 6, 18), 1, 24, K3), "direct", "direct", "c1")
_add("stem_res", S(1, (5, 6, 18), 1, 20, K3, res=True), "direct", "direct", "c1")
_add("c1_d2s_16", S(1, (5, 6, 18), 1, 16, K3, d2s=True), "direct", "direct", "direct")
_add("c1_d2s_32", S(2, (4, 5, 7), 1, 32, K3, d2s=True), "direct", "direct", "direct")
_add("c1_co36", S(1, (5, 6, 18), 1, 36, K3), "direct", "direct", "direct")                               # CoP = 48 > 32

# ---- mfma_shape
_add("ci6", S(1, (5, 6, 9), 6, 8, K3), "direct", "direct", "direct")
_add("co6", S(1, (5, 6, 9), 8, 6, K3), "direct", "direct", "direct")
_add("k555_co8", S(1, (6, 7, 9), 8, 8, K5), "mfma", "mfma", "mfma")
_add("k555_co16", S(1, (6, 7, 9), 8, 16, K5), "mfma", "mfma", "mfma")
_add("k555_co32", S(1, (6, 7, 9), 8, 32, K5), "direct", "mfma", "direct")                                # max_nsub = 1
_add("k555_ci32", S(1, (6, 7, 9), 32, 8, K5), "mfma", "direct", "mfma")                                  # ... of the mirrored conv
_add("k222_pad0", S(1, (5, 6, 9), 8, 16, K2, pad=P0), "mfma", "mfma", "mfma")
_add("k222_pad1", S(1, (5, 6, 9), 8, 16, K2, pad=(1, 1, 1)), "mfma", "mfma", "mfma")
_add("k133_pad002", S(1, (5, 6, 9), 8, 16, (1, 3, 3), pad=(0, 0, 2)), "mfma", "mfma", "mfma")
_add("k311_pad200", S(1, (5, 6, 9), 8, 16, (3, 1, 1), pad=(2, 0, 0)), "mfma", "mfma", "mfma")
_add("k311_pad010", S(1, (5, 6, 9), 8, 16, (3, 1, 1), pad=(1, 1, 0)), "mfma", "direct", "mfma")          # ph > kh - 1
_add("k133_stride2", S(1, (5, 8, 9), 8, 16, (1, 3, 3), stride=2), "direct", "direct", "direct")          # no shape entry
_add("d2s_cqp6", S(1, (4, 5, 6), 8, 48, K3, d2s=True), "direct", "direct", "direct")                     # Co / 8 = 6
_add("d2s_cq6", S(1, (4, 5, 6), 8, 64, K3, d2s=True, d2s_cq=6), "direct", "direct", "direct")
_add("d2s_cq4_of_8", S(1, (4, 5, 6), 8, 64, K3, d2s=True, d2s_cq=4), "mfma", "mfma", "mfma")

# ---- the Winograd thresholds under AUTO (cfun_wino_supported, cfun_wino_shape_ok, cfun_wino_wgrad_supported)
_add("wino_16_32", S(1, (5, 6, 9), 16, 32, K3), "wino", "mfma", "wino", "packT")
_add("wino_12_32", S(1, (5, 6, 9), 12, 32, K3), "mfma", "mfma", "wino", "packT")
_add("wino_16_28", S(1, (5, 6, 9), 16, 28, K3), "mfma", "mfma", "wino", "packT")
_add("wino_32_32_both", S(2, (5, 6, 9), 32, 32, K3, act=2, shift=True, res=True), "wino", "wino", "wino")
_add("wino_ph0", S(1, (5, 6, 9), 16, 32, K3, pad=(1, 0, 1)), "mfma", "mfma", "mfma", "packT")
_add("wino_pw2", S(1, (5, 6, 9), 16, 32, K3, pad=(1, 1, 2)), "mfma", "mfma", "mfma", "packT")
_add("wino_pd0", S(1, (5, 6, 9), 32, 32, K3, pad=(0, 1, 1)), "wino", "wino", "wino")
_add("wino_pd2", S(1, (5, 6, 9), 32, 32, K3, pad=(2, 1, 1)), "wino", "wino", "wino")
_add("wino_pd3", S(1, (5, 6, 9), 32, 32, K3, pad=(3, 1, 1)), "mfma", "direct", "mfma", "packT")
_add("wino_w1", S(1, (4, 5, 1), 16, 32, K3), "wino", "mfma", "wino", "packT")
_add("wino_h1_w2", S(1, (4, 1, 2), 32, 32, K3), "wino", "wino", "wino")
_add("wino_forced_d2s_cq", S(1, (4, 5, 6), 8, 64, K3, d2s=True, d2s_cq=4, algo=ALGO_WINO), "wino", "mfma", "wino", "packT")
_add("wino_forced_d2s", S(1, (4, 5, 6), 8, 64, K3, d2s=True, algo=ALGO_WINO), "wino", "wino", "wino")
# the weight gradient's own channel rule: C_in <= 8 and 17..20 stay on k_wgrad_mfma
_add("wgrad_ci8", S(1, (5, 6, 9), 8, 16, K3), "mfma", "mfma", "mfma", "packT")
_add("wgrad_ci12", S(1, (5, 6, 9), 12, 16, K3), "mfma", "mfma", "wino", "packT")
_add("wgrad_ci20", S(1, (5, 6, 9), 20, 16, K3), "mfma", "mfma", "mfma", "packT")
_add("wgrad_ci24", S(1, (5, 6, 9), 24, 16, K3), "mfma", "mfma", "wino", "packT")

# ---- stride 2: odd extents make the high-side bound test (vz < Dv and its twins) the deciding one, and are the only way to
# the direct data gradient of a 3x3x3 stride-2 conv under AUTO / MFMA
_add("s2_even_folded", S(1, (8, 8, 12), 4, 40, K3, stride=2), "mfma", "s2fold", "mfma", "s2fold")
for _algo, _tag in ((ALGO_AUTO, "auto"), (ALGO_MFMA, "mfma")):
    _add("s2_odd_all_" + _tag, S(2, (7, 9, 11), 4, 40, K3, stride=2, algo=_algo), "mfma", "direct", "mfma", "packT")
    _add("s2_odd_all_pro_" + _tag, S(2, (7, 9, 11), 4, 40, K3, stride=2, algo=_algo, pro=PRO_NORM), "mfma", "direct", "mfma",
         "packT")
_add("s2_odd_x", S(1, (8, 8, 9), 4, 40, K3, stride=2), "mfma", "direct", "mfma", "packT")
_add("s2_odd_x_pro", S(1, (8, 8, 9), 4, 40, K3, stride=2, pro=PRO_LRELU), "mfma", "direct", "mfma", "packT")
_add("s2_odd_z", S(1, (9, 8, 8), 8, 16, K3, stride=2), "mfma", "direct", "mfma", "packT")
_add("s2_odd_y", S(1, (8, 9, 8), 8, 16, K3, stride=2), "mfma", "direct", "mfma", "packT")
_add("s2_odd_20_40", S(1, (7, 9, 11), 20, 40, K3, stride=2), "mfma", "direct", "mfma", "packT")        # remainder tile
_add("s2_odd_20_40_pro", S(1, (7, 9, 11), 20, 40, K3, stride=2, pro=PRO_NORM), "mfma", "direct", "mfma", "packT")
_add("s2_k111_odd", S(2, (7, 9, 11), 8, 16, K1, stride=2), "mfma", "direct", "mfma", "packT")
_add("s2_k111_odd_pro", S(2, (7, 9, 11), 8, 16, K1, stride=2, pro=PRO_NORM), "mfma", "direct", "mfma", "packT")
_add("s2_k111_odd_x33", S(1, (3, 5, 33), 16, 40, K1, stride=2, act=2, shift=True), "mfma", "direct", "mfma", "packT")
for _algo, _tag in ((ALGO_AUTO, "auto"), (ALGO_MFMA, "mfma")):
    _add("s2_d2s_4_64_" + _tag, S(1, (8, 8, 12), 4, 64, K3, stride=2, d2s=True, algo=_algo), "mfma", "direct", "mfma", "packT")
_add("s2_d2s_8_32", S(1, (8, 8, 12), 8, 32, K3, stride=2, d2s=True), "mfma", "direct", "mfma", "packT")
_add("s2_k111_d2s", S(1, (8, 8, 12), 8, 32, K1, stride=2, d2s=True), "mfma", "direct", "mfma", "packT")

# ---- the data gradient (make_dgrad_params, use_mfma_dgrad)
_add("dgrad_pad3", S(1, (4, 5, 6), 8, 16, K3, pad=(3, 3, 3)), "mfma", "direct", "mfma", "packT")          # pad > k - 1
_add("dgrad_k111_pad1", S(1, (4, 5, 6), 8, 16, K1, pad=(1, 1, 1)), "mfma", "direct", "mfma", "packT")
_add("dgrad_pad2", S(1, (4, 5, 6), 8, 16, K3, pad=(2, 2, 2)), "mfma", "mfma", "mfma", "packT")
_add("dgrad_up2_odd", S(1, (3, 5, 7), 8, 16, K3, up2=True), "mfma", "mfma", "mfma", "packT")
_add("dgrad_k111_d2s", S(1, (4, 5, 6), 8, 32, K1, d2s=True), "mfma", "direct", "mfma", "packT")           # s2d gather: 3x3x3 only
_add("dgrad_k333_d2s", S(1, (4, 5, 6), 8, 32, K3, d2s=True), "mfma", "wino", "mfma")      # (cfun_wino_s2d_dgrad_supported: no channel rule)
_add("dgrad_k133_d2s", S(1, (4, 5, 6), 8, 32, (1, 3, 3), d2s=True), "mfma", "direct", "mfma", "packT")

# ---- degenerate volumes under 3x3x3
_add("vol_1", S(1, (1, 1, 1), 8, 16, K3), "mfma", "mfma", "mfma", "packT")
_add("vol_2", S(2, (2, 2, 2), 8, 16, K3), "mfma", "mfma", "mfma", "packT")
_add("vol_1_wino", S(1, (1, 1, 1), 32, 32, K3), "wino", "wino", "wino")
_add("vol_2_direct", S(2, (2, 2, 2), 6, 10, K3), "direct", "direct", "direct")


def _params(s):
    return ops._params(ps._spec(s), (s.n,) + s.dhw + (s.ci,), bool(s.scale_mode), bool(s.has_shift), bool(s.res_mode))


def families(s):
    """(forward, data gradient, weight gradient, data-gradient operand kind) of s, through the queries."""
    info, bwd = ps.kernel_info(s), ps.bwd_kernels(s)
    return info["fwd"], bwd["dgrad"], bwd["wgrad"], info["kinds"][1]


def check_families(name):
    """The case sits on the side of its boundary the table says; the weight-gradient tile query refuses exactly the C_in = 1
    and direct weight gradients; the data-gradient operand kind follows the data-gradient family."""
    s, (fwd, dgrad, wgrad, dgrad_op) = CASES[name]
    got = families(s)
    assert got[:3] == (fwd, dgrad, wgrad), "%s runs (fwd, dgrad, wgrad) = %s, the table says %s" % (name, got[:3], (fwd, dgrad, wgrad))
    assert ps.bwd_kernels(s)["wgrad_tile"] == (wgrad not in ("c1", "direct")), name
    if got[3] not in ("none", "?"):
        assert (got[3] == "s2fold") == (dgrad == "s2fold") and (got[3] in ("wino1T", "wino2T")) == (dgrad == "wino"), (name, got)
    if dgrad_op is not None:
        assert got[3] == dgrad_op, "%s: the data gradient reads %s, the table says %s" % (name, got[3], dgrad_op)


def run_scoped(s, device):
    """y, dx, dw of s with a parameter weight inside ops.WeightScope: pass 1 packs per conv, pass 2 takes its operands from the
    scope's one cfun_weight_prepare launch.  Returns the two passes and the second scope."""
    t = ps.make_tensors(s, device)

    def dev(v):
        return None if v is None else v.to(device)
    w = torch.nn.Parameter(t["w"].to(device))
    owner, runs, scope = torch.nn.Module(), [], None
    for _ in range(2):
        x = t["x"].clone().to(device).requires_grad_(True)
        w.grad = None
        xin = x if not s.pro else ops.NormedInput(x, dev(t["in_stats"]), ops.ACT_LRELU, ops.LRELU_SLOPE)
        with ops.WeightScope(owner) as scope:
            y = ops.conv3d_w(xin, w, ps._spec(s), scale=dev(t["scale"]), shift=dev(t["shift"]), res=dev(t["res"]))
            y.backward(dev(t["gy"]))
        runs.append((y.detach().clone(), x.grad.clone(), w.grad.clone()))
    return runs, scope


def check_case(device, name, emit=print):
    s, _ = CASES[name]
    check_families(name)
    # first under guard bands (tests/guard.py): operands shadowed between NaN bands, workspaces exactly as large as the
    # queries say -- a read outside an operand shows as a NaN, a write outside an output changes a band
    with guard.guarded_memory():
        got = ps.run_kernels(s, ps.make_tensors(s, device), device)
        guard.verify()
    for q in ("y", "dx", "dw", "dshift", "dres"):
        assert got[q] is None or bool(torch.isfinite(got[q]).all()), "%s: %s holds a non-finite value under guard" % (name, q)
    rep = ps.replay(s, device)
    emit(ps.format_row(rep))
    assert not rep["failures"], "\n".join(rep["failures"])
    kinds = rep["info"]["kinds"]
    if kinds != ("pack", "packT"):
        (first, second), scope = run_scoped(s, device)
        if "none" not in kinds and "?" not in kinds:
            assert scope.hits == 1 and scope.misses == 0, (name, kinds, scope.hits, scope.misses)
        for a, b, q in zip(first, second, ("y", "dx", "dw")):
            assert torch.equal(a, b), "%s: %s differs with prepared operands (%s)" % (name, q, "/".join(kinds))
    return rep


# ================================================================================================ through the C entries
GUARD = 64          # floats either side of an output: 256 bytes, so the output itself stays 16-byte aligned


def _guarded(shape, device):
    """(whole buffer, the output view in its middle)."""
    n = 1
    for d in shape:
        n *= d
    buf = torch.empty(n + 2 * GUARD, device=device)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _operands(s, device):
    """Device operands of the plain C entries for s: x, packed weight, its transpose, g (conv-sum gradient in y's layout)."""
    t = ps.make_tensors(s, device)
    wp = ops.pack_weight(t["w"].to(device)).detach().contiguous()
    return dict(x=t["x"].to(device).contiguous(), wp=wp, wpT=ops._transpose_pack(wp, s.co), g=t["gy"].to(device).contiguous())


def _mis(t):
    """The same values one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, device=t.device)
    off = 1 + (-(buf.data_ptr() // 4)) % 4
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _ws(nbytes, like):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=like.device)


def _fwd(lib, o, y, p, ws=None, ws_bytes=None, x=None):
    x = o["x"] if x is None else x
    return int(lib.cfun_conv3d_fwd(ptr(x), ptr(o["wp"]), None, None, None, ptr(y), C.byref(p), ptr(ws),
                                   (0 if ws is None else ws.numel()) if ws_bytes is None else ws_bytes, _lib.stream(x)))


def _dgrad(lib, o, dx, p, ws=None, ws_bytes=None):
    return int(lib.cfun_conv3d_bwd_data(ptr(o["g"]), ptr(o["wpT"]), ptr(dx), C.byref(p), ptr(ws),
                                        (0 if ws is None else ws.numel()) if ws_bytes is None else ws_bytes, _lib.stream(o["g"])))


def _wgrad(lib, o, dw, p):
    ws = _ws(lib.cfun_conv3d_bwd_weight_workspace_bytes(C.byref(p)), o["x"])
    return int(lib.cfun_conv3d_bwd_weight_oidhw(ptr(o["x"]), ptr(o["g"]), ptr(dw), C.byref(p), ptr(ws), ws.numel(), _lib.stream(o["x"])))


def check_pointwise_misaligned(device):
    """x or y off 16-byte alignment at a pointwise shape: the streaming kernel needs float4 rows, the call falls to the MFMA
    side, which answers CFUN_EALIGN and leaves y alone; the aligned call runs."""
    lib = _lib.load()
    s = CASES["pw_at_threshold"][0]
    assert families(s)[0] == "pointwise"
    o, p = _operands(s, device), _params(s)
    buf, y = _guarded(ps.y_shape(s), device)
    ybuf_m = torch.empty(y.numel() + 8, device=device)
    off = 1 + (-(ybuf_m.data_ptr() // 4)) % 4
    ym = ybuf_m[off:off + y.numel()].view(y.shape)
    _refused(CFUN_EALIGN, lambda: _fwd(lib, o, y, p, x=_mis(o["x"])), [buf], "pointwise shape, x misaligned")
    _refused(CFUN_EALIGN, lambda: _fwd(lib, o, ym, p), [ybuf_m], "pointwise shape, y misaligned")
    assert _fwd(lib, o, y, p) == CFUN_OK
    want = ops.conv3d(o["x"], o["wp"], ps._spec(s))
    assert torch.equal(y, want)


def check_pointwise_prologue_limit(device):
    """One sample above the 48 KB table: the pointwise kernel has no room for the prologue.  The support query says so, the C
    entry refuses the fused call and leaves y alone, and ``ops`` materialises the input: the recorded call carries no
    prologue and is right against fp64."""
    lib = _lib.load()
    at = CASES["pw_prologue_48k"][0]
    assert at.n * at.ci * 2 * 4 == 48 * 1024
    assert int(lib.cfun_conv3d_fused_support(C.byref(_params(at)))) & _lib.FUSE_IN_NORM
    s = at._replace(n=at.n + 1)
    p = _params(s)
    assert families(s)[0] == "pointwise" and int(lib.cfun_conv3d_fused_support(C.byref(p))) == 0
    t = ps.make_tensors(s, device)
    o = _operands(s, device)
    stats = t["in_stats"].to(device).contiguous()
    buf, y = _guarded(ps.y_shape(s), device)
    fz = _lib.ConvFusion(stats.data_ptr(), ops.ACT_LRELU, ops.LRELU_SLOPE, None, 0.0)
    ws = _ws(lib.cfun_conv3d_fwd_fused_workspace_bytes(C.byref(p), C.byref(fz)), y)
    _refused(CFUN_EINVAL, lambda: int(lib.cfun_conv3d_fwd_fused(ptr(o["x"]), ptr(o["wp"]), None, None, None, ptr(y), C.byref(p),
                                                               C.byref(fz), ptr(ws), ws.numel(), _lib.stream(y))),
             [buf], "pointwise prologue above 48 KB")
    got = ps.run_kernels(s, t, device)
    assert got["recorded"] == [s._replace(pro=ps.PRO_NONE)], [ps.sig_id(r) for r in got["recorded"]]
    rep = ps.replay(s._replace(pro=ps.PRO_NONE), device)
    assert not rep["failures"], "\n".join(rep["failures"])
    return rep


def _wino_bytes(lib, p):
    """cfun_wino_workspace_bytes(p) (conv3d_wino.hip): the library's internal threshold between the Winograd kernel and its
    fallback, a C++ symbol of the shared object (no entry of the C ABI reports it by itself)."""
    fn = getattr(lib, "_Z25cfun_wino_workspace_bytesPK16CfunConv3dParams")
    fn.restype, fn.argtypes = C.c_size_t, [C.POINTER(_lib.ConvParams)]
    return int(fn(C.byref(p)))


def check_wino_workspace_fallback(device):
    """A Winograd-eligible forward (16 -> 32) and data gradient (32 -> 16, whose mirrored conv is 16 -> 32) without a
    workspace, and with one byte less than the Winograd kernel needs: the MFMA kernel serves, bit for bit the forced-MFMA run
    (C_in = 16 of the conv that runs: fewer than 8 channel chunks, K is never split).  With prepared operands no plain kernel can
    read the weight: CFUN_EWORKSPACE and an untouched output."""
    lib = _lib.load()
    # forward
    s = ps.case_sig(1, (5, 6, 9), 16, 32, K3)
    assert families(s)[0] == "wino"
    o, p = _operands(s, device), _params(s)
    pm = _params(s._replace(algo=ALGO_MFMA))
    need = _wino_bytes(lib, p)
    assert 0 < need <= int(lib.cfun_conv3d_fwd_workspace_bytes(C.byref(p)))
    buf, y = _guarded(ps.y_shape(s), device)
    ref = torch.empty_like(y)
    assert _fwd(lib, o, ref, pm) == CFUN_OK
    full = _ws(need, y)
    assert _fwd(lib, o, y, p, full) == CFUN_OK                          # the Winograd kernel: another summation order
    assert ps.kc.rel_err(y, ref) < 1e-4 and not torch.equal(y, ref)
    for ws, nbytes, what in ((None, 0, "no workspace"), (full, need - 1, "workspace one byte short")):
        buf.fill_(777.0)
        assert _fwd(lib, o, y, p, ws, nbytes) == CFUN_OK, what
        assert torch.equal(y, ref), "forward, %s: not the MFMA kernel's result" % what
        assert bool((buf[:GUARD] == 777.0).all()) and bool((buf[-GUARD:] == 777.0).all()), what
        p.w_prepared = 1
        _refused(CFUN_EWORKSPACE, lambda: _fwd(lib, o, y, p, ws, nbytes), [buf], "prepared forward, " + what)
        p.w_prepared = 0
    # data gradient
    s = ps.case_sig(1, (5, 6, 9), 32, 16, K3)
    assert families(s)[1] == "wino"
    o, p = _operands(s, device), _params(s)
    pm = _params(s._replace(algo=ALGO_MFMA))
    q = _params(ps.case_sig(1, (5, 6, 9), 16, 32, K3))                  # the mirrored conv: g [.., 16] -> dx [.., 32]
    need = _wino_bytes(lib, q)
    assert 0 < need <= int(lib.cfun_conv3d_bwd_data_workspace_bytes(C.byref(p)))
    buf, dx = _guarded(tuple(o["x"].shape), device)
    ref = torch.empty_like(dx)
    assert _dgrad(lib, o, ref, pm) == CFUN_OK
    full = _ws(need, dx)
    assert _dgrad(lib, o, dx, p, full) == CFUN_OK
    assert ps.kc.rel_err(dx, ref) < 1e-4 and not torch.equal(dx, ref)
    for ws, nbytes, what in ((None, 0, "no workspace"), (full, need - 1, "workspace one byte short")):
        buf.fill_(777.0)
        assert _dgrad(lib, o, dx, p, ws, nbytes) == CFUN_OK, what
        assert torch.equal(dx, ref), "data gradient, %s: not the MFMA kernel's result" % what
        assert bool((buf[:GUARD] == 777.0).all()) and bool((buf[-GUARD:] == 777.0).all()), what
        p.w_prepared = 2
        _refused(CFUN_EWORKSPACE, lambda: _dgrad(lib, o, dx, p, ws, nbytes), [buf], "prepared data gradient, " + what)
        p.w_prepared = 0


def check_short_workspace_refused(device):
    """The up2 data gradient (its full-resolution gradient lives in the workspace) and the folded stride-2 data gradient (its
    folded weights do) with the workspace one byte short: CFUN_EWORKSPACE, dx and the canaries either side untouched; the
    full workspace runs."""
    lib = _lib.load()
    for name in ("dgrad_up2_odd", "s2_even_folded"):
        s = CASES[name][0]
        o, p = _operands(s, device), _params(s)
        need = int(lib.cfun_conv3d_bwd_data_workspace_bytes(C.byref(p)))
        assert need > 256, name
        ws = _ws(need, o["x"])
        buf, dx = _guarded(tuple(o["x"].shape), device)
        _refused(CFUN_EWORKSPACE, lambda: _dgrad(lib, o, dx, p, ws, need - 1), [buf], name + ", workspace one byte short")
        _refused(CFUN_EWORKSPACE, lambda: _dgrad(lib, o, dx, p, None, 0), [buf], name + ", no workspace")
        assert _dgrad(lib, o, dx, p, ws, need) == CFUN_OK, name
        assert bool((buf[:GUARD] == 777.0).all()) and bool((buf[-GUARD:] == 777.0).all()), name
        assert bool(torch.isfinite(dx).all()) and float(dx.abs().max()) > 0 and not bool((dx == 777.0).any()), name


def check_algo_mfma_refused(device):
    """CFUN_ALGO_MFMA on a shape with no MFMA kernel (C_in = 6): CFUN_EINVAL on the forward and the weight gradient, outputs
    untouched; the data gradient ("MFMA where one exists") runs on the direct kernel."""
    lib = _lib.load()
    s = CASES["ci6"][0]._replace(algo=ALGO_MFMA)
    o, p = _operands(s, device), _params(s)
    ybuf, y = _guarded(ps.y_shape(s), device)
    _refused(CFUN_EINVAL, lambda: _fwd(lib, o, y, p), [ybuf], "ALGO_MFMA forward without an MFMA kernel")
    wbuf, dw = _guarded((s.co, s.ci) + s.k, device)
    _refused(CFUN_EINVAL, lambda: _wgrad(lib, o, dw, p), [wbuf], "ALGO_MFMA weight gradient without an MFMA kernel")
    dbuf, dx = _guarded(tuple(o["x"].shape), device)
    dbuf.fill_(777.0)
    assert _dgrad(lib, o, dx, p) == CFUN_OK
    pa = _params(s._replace(algo=ALGO_AUTO))
    ref = torch.empty_like(dx)
    assert _dgrad(lib, o, ref, pa) == CFUN_OK and torch.equal(dx, ref)
    assert bool((dbuf[:GUARD] == 777.0).all()) and bool((dbuf[-GUARD:] == 777.0).all())


# Empty problems.  The library's answer: a conv over no samples, or whose output grid has no voxel, is a valid call on all
# three passes -- return code 0, y has no element, and the gradients are the empty sums: dx (where x has elements) and dw are
# exact zeros.  Nothing outside the outputs is written.
EMPTY_CASES = {
    "n0_mfma": ps.case_sig(0, (4, 5, 6), 8, 16, K3),
    "n0_wino_shape": ps.case_sig(0, (4, 5, 6), 32, 32, K3),
    "n0_direct": ps.case_sig(0, (4, 5, 6), 6, 10, K3),
    "n0_stem": ps.case_sig(0, (4, 5, 6), 1, 20, K3),
    "n0_pointwise_shape": ps.case_sig(0, (4, 5, 6), 8, 8, K1),
    "no_output_mfma": ps.case_sig(2, (2, 5, 6), 8, 16, K3, pad=(0, 1, 1)),
    "no_output_direct": ps.case_sig(2, (2, 5, 6), 6, 10, K3, pad=(0, 1, 1)),
    "no_output_stem": ps.case_sig(2, (2, 5, 6), 1, 20, K3, pad=(0, 1, 1)),
}


def check_empty(device, name):
    lib = _lib.load()
    s = EMPTY_CASES[name]
    assert s.n * ps.out_dims(s)[0] == 0
    o, p = _operands(s, device), _params(s)
    ybuf, y = _guarded(ps.y_shape(s), device)
    dbuf, dx = _guarded(tuple(o["x"].shape), device)
    wbuf, dw = _guarded((s.co, s.ci) + s.k, device)
    for b in (ybuf, dbuf, wbuf):
        b.fill_(777.0)
    assert y.numel() == 0 and o["g"].numel() == 0
    fwd_ws = _ws(lib.cfun_conv3d_fwd_workspace_bytes(C.byref(p)), y)
    dg_ws = _ws(lib.cfun_conv3d_bwd_data_workspace_bytes(C.byref(p)), y)
    rcs = (_fwd(lib, o, y, p, fwd_ws), _dgrad(lib, o, dx, p, dg_ws), _wgrad(lib, o, dw, p))
    assert rcs == (CFUN_OK, CFUN_OK, CFUN_OK), "%s: (forward, data gradient, weight gradient) returned %s" % (name, rcs)
    assert bool((ybuf == 777.0).all()), name + ": the forward wrote"
    assert bool((dx == 0).all()) and bool((dw == 0).all()), name + ": the gradients of an empty conv are zeros"
    for b in (dbuf, wbuf):
        assert bool((b[:GUARD] == 777.0).all()) and bool((b[-GUARD:] == 777.0).all()), name
    # the same through the autograd binding (the forward workspace query used to divide by the workgroup count)
    got = ps.run_kernels(s, ps.make_tensors(s, device), device)
    assert tuple(got["y"].shape) == ps.y_shape(s) and got["y"].numel() == 0, name
    assert tuple(got["dx"].shape) == tuple(o["x"].shape) and not bool(got["dx"].any()) and not bool(got["dw"].any()), name
