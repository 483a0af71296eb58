"""The convs a real training step issues, each checked on its own at its true shape against fp64.

Shared by the CPU tier (HIP emulator, tests/test_product_shapes_emu.py) and the GPU tier (tests/test_product_shapes_gpu.py):

* ``record()`` captures every call that passes ``ops._Conv3d.forward`` -- the one place all convs go through -- and
  reduces it to a hashable ``Sig``: everything that can change the kernel or its indexing, no pointers, no ``w_prepared``.
* ``replay()`` rebuilds seeded random tensors from a ``Sig``, calls ``ops.conv3d_w`` / ``ops.conv3d`` the way the step did
  and compares
    - y and dx on BOXES cut from the volumes (corners, faces, the seam between the last full 4x4x16 tile and the ragged
      remainder of each axis, the planes either side of a sample boundary, seeded interior boxes): the plain torch
      formulation (``kernel_cases.ref_conv``) on the crop with its kernel halo, zero-padded only where the box touches
      the volume border, in float64;
    - dw, dshift and dres in FULL (every voxel) in float64; dw tap by tap as g^T . x_shifted_t, where x_shifted_t is a
      flat row offset into the zero-padded (and, for stride 2, phase-split) input -- a view, no copy per tap;
    - the statistics epilogue against the two-pass float64 statistics of the kernel's own y;
    - prologue runs bit for bit against the same kernels fed the materialised input.
  The activation's derivative in the gradient references is taken at the KERNEL's y (whose values the boxes prove): a
  pre-activation within rounding of zero can then not land on different sides in the reference and in the kernel, so the
  gradient comparison is between the backward kernels and fp64 on identical operands.
* The tolerance is a rule (``bound``): every reference is evaluated in float32 on the host as well, on the same boxes and
  the same full reductions; its deviation from float64 is e32 and the kernel must stay within
  bench.GRAD_FP64_FACTOR * e32 + bench.GRAD_FP64_FLOOR, in ``kernel_cases.rel_err``'s metric (max-abs error over max-abs of
  the reference).
"""
import ast
import contextlib
import ctypes as C
import json
import os
import sys
import time
import zlib
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the project's fp64 margin: GRAD_FP64_FACTOR, GRAD_FP64_FLOOR)
import kernel_cases as kc  # noqa: E402
from cfun_amd import _lib, ops  # noqa: E402
from cfun_amd._lib import ACT_LRELU, ACT_NONE, ACT_RELU  # noqa: E402

MANIFEST = os.path.join(ROOT, "tests", "golden", "product_shapes_signatures.json")
TILE = (4, 4, 16)           # output tile of the conv kernels (z, y, x)
BOX = (6, 6, 34)            # a whole tile plus its seams, whatever the alignment in z / y; two x tiles and their seams
N_RANDOM_BOXES = 8
STATS_TOL = 2e-5            # kernel_cases.check_conv's bound on the epilogue statistics
PRO_NONE, PRO_LRELU, PRO_NORM = 0, 1, 2
KERNEL_NAMES = {0: "direct", 1: "mfma", 2: "wino", 3: "stem", 4: "pointwise"}
WOP_NAMES = {0: "none", 1: "pack", 2: "packT", 3: "wino1", 4: "wino2", 5: "wino1T", 6: "wino2T", 7: "s2fold"}
ALGO_NAMES = {0: "auto", 1: "direct", 2: "mfma", 4: "wino", 5: "wino2"}

Sig = namedtuple("Sig", "n dhw ci co cop k stride pad up2 d2s d2s_cq tap_skip res_up2 act scale_mode has_shift res_mode "
                        "algo pro stats need oidhw shift_scaled")
# need: gradients wanted for (x, weight, shift, res)


# ------------------------------------------------------------------------------------------ signatures
def signature(needs, x, wp, scale, shift, res, w_src, call):
    p, spec = call.p, call.spec
    need = dict(zip(ops._CONV_INPUTS, needs))
    pro = PRO_NONE if call.pro is None else (PRO_LRELU if call.pro[0] is None else PRO_NORM)
    return Sig(n=int(p.N), dhw=(int(p.Di), int(p.Hi), int(p.Wi)), ci=int(p.Ci), co=int(p.Co), cop=int(p.CoP),
               k=(int(p.kd), int(p.kh), int(p.kw)), stride=int(p.stride), pad=(int(p.pd), int(p.ph), int(p.pw)),
               up2=int(p.up2), d2s=int(p.d2s), d2s_cq=int(p.d2s_cq), tap_skip=int(p.tap_skip), res_up2=int(p.res_up2),
               act=int(p.act), scale_mode=int(p.scale_mode), has_shift=int(p.has_shift), res_mode=int(p.res_mode),
               algo=int(p.algo), pro=pro, stats=int(call.stats is not None),
               need=(bool(need["x"]), bool(need["wp"] or need["w_src"]), bool(need["shift"]), bool(need["res"])),
               oidhw=int(w_src is not None), shift_scaled=int(bool(call.shift_scaled)))


def case_sig(n, dhw, ci, co, k, stride=1, pad=None, up2=False, act=ACT_NONE, scale=False, shift=False, res=False,
             res_up2=False, per_n=False, algo=0, d2s=False, d2s_cq=0, pro=PRO_NONE):
    """A signature written by hand (the emulator tier's reference checks, tests/dispatch_cases.py): an OIDHW weight, every
    gradient its operands can take."""
    pad = tuple(pad) if pad is not None else tuple(kk // 2 for kk in k)
    return Sig(n=n, dhw=tuple(dhw), ci=ci, co=co, cop=(co + 15) // 16 * 16, k=tuple(k), stride=stride, pad=pad, up2=int(up2),
               d2s=int(d2s), d2s_cq=int(d2s_cq), tap_skip=0, res_up2=int(res_up2 and res), act=act,
               scale_mode=0 if not scale else (2 if per_n else 1), has_shift=int(shift), res_mode=int(res), algo=algo,
               pro=pro, stats=0, need=(True, True, bool(shift), bool(res)), oidhw=1, shift_scaled=0)


def sig_id(s):
    """A readable, stable test id: k333_s1_4x96x96x96_40to40_lrelu_res_stats."""
    parts = ["k%d%d%d" % s.k, "s%d" % s.stride, "%dx%dx%dx%d" % ((s.n,) + s.dhw), "%dto%d" % (s.ci, s.co)]
    if s.pad != tuple(kk // 2 for kk in s.k):
        parts.append("p%d%d%d" % s.pad)
    if s.up2:
        parts.append("up2")
    if s.d2s:
        parts.append("d2s%s" % (("cq%d" % s.d2s_cq) if s.d2s_cq else ""))
    if s.tap_skip:
        parts.append("tapskip")
    if s.pro:
        parts.append({PRO_LRELU: "inlrelu", PRO_NORM: "innorm"}[s.pro])
    if s.act:
        parts.append({ACT_RELU: "relu", ACT_LRELU: "lrelu"}[s.act])
    if s.scale_mode:
        parts.append({1: "scale", 2: "scalen"}[s.scale_mode])
    if s.has_shift:
        parts.append("shiftscaled" if s.shift_scaled else "shift")
    if s.res_mode:
        parts.append("resup2" if (s.res_up2 and not s.d2s) else "res")
    if s.stats:
        parts.append("stats")
    if s.algo:
        parts.append(ALGO_NAMES.get(s.algo, "algo%d" % s.algo))
    if not s.oidhw:
        parts.append("packed")
    parts.append("g" + "".join(c for c, on in zip("xwsr", s.need) if on) if any(s.need) else "nograd")
    return "_".join(parts)


def sig_to_json(s):
    return {k: (list(v) if isinstance(v, tuple) else v) for k, v in s._asdict().items()}


def sig_from_json(d):
    return Sig(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in d.items()})


def load_manifest(path=MANIFEST):
    """{configuration: [Sig, ...]} as recorded on an MI355X (``python tests/product_shapes.py --write-manifest``)."""
    with open(path) as f:
        raw = json.load(f)
    return {cfg: [sig_from_json(d) for d in sigs] for cfg, sigs in raw.items()}


class Recorder:
    def __init__(self):
        self.calls = []           # one Sig per conv call, in call order

    @property
    def sigs(self):
        """The distinct signatures, in first-seen order."""
        return list(dict.fromkeys(self.calls))


@contextlib.contextmanager
def record(rec=None):
    """Every conv call inside the block lands in ``rec.calls`` (ops._Conv3d.forward is wrapped, then restored)."""
    rec = Recorder() if rec is None else rec
    orig = ops._Conv3d.forward

    def forward(ctx, x, wp, scale, shift, res, w_src, call):
        rec.calls.append(signature(ctx.needs_input_grad, x, wp, scale, shift, res, w_src, call))
        return orig(ctx, x, wp, scale, shift, res, w_src, call)

    ops._Conv3d.forward = staticmethod(forward)
    try:
        yield rec
    finally:
        ops._Conv3d.forward = staticmethod(orig)


def count_conv_nodes(*roots):
    """_Conv3d nodes in the autograd graph below the tensors ``roots``."""
    seen, todo, n = set(), [r.grad_fn for r in roots if r is not None and r.grad_fn is not None], 0
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        n += type(fn).__name__ == "_Conv3dBackward"
        todo.extend(f for f, _ in fn.next_functions)
    return n


def fixed_dropout_masks(cfg, n_pos, seed=1):
    """The Dropout3d masks test_cfg2_full_size_step_properties fixes (so the sparse-dropout convs appear, reproducibly)."""
    if getattr(cfg, "UNET_DROPOUT", 0.6) <= 0:
        return None
    b = cfg.UNET_MASK_BRANCH_CHANNEL
    gen = torch.Generator().manual_seed(seed)
    return [torch.empty(n_pos, c).bernoulli_(0.4, generator=gen) / 0.4 for c in (b, 2 * b, 4 * b, 8 * b, 16 * b)]


def record_step(cfg, device, n_pos=None, backward=True):
    """One seeded training step of ``cfg`` under the recorder -> (Recorder, number of _Conv3d autograd nodes or None)."""
    from cfun_amd import step
    torch.manual_seed(0)
    net = step.CFUNHotPath(cfg).to(device)
    s = step.synthetic_inputs(cfg, device, 0)
    if n_pos is not None:
        s["p_rois"], s["mask_labels"] = s["p_rois"][:n_pos], s["mask_labels"][:n_pos]
        s["n_rois"] = s["n_rois"][:2 * n_pos]
        keep = list(range(n_pos)) + list(range(4, 4 + 2 * n_pos))
        s["target_class_ids"], s["target_deltas"] = s["target_class_ids"][keep], s["target_deltas"][keep]
    if getattr(net, "mask", None) is not None and hasattr(net.mask, "modified_u_net"):
        net.mask.modified_u_net.dropout_masks = fixed_dropout_masks(cfg, s["p_rois"].shape[0])
    nodes = None
    with record() as rec:
        if backward:
            step.training_step(net, s)
        else:
            out = net.predict_training(s["image"], s["p_rois"], s["n_rois"], lazy_rois=True, defer_mask_probs=True)
            losses = net.compute_losses(out, s["rpn_match"], s["rpn_bbox_t"], s["target_class_ids"], s["target_deltas"],
                                        s["mask_labels"])
            nodes = count_conv_nodes(net.total_loss(losses))
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    return rec, nodes


# ------------------------------------------------------------------------------------------ geometry
def out_dims(s):
    sh = 2 if s.up2 else 1
    return tuple((d * sh + 2 * p - k) // s.stride + 1 for d, p, k in zip(s.dhw, s.pad, s.k))


def y_shape(s):
    do, ho, wo = out_dims(s)
    if s.d2s:
        return (s.n, 2 * do, 2 * ho, 2 * wo, s.d2s_cq or s.co // 8)
    return (s.n, do, ho, wo, s.co)


def res_shape(s):
    do, ho, wo = out_dims(s)
    if s.d2s:
        return (s.n, do, ho, wo, s.d2s_cq or s.co // 8)
    if s.res_up2:
        return (s.n, do // 2, ho // 2, wo // 2, s.co)
    return (s.n, do, ho, wo, s.co)


def live_rows(s):
    """Rows of the weight that produce channels of y: all of them, or for a depth-to-space conv with padded parity groups
    (d2s_cq < Co / 8) the first d2s_cq of each group."""
    if not (s.d2s and s.d2s_cq and s.d2s_cq != s.co // 8):
        return None
    cqp = s.co // 8
    return torch.tensor([par * cqp + o for par in range(8) for o in range(s.d2s_cq)], dtype=torch.long)


def axis_positions(size, box, tile):
    """Start offsets of the box along one axis: low border, high border, the seam between the last full tile and the
    ragged remainder, the middle."""
    b = min(box, size)
    last = size - b
    seam = min(max((size // tile) * tile - tile - 1, 0), last)
    return dict(lo=0, hi=last, seam=seam, mid=last // 2), b


def boxes_for(dims, n, rng, box=BOX):
    """Fixed, seeded box placement over an [n, *dims] volume -> sorted list of distinct (sample, (z0,z1), (y0,y1), (x0,x1))."""
    pos, ext = zip(*(axis_positions(d, b, t) for d, b, t in zip(dims, box, TILE)))
    out = []

    def add(sample, starts):
        out.append((sample,) + tuple((int(st), int(st) + e) for st, e in zip(starts, ext)))

    i = 0
    for cz in ("lo", "hi"):                                    # the eight corners
        for cy in ("lo", "hi"):
            for cx in ("lo", "hi"):
                add(i % n, (pos[0][cz], pos[1][cy], pos[2][cx]))
                i += 1
    for ax in range(3):                                        # one box on each face
        for side in ("lo", "hi"):
            add(i % n, tuple(pos[a][side] if a == ax else pos[a]["mid"] for a in range(3)))
            i += 1
    for ax in range(3):                                        # last full tile | ragged remainder, per axis and in all three
        add(i % n, tuple(pos[a]["seam"] if a == ax else pos[a]["mid"] for a in range(3)))
        i += 1
    add(n - 1, tuple(pos[a]["seam"] for a in range(3)))
    for sample in range(min(n - 1, 3)):                        # the last planes of sample n and the first of n + 1
        yx = (pos[1]["mid"], pos[2]["mid"])
        add(sample, (pos[0]["hi"],) + yx)
        add(sample + 1, (pos[0]["lo"],) + yx)
    for _ in range(N_RANDOM_BOXES):                            # seeded interior boxes
        add(int(rng.randint(n)), tuple(int(rng.randint(d - e + 1)) for d, e in zip(dims, ext)))
    return sorted(set(out))


def _axis_crop(s, ax, o0, o1):
    """Outputs [o0, o1) of axis ``ax`` read which stored input planes?  -> (source range, offset into the (up-sampled)
    source crop, length, (zero planes below, above))."""
    sh = 2 if s.up2 else 1
    lo = o0 * s.stride - s.pad[ax]
    hi = (o1 - 1) * s.stride - s.pad[ax] + s.k[ax]
    clo, chi = max(lo, 0), min(hi, s.dhw[ax] * sh)
    if s.up2:
        s0, s1 = clo // 2, (chi - 1) // 2 + 1
        return (s0, s1), clo - 2 * s0, chi - clo, (clo - lo, hi - chi)
    return (clo, chi), 0, chi - clo, (clo - lo, hi - chi)


def _prep_crop(s, xc, crops):
    """Source crop [1,d,h,w,Ci] -> the conv's input window: nearest x2, cut, zero planes where the box touches the border."""
    if s.up2:
        xc = F.interpolate(xc.permute(0, 4, 1, 2, 3), scale_factor=2, mode="nearest").permute(0, 2, 3, 4, 1)
        (_, oz, lz, _), (_, oy, ly, _), (_, ox, lx, _) = crops
        xc = xc[:, oz:oz + lz, oy:oy + ly, ox:ox + lx]
    (_, _, _, pz), (_, _, _, py), (_, _, _, px) = crops
    return F.pad(xc, (0, 0) + tuple(px) + tuple(py) + tuple(pz))


def _up_crop(r, sample, obox):
    """up2(r)[sample, obox] without up-sampling all of r."""
    sl = [slice(o0 // 2, (o1 - 1) // 2 + 1) for o0, o1 in obox]
    rc = r[sample:sample + 1, sl[0], sl[1], sl[2]]
    rc = F.interpolate(rc.permute(0, 4, 1, 2, 3), scale_factor=2, mode="nearest").permute(0, 2, 3, 4, 1)
    off = [o0 - 2 * (o0 // 2) for o0, _ in obox]
    return rc[:, off[0]:off[0] + obox[0][1] - obox[0][0], off[1]:off[1] + obox[1][1] - obox[1][0],
              off[2]:off[2] + obox[2][1] - obox[2][0]]


def _spec(s, **kw):
    d = dict(k=s.k, co=s.co, stride=s.stride, pad=s.pad, up2=bool(s.up2), act=s.act, res_up2=bool(s.res_up2),
             scale_per_n=s.scale_mode == 2, d2s=bool(s.d2s), d2s_cq=s.d2s_cq, tap_skip=bool(s.tap_skip), algo=s.algo)
    d.update(kw)
    return ops.ConvSpec(**d)


def apply_prologue(s, x, in_stats, slope=ops.LRELU_SLOPE):
    """What the conv reads in place of x: lrelu(x) or lrelu((x - mean) * rstd)."""
    if s.pro == PRO_NONE:
        return x
    if s.pro == PRO_NORM:
        st = in_stats.to(x.dtype)
        x = (x - st[..., 0].view(s.n, 1, 1, 1, s.ci)) * st[..., 1].view(s.n, 1, 1, 1, s.ci)
    return F.leaky_relu(x, slope)


# ------------------------------------------------------------------------------------------ box references
def ref_y_box(s, box, x, w, scale, shift, res):
    """y on one output box (conv-output coordinates; a depth-to-space conv's box covers twice the extent of y): the plain
    formulation on the crop.  x is the tensor the conv reads (the prologue already applied), all operands in one dtype."""
    sample, obox = box[0], box[1:]
    crops = [_axis_crop(s, ax, *obox[ax]) for ax in range(3)]
    (z, y_, x_) = [c[0] for c in crops]
    xc = _prep_crop(s, x[sample:sample + 1, z[0]:z[1], y_[0]:y_[1], x_[0]:x_[1]], crops)
    rows = live_rows(s)
    if rows is not None:
        if scale is not None or shift is not None:
            raise NotImplementedError("scale / shift on a depth-to-space conv with padded parity groups")
        w = w.index_select(0, rows)
    sc = None if scale is None else (scale[sample:sample + 1] if s.scale_mode == 2 else scale)
    rc = None
    if res is not None:
        if s.res_up2 and not s.d2s:
            rc = _up_crop(res, sample, obox)
        else:
            rc = res[sample:sample + 1, obox[0][0]:obox[0][1], obox[1][0]:obox[1][1], obox[2][0]:obox[2][1]]
    spec = _spec(s, co=w.shape[0], pad=(0, 0, 0), up2=False, res_up2=False, d2s_cq=0, tap_skip=False)
    out = kc.ref_conv(xc, w, spec, sc, shift, rc)
    want = tuple((o1 - o0) * (2 if s.d2s else 1) for o0, o1 in obox)
    assert tuple(out.shape[1:4]) == want, (tuple(out.shape), want)
    return out


def cut_y(s, y, box):
    m = 2 if s.d2s else 1
    sample, (z, y_, x_) = box[0], box[1:]
    return y[sample:sample + 1, m * z[0]:m * z[1], m * y_[0]:m * y_[1], m * x_[0]:m * x_[1]]


def ref_dx_box(s, box, w, g):
    """dx on one INPUT box from the conv-sum gradient g [N,Do,Ho,Wo,rows] (dL/d(conv sum): activation derivative and scale
    applied, depth-to-space undone): the transpose of the plain conv on the crop of every output that touches the box."""
    sample, ibox = box[0], box[1:]
    sh = 2 if s.up2 else 1
    dims = out_dims(s)
    orange = []
    for ax in range(3):
        u0, u1 = ibox[ax][0] * sh, ibox[ax][1] * sh
        o0 = max(0, -((-(u0 + s.pad[ax] - (s.k[ax] - 1))) // s.stride))
        o1 = min(dims[ax], (u1 - 1 + s.pad[ax]) // s.stride + 1)
        orange.append((o0, o1))
    out = torch.zeros((1,) + tuple(b1 - b0 for b0, b1 in ibox) + (s.ci,), dtype=g.dtype)
    if any(o1 <= o0 for o0, o1 in orange):
        return out
    crops = [_axis_crop(s, ax, *orange[ax]) for ax in range(3)]
    src = [c[0] for c in crops]
    leaf = torch.zeros((1,) + tuple(b - a for a, b in src) + (s.ci,), dtype=g.dtype, requires_grad=True)
    lin = kc.ref_conv(_prep_crop(s, leaf, crops), w, ops.ConvSpec(k=s.k, co=w.shape[0], stride=s.stride, pad=(0, 0, 0)),
                      None, None, None)
    gc = g[sample:sample + 1, orange[0][0]:orange[0][1], orange[1][0]:orange[1][1], orange[2][0]:orange[2][1]]
    assert lin.shape == gc.shape, (tuple(lin.shape), tuple(gc.shape))
    lin.backward(gc)
    # the crop covers [src) of the input; the box may reach planes no output reads (stride 2): those keep dx = 0
    sl_out, sl_in = [], []
    for ax in range(3):
        a, b = max(ibox[ax][0], src[ax][0]), min(ibox[ax][1], src[ax][1])
        sl_out.append(slice(a - ibox[ax][0], max(b, a) - ibox[ax][0]))
        sl_in.append(slice(a - src[ax][0], max(b, a) - src[ax][0]))
    out[:, sl_out[0], sl_out[1], sl_out[2]] = leaf.grad[:, sl_in[0], sl_in[1], sl_in[2]]
    return out


# ------------------------------------------------------------------------------------------ full reductions
def act_derivative(s, y, dtype):
    if s.act == ACT_NONE:
        return None
    return torch.where(y > 0, torch.ones((), dtype=dtype), torch.full((), ops.LRELU_SLOPE if s.act == ACT_LRELU else 0.0,
                                                                     dtype=dtype))


def conv_sum_gradients(s, gy, y_kernel, scale, dtype):
    """(gp, g): dL/d(pre-activation) in y's layout and dL/d(conv sum) [N,Do,Ho,Wo,rows]; the activation's derivative is
    evaluated at the kernel's own y (see the module docstring)."""
    gp = gy.to(dtype)
    da = act_derivative(s, y_kernel, dtype)
    if da is not None:
        gp = gp * da
    g = gp
    if s.d2s:       # space-to-depth: voxel (2z+pz, 2y+py, 2x+px), channel o -> voxel (z,y,x), channel (pz,py,px,o)
        n, d2, h2, w2, cq = gp.shape
        g = gp.view(n, d2 // 2, 2, h2 // 2, 2, w2 // 2, 2, cq).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(
            n, d2 // 2, h2 // 2, w2 // 2, 8 * cq)
    if scale is not None:
        sc = scale.to(dtype)
        g = g * (sc.view(s.n, 1, 1, 1, -1) if s.scale_mode == 2 else sc.view(1, 1, 1, 1, -1))
    return gp, g.contiguous()


def _gtx(gf, xf, off, threads):
    """sum_i gf[i]^T xf[i + off] over the rows both have: [L,Co], [L,Ci] -> [Co,Ci].  Cut into ``threads`` row blocks (one
    batched matmul: the blocks run in parallel, which a single tall-skinny GEMM does not) whose partial sums are added."""
    rows = gf.shape[0] - off
    ch = rows // threads
    if ch < 2048:
        return gf[:rows].t() @ xf[off:off + rows]
    a = gf[:threads * ch].view(threads, ch, gf.shape[1]).transpose(1, 2)
    acc = torch.bmm(a, xf[off:off + threads * ch].view(threads, ch, xf.shape[1])).sum(0)
    if rows > threads * ch:
        acc = acc + gf[threads * ch:rows].t() @ xf[off + threads * ch:off + rows]
    return acc


def ref_dw_full(s, x, g, dtype):
    """The complete weight gradient [rows, Ci, kd, kh, kw], every voxel, in ``dtype``: dw[:, :, t] = g^T . x_shifted_t.
    Per sample the zero-padded input is split into stride^3 phase grids (one for stride 1) of the extent of the output
    grid plus the taps' reach, g is zero-extended to the same grid, and tap t = stride * q + r is then a FLAT row offset
    of q into phase r: both operands of the matmul are views."""
    x, g = x.to(dtype), g.to(dtype)
    if s.up2:
        x = F.interpolate(x.permute(0, 4, 1, 2, 3), scale_factor=2, mode="nearest").permute(0, 2, 3, 4, 1)
    st, dims = s.stride, out_dims(s)
    grid = [dims[ax] + (s.k[ax] - 1) // st for ax in range(3)]
    hi = [st * grid[ax] - x.shape[1 + ax] - s.pad[ax] for ax in range(3)]
    assert min(hi) >= 0, hi
    rows, threads = g.shape[-1], max(1, torch.get_num_threads())
    dw = torch.zeros((rows, s.ci) + tuple(s.k), dtype=dtype)
    for n in range(s.n):
        xp = F.pad(x[n], (0, 0, s.pad[2], hi[2], s.pad[1], hi[1], s.pad[0], hi[0]))
        gq = F.pad(g[n], (0, 0, 0, grid[2] - dims[2], 0, grid[1] - dims[1], 0, grid[0] - dims[0])).reshape(-1, rows)
        phases = {}
        for a in range(s.k[0]):
            for b in range(s.k[1]):
                for c in range(s.k[2]):
                    r = (a % st, b % st, c % st)
                    if r not in phases:
                        phases[r] = xp[r[0]::st, r[1]::st, r[2]::st].reshape(-1, s.ci)
                    off = ((a // st) * grid[1] + b // st) * grid[2] + c // st
                    dw[:, :, a, b, c] += _gtx(gq, phases[r], off, threads)
    return dw


def ref_dres(s, gp):
    if not (s.d2s or s.res_up2):
        return gp
    n, d, h, w, c = gp.shape
    return gp.view(n, d // 2, 2, h // 2, 2, w // 2, 2, c).sum(dim=(2, 4, 6))


def live_tap_mask(s, rows):
    """tap_skip: only the taps {p, p+1}^3 of each output parity p carry weight (and gradient); the kernels skip the rest."""
    m = torch.zeros((8, rows // 8, 1, 3, 3, 3), dtype=torch.bool)
    for pz in range(2):
        for py in range(2):
            for px in range(2):
                m[(pz * 2 + py) * 2 + px, :, :, pz:pz + 2, py:py + 2, px:px + 2] = True
    return m.reshape(rows, 1, 3, 3, 3)


# ------------------------------------------------------------------------------------------ the rule
def bound(e32):
    return bench.GRAD_FP64_FACTOR * e32 + bench.GRAD_FP64_FLOOR


class _Err:
    """kernel_cases.rel_err accumulated over pieces: max-abs error over max-abs of the reference."""

    def __init__(self):
        self.diff, self.ref = 0.0, 0.0

    def add(self, got, ref):
        assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
        if ref.numel():
            self.diff = max(self.diff, float((got.double() - ref.double()).abs().max()))
            self.ref = max(self.ref, float(ref.double().abs().max()))

    @property
    def value(self):
        return self.diff / (self.ref + 1e-30)


def _ratio(ek, e32):
    return ek / e32 if e32 > 0 else (0.0 if ek == 0 else float("inf"))


# ------------------------------------------------------------------------------------------ replay
def make_tensors(s, device):
    """Seeded random operands of signature s (host tensors; the seed is the signature's id)."""
    gen = torch.Generator().manual_seed(zlib.crc32(sig_id(s).encode()))
    t = {}
    t["x"] = torch.randn(s.n, *s.dhw, s.ci, generator=gen)
    fan = float(s.ci * s.k[0] * s.k[1] * s.k[2]) ** 0.5
    if s.tap_skip:      # a parity-folded "nearest x2 -> 3x3x3" weight, as the step builds it (zeros at the skipped taps)
        cqp = s.co // 8
        w3 = torch.randn(s.d2s_cq or cqp, s.ci, 3, 3, 3, generator=gen) / fan
        t["w"] = ops.fold_up2_weight(w3.to(device), cqp).detach().cpu()
    else:
        t["w"] = torch.randn(s.co, s.ci, *s.k, generator=gen) / fan
    t["scale"] = None if not s.scale_mode else torch.rand(*((s.n, s.co) if s.scale_mode == 2 else (s.co,)), generator=gen) + 0.5
    t["shift"] = torch.randn(s.co, generator=gen) if s.has_shift else None
    t["res"] = torch.randn(*res_shape(s), generator=gen) if s.res_mode else None
    t["gy"] = torch.randn(*y_shape(s), generator=gen)
    t["in_stats"] = None
    if s.pro == PRO_NORM:
        t["in_stats"] = torch.stack([torch.randn(s.n, s.ci, generator=gen) * 0.5, torch.rand(s.n, s.ci, generator=gen) + 0.5], dim=-1)
    return t


def run_kernels(s, t, device, materialised=False):
    """Call the conv as the step did (or, ``materialised``, the same conv fed ``NormedInput.materialize()``, a plain tensor)
    -> dict of host tensors y, dx, dw, dshift, dres, stats + the signature the call itself recorded."""
    def dev(v, grad=False):
        return None if v is None else v.detach().clone().to(device).requires_grad_(grad)
    need_x, need_w, need_s, need_r = s.need
    xd, wd = dev(t["x"], need_x), dev(t["w"], need_w)
    sfd, rsd = dev(t["shift"], need_s), dev(t["res"], need_r)
    xin = xd
    if s.pro:
        xin = ops.NormedInput(xd, dev(t["in_stats"]), ACT_LRELU, ops.LRELU_SLOPE)
        if materialised:      # the project's own stand-alone apply pass; its backward hands the gradient through to xd
            xin = xin.materialize()
    spec = _spec(s)
    slot = ops.StatsSlot(s.n) if s.stats else None
    with record() as rec, (contextlib.nullcontext() if any(s.need) else torch.no_grad()):
        if s.oidhw:
            y = ops.conv3d_w(xin, wd, spec, scale=dev(t["scale"]), shift=sfd, res=rsd, stats=slot,
                             shift_scaled=bool(s.shift_scaled))
        else:
            y = ops.conv3d(xin, ops.pack_weight(wd), spec, scale=dev(t["scale"]), shift=sfd, res=rsd, stats=slot)
        if any(s.need):
            y.backward(dev(t["gy"]))

    def host(v):
        return None if v is None else v.detach().cpu()
    got = dict(y=host(y), dx=host(xd.grad), dw=host(wd.grad), dshift=host(None if sfd is None else sfd.grad),
               dres=host(None if rsd is None else rsd.grad), stats=host(None if slot is None else slot.get(s.n, y.shape[-1])),
               recorded=rec.calls)
    return got


def kernel_info(s):
    """What the dispatcher does with this conv: the forward kernel family, the operand kinds of the forward and the data
    gradient, the three workspace sizes."""
    lib = _lib.load()
    p = ops._params(_spec(s), (s.n,) + s.dhw + (s.ci,), bool(s.scale_mode), bool(s.has_shift), bool(s.res_mode))
    kinds, nbytes = (C.c_int32 * 2)(), (C.c_size_t * 2)()
    rc = lib.cfun_weight_prepare_kinds(C.byref(p), kinds, nbytes)
    return dict(fwd=KERNEL_NAMES.get(int(lib.cfun_conv3d_fwd_kernel(C.byref(p))), "?"),
                kinds=tuple(WOP_NAMES.get(int(k), "?") for k in kinds) if rc == 0 else ("?", "?"),
                ws=(int(lib.cfun_conv3d_fwd_workspace_bytes(C.byref(p))), int(lib.cfun_conv3d_bwd_data_workspace_bytes(C.byref(p))),
                    int(lib.cfun_conv3d_bwd_weight_workspace_bytes(C.byref(p)))))


BWD_NAMES = {0: "direct", 1: "mfma", 2: "wino", 3: "s2fold", 4: "c1"}


def bwd_kernels(s):
    """(data-gradient family, weight-gradient family) of this conv (cfun_conv3d_bwd_kernels), and whether the weight-gradient
    tile query answers (it refuses exactly the C_in = 1 and direct weight gradients)."""
    lib = _lib.load()
    p = ops._params(_spec(s), (s.n,) + s.dhw + (s.ci,), bool(s.scale_mode), bool(s.has_shift), bool(s.res_mode))
    out, tile = (C.c_int32 * 2)(), (C.c_int32 * 3)()
    _lib.check(lib.cfun_conv3d_bwd_kernels(C.byref(p), out), "conv3d_bwd_kernels")
    return dict(dgrad=BWD_NAMES.get(int(out[0]), "?"), wgrad=BWD_NAMES.get(int(out[1]), "?"),
                wgrad_tile=int(lib.cfun_conv3d_wgrad_tile(C.byref(p), tile)) == 0)


def replay(s, device, algo=None):
    """Run signature s on ``device`` and compare with fp64 under the rule.  Returns a report dict (``rows``: quantity ->
    (e_kernel, e32), ``failures``: list of messages, ``info``, ``ref_seconds``); the caller asserts ``failures`` is empty
    after printing ``format_row``.  ``algo`` overrides the recorded CFUN_ALGO_* (the emulator tier records under the direct
    kernels and replays under the dispatcher's own choice)."""
    if algo is not None:
        s = s._replace(algo=algo)
    t = make_tensors(s, device)
    got = run_kernels(s, t, device)
    failures = []
    if got["recorded"] != [s]:
        failures.append("the replayed call recorded %s, not %s" % ([sig_id(r) for r in got["recorded"]], sig_id(s)))
    t0 = time.time()
    seed = zlib.crc32(sig_id(s).encode()) & 0x7FFFFFFF
    yboxes = boxes_for(out_dims(s), s.n, np.random.RandomState(seed))
    xboxes = boxes_for(s.dhw, s.n, np.random.RandomState(seed ^ 1))
    rows_sel = live_rows(s)
    errs = {}
    ops64 = {dt: {k: (None if t[k] is None else t[k].to(dt)) for k in ("w", "scale", "shift", "res")}
             for dt in (torch.float64, torch.float32)}
    xin = {dt: apply_prologue(s, t["x"].to(dt), t["in_stats"]) for dt in (torch.float64, torch.float32)}
    # y on the boxes
    ek, e32 = _Err(), _Err()
    for box in yboxes:
        o = ops64[torch.float64]
        ref = ref_y_box(s, box, xin[torch.float64], o["w"], o["scale"], o["shift"], o["res"])
        o = ops64[torch.float32]
        ek.add(cut_y(s, got["y"], box), ref)
        e32.add(ref_y_box(s, box, xin[torch.float32], o["w"], o["scale"], o["shift"], o["res"]), ref)
    errs["y"] = (ek.value, e32.value)
    # the statistics epilogue: the reduction of the kernel's own y
    if s.stats:
        if got["stats"] is None:
            failures.append("the step got epilogue statistics from this conv, the replay did not")
        else:
            y64 = got["y"].double().reshape(s.n, -1, got["y"].shape[-1])
            mean = y64.mean(dim=1)
            rstd = 1.0 / torch.sqrt(y64.var(dim=1, unbiased=False) + 1e-5)
            for nm, a, b in (("mean", got["stats"][..., 0], mean), ("rstd", got["stats"][..., 1], rstd)):
                e = kc.rel_err(a, b)
                errs["stats." + nm] = (e, None)
                if not e < STATS_TOL:
                    failures.append("epilogue %s: rel err %.3e >= %.1e" % (nm, e, STATS_TOL))
    if any(s.need):
        grads = {}
        for dt in (torch.float64, torch.float32):
            gp, g = conv_sum_gradients(s, t["gy"], got["y"], t["scale"], dt)
            w = ops64[dt]["w"] if rows_sel is None else ops64[dt]["w"].index_select(0, rows_sel)
            r = {}
            if s.need[0]:
                r["dx"] = [ref_dx_box(s, box, w, g) for box in xboxes]
            if s.need[1]:
                r["dw"] = ref_dw_full(s, xin[dt], g, dt)
            if s.need[2]:
                src = g if (s.shift_scaled and s.scale_mode) else gp      # (ops.fold_bias(..., pre=True): db = sum(g))
                r["dshift"] = src.reshape(-1, src.shape[-1]).sum(0)
            if s.need[3]:
                r["dres"] = ref_dres(s, gp)
            grads[dt] = r
            del gp, g
        r64, r32 = grads[torch.float64], grads[torch.float32]
        if s.need[0]:
            ek, e32 = _Err(), _Err()
            for box, a, b in zip(xboxes, r64["dx"], r32["dx"]):
                sample, (z, y_, x_) = box[0], box[1:]
                ek.add(got["dx"][sample:sample + 1, z[0]:z[1], y_[0]:y_[1], x_[0]:x_[1]], a)
                e32.add(b, a)
            errs["dx"] = (ek.value, e32.value)
        if s.need[1]:
            dwk = got["dw"] if rows_sel is None else got["dw"].index_select(0, rows_sel)
            if rows_sel is not None:      # the padding rows of each parity group produce no channel of y: no gradient
                pad_rows = torch.ones(s.co, dtype=torch.bool)
                pad_rows[rows_sel] = False
                if float(got["dw"][pad_rows].abs().max()) != 0.0:
                    failures.append("dw: the padded parity rows carry a gradient")
            a, b = r64["dw"], r32["dw"]
            if s.tap_skip:
                # the folded weight is zero at the dead taps and ops.fold_up2_weight's backward reads the live ones only.
                # A kernel that skips the dead taps writes zeros there (the MFMA wgrad does); one that does not skip (the
                # direct kernels the dispatcher falls back to) delivers the dense gradient, which the reference holds as
                # well.  Nothing else may stand there: all zero -> compare the live taps, otherwise the whole tensor.
                m = live_tap_mask(s, a.shape[0])
                if float((dwk * ~m).abs().max()) == 0.0:
                    a, b = a * m, b * m
            errs["dw"] = (kc.rel_err(dwk, a), kc.rel_err(b, a))
        if s.need[2]:
            errs["dshift"] = (kc.rel_err(got["dshift"], r64["dshift"]), kc.rel_err(r32["dshift"], r64["dshift"]))
        if s.need[3]:
            errs["dres"] = (kc.rel_err(got["dres"], r64["dres"]), kc.rel_err(r32["dres"], r64["dres"]))
    ref_seconds = time.time() - t0
    for q, (e, e3) in errs.items():
        if e3 is not None and not e <= bound(e3):
            failures.append("%s: rel err vs fp64 %.3e > %.1f x %.3e (the fp32 formulation's) + %.0e"
                            % (q, e, bench.GRAD_FP64_FACTOR, e3, bench.GRAD_FP64_FLOOR))
    # the prologue repeats the stand-alone passes' arithmetic: bit for bit the same kernels fed the materialised input
    if s.pro:
        mat = run_kernels(s, t, device, materialised=True)
        if mat["recorded"] != [s._replace(pro=PRO_NONE)]:
            failures.append("prologue: the materialised-input run recorded %s" % [sig_id(r) for r in mat["recorded"]])
        for q in ("y", "dx", "dw", "dshift", "dres", "stats"):
            if (got[q] is None) != (mat[q] is None):
                failures.append("prologue: %s is delivered by only one of the prologue / materialised-input runs" % q)
            elif got[q] is not None and not torch.equal(got[q], mat[q]):
                failures.append("prologue: %s differs from the materialised-input run (max abs %.3e)"
                                % (q, float((got[q] - mat[q]).abs().max())))
    return dict(sig=s, rows=errs, failures=failures, info=kernel_info(s), ref_seconds=ref_seconds)


def format_row(rep):
    i = rep["info"]
    head = "%-78s fwd=%-9s ops=%s/%s ws=%d/%d/%d ref=%.1fs" % ((sig_id(rep["sig"]), i["fwd"]) + i["kinds"] + i["ws"]
                                                               + (rep["ref_seconds"],))
    cells = []
    for q, (e, e3) in rep["rows"].items():
        if e3 is None:
            cells.append("%s %.2e" % (q, e))
        else:
            cells.append("%s %.2e/%.2e=%.2f (%.2f of bound)" % (q, e, e3, _ratio(e, e3), e / bound(e3)))
    return head + " | " + " | ".join(cells)


def worst_of_bound(rep):
    return max([e / bound(e3) for e, e3 in rep["rows"].values() if e3 is not None] or [0.0])


# ------------------------------------------------------------------------------------------ the product's configurations
def product_configs():
    """name -> (configuration factory, positive RoIs kept of the synthetic inputs or None for all)."""
    from cfun_amd import config
    return {"cfg0": (lambda: config.heart_config("beginning", 64, 64, 32), 2),    # test_training_step_cfg0_vs_oracle's step
            "cfg2": (lambda: config.heart_config("finetune", 256, 256, 128), None),      # the benchmarked step
            "cfg3": (lambda: config.heart_config("finetune", 512, 512, 256), None),
            "lits_beginning": (lambda: config.LiTSConfig("beginning"), None),
            "lits_together": (lambda: config.LiTSConfig("together"), None)}


class _Fold(ast.NodeTransformer):
    """``B`` and ``<int> * B`` -> their integer values, so that ast.literal_eval (data only) reads the table."""

    def __init__(self, env):
        self.env = env

    def visit_Name(self, node):
        return ast.copy_location(ast.Constant(self.env[node.id]), node)

    def visit_BinOp(self, node):
        node = self.generic_visit(node)
        if isinstance(node.op, ast.Mult) and all(isinstance(v, ast.Constant) and isinstance(v.value, int)
                                                 for v in (node.left, node.right)):
            return ast.copy_location(ast.Constant(node.left.value * node.right.value), node)
        return node


def bench_layers_plain():
    """The plain-conv (mode "") entries of tools/bench_layers.LAYERS, read without importing the script."""
    with open(os.path.join(ROOT, "tools", "bench_layers.py")) as f:
        tree = ast.parse(f.read())
    env = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name):
            name = node.targets[0].id
            if name == "B":
                env["B"] = ast.literal_eval(node.value)
            elif name == "LAYERS":
                layers = ast.literal_eval(_Fold(env).visit(node.value))
                return [L for L in layers if L[7] == ""]
    raise RuntimeError("tools/bench_layers.py: no LAYERS table")


def layer_matches(layer, s):
    name, n, dhw, ci, co, k, stride, mode = layer
    return (s.n == n and s.dhw == tuple(dhw) and s.ci == ci and s.co == co and s.k == (k, k, k) and s.stride == stride
            and not s.up2 and not s.d2s)


def write_manifest(device="cuda:0", path=MANIFEST):
    out = {}
    for name, (make, n_pos) in product_configs().items():
        rec, _ = record_step(make(), device, n_pos=n_pos)
        out[name] = [sig_to_json(s) for s in sorted(set(rec.calls), key=sig_id)]
        print("%s: %d conv calls, %d distinct signatures" % (name, len(rec.calls), len(out[name])))
        torch.cuda.empty_cache()
    with open(path, "w") as f:          # one signature per line
        f.write("{\n" + ",\n".join('"%s": [\n%s\n]' % (name, ",\n".join(json.dumps(d, sort_keys=True) for d in sigs))
                                  for name, sigs in sorted(out.items())) + "\n}\n")


if __name__ == "__main__":
    if "--write-manifest" in sys.argv:          # on an MI355X; an optional path follows the flag
        rest = sys.argv[sys.argv.index("--write-manifest") + 1:]
        write_manifest(path=rest[0] if rest else MANIFEST)
    else:
        print(__doc__)
