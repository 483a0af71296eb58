"""Head tier: the detection head and the inference tail (csrc/fc.hip, csrc/roi_nms.hip, csrc/resize.hip) against float64 at
the launch-geometry and value edges their golden cases and fuzz sweeps do not reach.  Shared by the CPU tier (HIP emulator,
tests/test_head_emu.py) and the GPU tier (tests/test_head_gpu.py).

The rule is the memory-bound tier's (``membound_cases.hold``): three evaluations of the same fp32 inputs -- the float64
reference, the torch-CPU fp32 evaluation of that reference (e32 = its error), the kernel (ek) -- and

    ek <= bench.GRAD_FP64_FACTOR * e32 + bench.GRAD_FP64_FLOOR              (product_shapes.bound)

whole-tensor and per segment (a row of y, a 256-column K chunk of dx / dW, one grid sweep of a grid-stride kernel).  Trilinear
resampling is continuous in the source coordinate, so a float64 reference that takes another floor index within an ulp of an
integer is still a reference.  Where a kernel promises more than the rule -- integer crop bounds, keep lists, nearest-neighbour
copies, label volumes, run-to-run identical sums -- the promise is asserted bit for bit.  No tolerance constant is defined here.

Groups: A classifier GEMMs, B RoIAlign, C NMS, D mask targets and the inference tail.  Every input is seeded here; nothing is
read from disk."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import torch
import torch.nn.functional as F

from membound_cases import REPORT, _canary_intact, _dev_slice, bits_equal, hold, hold_fp64_sum, report_lines  # noqa: F401
from product_shapes import bound          # noqa: F401  (the rule's right-hand side: imported, never copied)
from cfun_amd import _lib, ops
from cfun_amd._lib import ACT_LRELU, ACT_NONE, ACT_RELU
from kernel_cases import _gen, py_bounds, randn
from oracle import cfun_oracle as orc

CFUN_OK, CFUN_EINVAL, CFUN_EWORKSPACE = 0, -1, -2           # include/cfun_hip.h

# ---- launch constants, next to the source lines they come from; check_launch_constants() reads each line from the shipped
# source and compares.  A change of the source then fails an assertion instead of moving a case silently off its edge.
K_KC = 256                           # fc.hip: constexpr int kKC = 256;        K chunk of k_fc_fwd / k_fc_bwd_weight
K_RT = 16                            # fc.hip: constexpr int kRT = 16;         RoIs per register tile (k_fc_bwd_data, NR tiles)
FC_U = 16                            # fc.hip: constexpr int U = 16;           weight rows in flight in k_fc_bwd_data
FC_FINISH_GROUPS = 64                # fc.hip: k_fc_finish: row += 64 / red[64][17]
FC_BWD_DATA_K = 128 * 4              # fc.hip: k_fc_bwd_data: 128 lanes x 4 consecutive k per block
FC_MAX_ROWS = 64                     # fc.hip: R > 64 -> CFUN_EINVAL
ROI_FWD_CAP = 256 * 16               # roi_nms.hip: cfun_roi_align3d_slab_fwd grid cap (blocks)
ROI_BWD_CAP = 256 * 32               # roi_nms.hip: cfun_roi_align3d_slab_bwd
UNMOLD_CAP = 256 * 32                # roi_nms.hip: cfun_unmold_argmax / cfun_unmold_overlap
MASK_TARGET_CAP = 256 * 16           # roi_nms.hip: cfun_mask_target_labels
RESIZE_CAP = 256 * 64                # resize.hip: cfun_resize3d
ROI_FWD_SWEEP, ROI_BWD_SWEEP = ROI_FWD_CAP * 256, ROI_BWD_CAP * 256          # elements one grid sweep covers
UNMOLD_SWEEP, MASK_TARGET_SWEEP, RESIZE_SWEEP = UNMOLD_CAP * 256, MASK_TARGET_CAP * 256, RESIZE_CAP * 256
ROI_BOUNDS_BLOCK = 64                # roi_nms.hip: k_roi_bounds: dim3((R + 63) / 64), dim3(64)
MAX_OVERLAP_BOXES = 64               # roi_nms.hip: constexpr int kMaxOverlapBoxes = 64;
NMS_CH = 16                          # roi_nms.hip: k_nms_scan: constexpr int CH = 16;
NMS_MAX_N = 4096                     # roi_nms.hip: if (n < 0 || n > 4096) return CFUN_EINVAL;


def _src(name):
    return open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", name)).read()


def check_launch_constants(device):
    fc, roi, rs = _src("fc.hip"), _src("roi_nms.hip"), _src("resize.hip")

    def one(src, pattern):
        found = re.findall(pattern, src, re.S)
        assert len(found) >= 1 and len(set(found)) == 1, "%r matches %s" % (pattern, found)
        return found[0]

    def body(src, head):          # the text of one function, from its head to the first closing brace in column 0
        m = re.search(re.escape(head) + r".*?\n\}", src, re.S)
        assert m, head
        return m.group(0)

    def cap(src, head):
        c = re.findall(r"if \(blocks > (\d+) \* (\d+)\) blocks = (\d+) \* (\d+);", body(src, head))
        assert len(c) == 1 and c[0][:2] == c[0][2:], (head, c)
        return int(c[0][0]) * int(c[0][1])

    assert int(one(fc, r"constexpr int kKC = (\d+);")) == K_KC
    assert int(one(fc, r"constexpr int kRT = (\d+);")) == K_RT
    assert int(one(fc, r"constexpr int U = (\d+);")) == FC_U
    fin = body(fc, "k_fc_finish(const float*")
    assert int(one(fin, r"row < nchunks; row \+= (\d+)\)")) == FC_FINISH_GROUPS
    assert int(one(fin, r"__shared__ float red\[(\d+)\]\[17\];")) == FC_FINISH_GROUPS
    assert int(one(fin, r"for \(int i = 0; i < (\d+); \+\+i\) v \+= red\[i\]\[c\];")) == FC_FINISH_GROUPS
    assert int(one(fc, r"const int64_t k = \(\(int64_t\)blockIdx\.x \* (\d+) \+ tid\) \* 4;")) * 4 == FC_BWD_DATA_K
    assert set(re.findall(r"\(K & 3\) \|\| R > (\d+)\) return CFUN_EINVAL;", fc)) == {str(FC_MAX_ROWS)}
    assert cap(roi, "int cfun_roi_align3d_slab_fwd(") == ROI_FWD_CAP
    assert cap(roi, "int cfun_roi_align3d_slab_bwd(") == ROI_BWD_CAP
    assert cap(roi, "int cfun_unmold_argmax(") == UNMOLD_CAP
    assert cap(roi, "int cfun_unmold_overlap(") == UNMOLD_CAP
    assert cap(roi, "int cfun_mask_target_labels(") == MASK_TARGET_CAP
    assert cap(rs, 'extern "C" int cfun_resize3d(') == RESIZE_CAP
    # every capped launch strides by the whole grid, 256 threads a block
    assert len(re.findall(r"i \+= \(int64_t\)gridDim\.x \* 256\)", roi)) == 5
    assert len(re.findall(r"i \+= \(int64_t\)gridDim\.x \* 256\)", rs)) == 1
    assert one(roi, r"k_roi_bounds, dim3\(\(R \+ (\d+)\) / (\d+)\), dim3\((\d+)\)") == ("63", "64", str(ROI_BOUNDS_BLOCK))
    assert int(one(roi, r"constexpr int kMaxOverlapBoxes = (\d+);")) == MAX_OVERLAP_BOXES
    assert int(one(roi, r"constexpr int CH = (\d+);")) == NMS_CH
    assert int(one(roi, r"if \(n < 0 \|\| n > (\d+)\) return CFUN_EINVAL;")) == NMS_MAX_N
    # what the library lets one observe: the chunk count through the workspace, the row limit through a refusal
    lib = _lib.load()
    for k in (4, K_KC, K_KC + 4, 65 * K_KC):
        assert int(lib.cfun_fc_workspace_bytes(3, k, 8)) == -(-k // K_KC) * 3 * 8 * 4, k
    assert int(lib.cfun_fc_bwd_weight_max_rows(16)) == FC_MAX_ROWS


# ========================================================================================== A. classifier GEMMs
FC_K_EDGES = (4, 252, 256, 260, 508, 512, 516, 1028)                     # at R = 5, O = 12
FC_CHUNK_EDGES = tuple((c - 1) * K_KC + 4 for c in (63, 64, 65, 129))    # at R = 3, O = 8: a ragged 4-wide last chunk
FC_R_EDGES = (1, 15, 16, 17, 32, 33, 48, 49, 64)                         # at K = 516, O = 20
FC_O_EDGES = (1, 2, 3, 4, 13, 15, 16, 17, 19, 31, 32, 33)                # at R = 17, K = 516
assert FC_CHUNK_EDGES[2] == 16388 and all(k % 4 == 0 for k in FC_K_EDGES + FC_CHUNK_EDGES)
FC_EPILOGUES = ("full", "scale", "none")


def _fc_inputs(r, k, o, epi, seed):
    gen = _gen(seed)
    x, w, gy = randn(gen, r, k), randn(gen, o, k) * (k ** -0.5), randn(gen, r, o)
    scale = shift = None
    act = ACT_NONE
    if epi in ("full", "scale"):
        scale = randn(gen, o) + 0.25                # both signs ...
        scale[scale == 0] = 0.25
        dead = 1 + (r + o) % 4                      # ... and exact zeros (a dead folded-BN channel) at dead, dead + 5, ...:
        scale[dead::5] = 0.0                        # never column 0, so O = 1 ... 4 keep a live column and every O a live row 0
        neg = 0 if dead == 1 or o == 1 else 1
        scale[neg] = -abs(scale[neg]) - 0.5
        assert bool((scale != 0).any()) and bool((scale < 0).any()) and (o <= dead or bool((scale == 0).any()))
    if epi == "full":
        shift, act = randn(gen, o) * 0.5, ACT_RELU
    return x, w, scale, shift, act, gy


def _fc_y(x, w, scale, shift, act, dt):
    y = F.linear(x.to(dt), w.to(dt))
    if scale is not None:
        y = y * scale.to(dt)
    if shift is not None:
        y = y + shift.to(dt)
    return F.relu(y) if act == ACT_RELU else y


def _by_chunk(t):
    """[rows, K] -> [chunks, rows * 256] (K padded with zeros): flat segments of rows * 256 are then the K chunks."""
    rows, k = t.shape
    pad = (-k) % K_KC
    t = F.pad(t.detach().cpu(), (0, pad))
    return t.reshape(rows, -1, K_KC).permute(1, 0, 2).contiguous()


def _hold_chunks(case, what, got, r64, r32):
    hold(case, what, _by_chunk(got), _by_chunk(r64), _by_chunk(r32), seg=got.shape[0] * K_KC)


def check_fc_abi(device, r, k, o, epi="full", seed=301):
    """cfun_fc_fwd / _bwd_data / _bwd_weight at the C ABI.  y per row, dx and dW per 256-column K chunk; every kernel twice,
    bit-identical.  The gradient fed to the backward kernels is dy * relu'(y) * scale at the KERNEL's own y (as the product-shape
    tier does), so a pre-activation within rounding of zero cannot put the kink into the comparison."""
    lib = _lib.load()
    case = "fc abi R=%d K=%d O=%d %s" % (r, k, o, epi)
    x, w, scale, shift, act, gy = _fc_inputs(r, k, o, epi, seed + r + 7 * k + 13 * o)
    xd, wd = x.to(device), w.to(device)
    sd, hd = (None if t is None else t.to(device) for t in (scale, shift))
    st = ops.stream(xd)
    nb = int(lib.cfun_fc_workspace_bytes(r, k, o))
    assert nb == -(-k // K_KC) * r * o * 4
    ys = []
    for _ in range(2):
        ws = torch.full((nb,), 0xA5, dtype=torch.uint8, device=device)
        y = torch.full((r, o), float("nan"), device=device)
        assert lib.cfun_fc_fwd(ops.ptr(xd), ops.ptr(wd), ops.ptr(sd), ops.ptr(hd), ops.ptr(y), r, k, o, act, ops.ptr(ws), nb, st) == CFUN_OK
        ys.append(y)
    assert bits_equal(ys[0], ys[1]), case + ": two forward runs differ"
    y = ys[0].cpu()
    hold(case, "y", y, _fc_y(x, w, scale, shift, act, torch.float64), _fc_y(x, w, scale, shift, act, torch.float32), seg=o)
    g = gy.clone()
    if act == ACT_RELU:
        g = torch.where(y > 0, g, torch.zeros(()))
    if scale is not None:
        g = g * scale
    assert bool((g != 0).any()), case + ": the gradient fed to the backward kernels is all zeros -- the case could not fail"
    gd = g.to(device)
    dxs = []
    for _ in range(2):
        dx = torch.full((r, k), float("nan"), device=device)
        assert lib.cfun_fc_bwd_data(ops.ptr(gd), ops.ptr(wd), ops.ptr(dx), r, k, o, st) == CFUN_OK
        dxs.append(dx)
    assert bits_equal(dxs[0], dxs[1]), case + ": two data-gradient runs differ"
    _hold_chunks(case, "dx", dxs[0], g.double() @ w.double(), g @ w)
    # every shape this function is given (R <= 64, O <= 33) is meant to fit the weight-gradient kernel's LDS in one call
    assert r <= int(lib.cfun_fc_bwd_weight_max_rows(o)), case + ": dW would need row chunks (that is check_fc_ops' case)"
    dws = []
    for _ in range(2):
        dw = torch.full((o, k), float("nan"), device=device)
        assert lib.cfun_fc_bwd_weight(ops.ptr(xd), ops.ptr(gd), ops.ptr(dw), r, k, o, st) == CFUN_OK
        dws.append(dw)
    assert bits_equal(dws[0], dws[1]), case + ": two weight-gradient runs differ"
    _hold_chunks(case, "dW", dws[0], g.double().t() @ x.double(), g.t() @ x)


def check_fc_ops(device, r, k, o, epi="full", seed=331):
    """ops.fc with autograd: y, dx, dW (in row chunks when R exceeds cfun_fc_bwd_weight_max_rows) and dshift."""
    case = "ops.fc R=%d K=%d O=%d %s" % (r, k, o, epi)
    x, w, scale, shift, act, gy = _fc_inputs(r, k, o, epi, seed + r + 7 * k + 13 * o)
    xd, wd = (t.clone().to(device).requires_grad_(True) for t in (x, w))
    sd = None if scale is None else scale.to(device)
    hd = None if shift is None else shift.clone().to(device).requires_grad_(True)
    y = ops.fc(xd, wd, sd, hd, act)
    y.backward(gy.to(device))
    yk = y.detach().cpu()
    hold(case, "y", yk, _fc_y(x, w, scale, shift, act, torch.float64), _fc_y(x, w, scale, shift, act, torch.float32), seg=o)

    def grads(dt):
        gp = gy.to(dt)
        if act == ACT_RELU:
            gp = torch.where(yk > 0, gp, torch.zeros((), dtype=dt))
        g = gp if scale is None else gp * scale.to(dt)
        return g @ w.to(dt), g.t() @ x.to(dt), gp.sum(0)

    r64, r32 = grads(torch.float64), grads(torch.float32)
    assert all(bool((t != 0).any()) for t in r64), case + ": a reference gradient is all zeros -- the case could not fail"
    _hold_chunks(case, "dx", xd.grad, r64[0], r32[0])
    _hold_chunks(case, "dW", wd.grad, r64[1], r32[1])
    if hd is not None:
        hold(case, "dshift", hd.grad, r64[2], r32[2])


def fc_row_chunk_cases(device):
    """(R, K, O) of the dW row-chunking cases: for a wide O, R = the rows the kernel's LDS holds and one more (a one-row
    remainder chunk); and the O = 1024, R = 64 case of kernel_cases.check_fc."""
    lib = _lib.load()
    o = 1024
    rmax = int(lib.cfun_fc_bwd_weight_max_rows(o))
    assert 1 <= rmax < FC_MAX_ROWS, "O = %d must not fit %d rows, or nothing is chunked" % (o, FC_MAX_ROWS)
    return ((rmax, 260, o), (rmax + 1, 260, o), (64, 128, o))


def check_fc_zero_rows(device):
    """R = 0: cfun_fc_bwd_weight writes zeros (the gradient of an empty batch), nothing outside."""
    lib = _lib.load()
    o, k = 5, 260
    buf, dw = _dev_slice(torch.full((o * k,), float("nan")), device, 4)
    assert lib.cfun_fc_bwd_weight(None, None, ops.ptr(dw), 0, k, o, ops.stream(dw)) == CFUN_OK
    assert bool((dw == 0).all()) and _canary_intact(buf, 4, o * k)
    z = ops.fc(torch.zeros(0, k, device=device), torch.ones(o, k, device=device))
    assert tuple(z.shape) == (0, o)


def check_fc_refusals(device):
    """Every refused call returns CFUN_EINVAL and leaves its outputs and the canaries either side of them alone."""
    lib = _lib.load()
    r, k, o = 3, 260, 8
    gen = _gen(340)
    n_in = FC_MAX_ROWS * 2 * k
    _, x = _dev_slice(randn(gen, n_in), device, 0)
    _, w = _dev_slice(randn(gen, n_in), device, 0)
    _, g = _dev_slice(randn(gen, n_in), device, 0)
    _, x1 = _dev_slice(randn(gen, n_in), device, 1)        # 4 bytes past a 16-byte boundary
    _, w1 = _dev_slice(randn(gen, n_in), device, 1)
    nb = int(lib.cfun_fc_workspace_bytes(FC_MAX_ROWS, k, o))
    ws = torch.zeros(nb + 16, dtype=torch.uint8, device=device)
    st = ops.stream(x)
    n_out = (FC_MAX_ROWS + 1) * max(k, o)
    outs = [_dev_slice(torch.full((n_out,), 555.0), device, 4) for _ in range(3)]
    (_, y), (_, dw), (_, dx) = outs
    p = ops.ptr

    def fwd(xx=x, ww=w, rr=r, kk=k, act=ACT_RELU, wsp=None, nbytes=nb):
        return lib.cfun_fc_fwd(p(xx), p(ww), None, None, p(y), rr, kk, o, act, p(ws) if wsp is None else wsp, nbytes, st)

    assert fwd() == CFUN_OK                                 # the accepted call the refusals are one step away from
    y.fill_(555.0)
    calls = {
        "fwd K=258": lambda: fwd(kk=258),
        "bwd_weight K=258": lambda: lib.cfun_fc_bwd_weight(p(x), p(g), p(dw), r, 258, o, st),
        "bwd_data K=258": lambda: lib.cfun_fc_bwd_data(p(g), p(w), p(dx), r, 258, o, st),
        "fwd R=65": lambda: fwd(rr=FC_MAX_ROWS + 1),
        "bwd_weight R=65": lambda: lib.cfun_fc_bwd_weight(p(x), p(g), p(dw), FC_MAX_ROWS + 1, k, o, st),
        "bwd_data R=65": lambda: lib.cfun_fc_bwd_data(p(g), p(w), p(dx), FC_MAX_ROWS + 1, k, o, st),
        "fwd x + 4 bytes": lambda: fwd(xx=x1),
        "bwd_weight x + 4 bytes": lambda: lib.cfun_fc_bwd_weight(p(x1), p(g), p(dw), r, k, o, st),
        "fwd w + 4 bytes": lambda: fwd(ww=w1),
        "bwd_data w + 4 bytes": lambda: lib.cfun_fc_bwd_data(p(g), p(w1), p(dx), r, k, o, st),
        "fwd ws + 4 bytes": lambda: fwd(wsp=ws.data_ptr() + 4),
        "fwd ws one byte short": lambda: fwd(nbytes=int(lib.cfun_fc_workspace_bytes(r, k, o)) - 1),
        "fwd act=LRELU": lambda: fwd(act=ACT_LRELU),
    }
    for name, call in calls.items():
        assert call() == CFUN_EINVAL, name
        for buf, view in outs:
            assert bool((view == 555.0).all()), name + ": an output was written"
            assert _canary_intact(buf, 4, n_out), name + ": a canary was written"


# ========================================================================================== B. RoIAlign
def _roi_refs(fm, boxes, pool, gy):
    """(out64, g64, out32, g32) in the kernel's layouts ([R,pd,ph,pw,C], [D,H,W,C]): the oracle's crop + F.interpolate(
    align_corners=True) on the float64 and on the fp32 map, and their autograd gradients."""
    res = []
    for dt in (torch.float64, torch.float32):
        f = fm.permute(3, 0, 1, 2).to(dt).clone().requires_grad_(True)
        out = orc.roi_align(f, pool, boxes)
        grad = None
        if gy is not None:
            grad = torch.zeros_like(f)
            if out.requires_grad:
                grad = torch.autograd.grad((out * gy.permute(0, 4, 1, 2, 3).to(dt)).sum(), f)[0]
            grad = grad.permute(1, 2, 3, 0).contiguous()
        res += [out.detach().permute(0, 2, 3, 4, 1).contiguous(), grad]
    return res


def _roi_run(device, fm, boxes, pool, gy=None, slab=None):
    fd = fm.clone().to(device).requires_grad_(True)
    out, bounds = ops.roi_align(fd, boxes.to(device), pool, slab=slab)
    if gy is not None:
        out.backward(gy.to(device))
    return out.detach(), bounds, fd.grad


def _check_roi(case, device, fm, boxes, pool, seed, fwd_seg=None, bwd_seg=None, twice=False):
    gen = _gen(seed)
    gy = randn(gen, boxes.shape[0], *pool, fm.shape[-1])
    out, bounds, grad = _roi_run(device, fm, boxes, pool, gy)
    want = py_bounds(boxes, fm.shape[:3])
    np.testing.assert_array_equal(bounds.cpu().numpy()[:boxes.shape[0]], want)               # bit-exact crop bounds
    o64, g64, o32, g32 = _roi_refs(fm, boxes, pool, gy)
    hold(case, "out", out, o64, o32, seg=fwd_seg)
    hold(case, "dfm", grad, g64, g32, seg=bwd_seg)
    if twice:
        out2, _, grad2 = _roi_run(device, fm, boxes, pool, gy)
        assert bits_equal(out, out2) and bits_equal(grad, grad2), case + ": two runs differ"
    return want, g64


ROI_FWD_SWEEPS = dict(dhw=(11, 13, 12), c=51, pool=(24, 24, 24), r=3)
# (pool 3 x 4 x 3: with 2 or 3 samples an axis every weight is 0, 1/2 or 1 and the gradient exact in any precision; 4 samples over
# the boxes' 5 ... 65 source voxels give weights that round)
ROI_BWD_SWEEPS = dict(dhw=(17, 63, 65), c=61, pool=(3, 4, 3))


def check_roi_fwd_sweeps(device, seed=401):
    """The forward over two sweeps of its 4096-block grid and a ragged third (R = 3, pool 24^3, C = 51)."""
    cfg = ROI_FWD_SWEEPS
    total = cfg["r"] * 24 ** 3 * cfg["c"]
    assert 2 * ROI_FWD_SWEEP < total < 3 * ROI_FWD_SWEEP
    gen = _gen(seed)
    fm = randn(gen, *cfg["dhw"], cfg["c"])
    boxes = torch.tensor([[0.0, 0.0, 0.0, 1.0, 1.0, 1.0], [0.1, 0.3, 0.2, 0.7, 0.9, 0.85], [0.5, 0.0, 0.4, 0.95, 0.6, 1.0]])
    _check_roi("roi fwd sweeps", device, fm, boxes, cfg["pool"], seed, fwd_seg=ROI_FWD_SWEEP)


def check_roi_bwd_sweeps(device, seed=402):
    """The backward gather over two sweeps of its 8192-block grid and a ragged third: a (17, 63, 65, 61) map, three boxes, a
    small pool (short gather loops), every sweep holding non-zero gradient; segmented by sweep."""
    cfg = ROI_BWD_SWEEPS
    d, h, w = cfg["dhw"]
    c = cfg["c"]
    total = d * h * w * c
    assert 2 * ROI_BWD_SWEEP < total < 3 * ROI_BWD_SWEEP
    # element 2 * ROI_BWD_SWEEP sits in plane 16 at row y = 49: the third box has to reach below it
    assert (2 * ROI_BWD_SWEEP) // (h * w * c) == d - 1 and ((2 * ROI_BWD_SWEEP) % (h * w * c)) // (w * c) == 49
    gen = _gen(seed)
    fm = randn(gen, d, h, w, c)
    boxes = torch.tensor([[0.0, 0.1, 0.1, 5.0 / d, 0.6, 0.5], [9.0 / d, 0.3, 0.4, 14.0 / d, 0.9, 1.0],
                          [15.0 / d, 40.0 / h, 0.0, 1.0, 1.0, 1.0]])
    _, g64 = _check_roi("roi bwd sweeps", device, fm, boxes, cfg["pool"], seed, bwd_seg=ROI_BWD_SWEEP)
    assert REPORT[-2][3] > 0, "the fp32 reference is exact: the weights of this case do not round"
    flat = g64.reshape(-1)
    for s in range(3):
        assert bool((flat[s * ROI_BWD_SWEEP:(s + 1) * ROI_BWD_SWEEP] != 0).any()), "sweep %d holds no gradient" % s


ROI_EDGE_S = 64              # a power of two: k / S and its fp32 product with S are exact, the crop extents are what is asked


def roi_extents(p):
    """Crop extents against pool p: {1, 2, 3, p-1, p, p+1, 2p-1, 2p, 3p+1}; (n-1)/(p-1) is not representable for most pairs
    (n = 8, p = 4: 7/3), so the last sample's source index lands within an ulp of n - 1."""
    return sorted({n for n in (1, 2, 3, p - 1, p, p + 1, 2 * p - 1, 2 * p, 3 * p + 1) if n >= 1})


def check_roi_resampling_edges(device, pz, py, px, seed=410):
    """Crop extent against pool size, per axis and independently: box r takes the r-th extent of each axis' own list."""
    s = ROI_EDGE_S
    gen = _gen(seed + 100 * pz + 10 * py + px)
    fm = randn(gen, s, s, s, 2)
    ext = [roi_extents(p) for p in (pz, py, px)]
    nb = max(len(e) for e in ext)
    rows = []
    for r in range(nb):
        n = [e[(r + a) % len(e)] for a, e in enumerate(ext)]           # (shifted per axis: the axes do not move together)
        lo = [int(torch.randint(0, s - nn + 1, (1,), generator=gen)) for nn in n]
        rows.append([lo[0] / s, lo[1] / s, lo[2] / s, (lo[0] + n[0]) / s, (lo[1] + n[1]) / s, (lo[2] + n[2]) / s])
    boxes = torch.tensor(rows, dtype=torch.float32)
    want, _ = _check_roi("roi edges pool=%d,%d,%d" % (pz, py, px), device, fm, boxes, (pz, py, px), seed)
    for a, e in enumerate(ext):
        assert sorted(set((want[:, 3 + a] - want[:, a]).tolist())) == e, "the crop extents are not the ones asked for"


def _ulp(v, k):
    return float(np.nextafter(np.float32(v), np.float32(k * 10.0)))


def check_roi_box_coordinates(device, seed=420):
    """Box coordinates exactly k / S, one ulp either side, negative (python wrap), above 1, lo >= hi -- on a map whose extents
    are no powers of two.  The integer bounds are bit-exact; the values follow the rule."""
    d, h, w, c = 9, 7, 6, 5
    gen = _gen(seed)
    fm = randn(gen, d, h, w, c)
    rows = []
    for k in (1, 2, 3, 5):
        for step in (0, -1, 1):
            lo = [_ulp(k / s, step) if step else float(np.float32(k / s)) for s in (d, h, w)]
            hi = [_ulp((k + 1) / s, step) if step else float(np.float32((k + 1) / s)) for s in (d, h, w)]
            rows.append(lo + hi)
    rows += [[-0.2, -0.1, 0.0, 0.5, 1.2, 0.7], [-0.5, 0.0, 0.0, -0.1, 1.0, 1.0], [0.2, 0.2, 0.2, 1.5, 2.0, 1.01],
             [0.6, 0.1, 0.1, 0.3, 0.9, 0.9], [0.5, 0.5, 0.5, 0.5, 0.5, 0.5], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
             [-1.5, -2.0, -0.01, 1.0, 1.0, 1.0], [1.0, 0.0, 0.0, 1.2, 1.0, 1.0]]
    boxes = torch.tensor(rows, dtype=torch.float32)
    want, _ = _check_roi("roi box coordinates", device, fm, boxes, (4, 3, 5), seed)
    ext = want[:, 3:] - want[:, :3]
    assert (ext.min(axis=1) == 0).any() and (ext.min(axis=1) > 0).any()


def check_roi_counts(device, r, seed=430):
    """R = 64 and 65: the block edge of k_roi_bounds."""
    gen = _gen(seed + r)
    fm = randn(gen, 6, 7, 5, 3)
    lo = torch.rand(r, 3, generator=gen) * 0.6
    boxes = torch.cat([lo, (lo + 0.1 + torch.rand(r, 3, generator=gen) * 0.5).clamp(max=1.0)], dim=1)
    _check_roi("roi R=%d" % r, device, fm, boxes, (2, 2, 3), seed)


def check_roi_zero_rois(device):
    """R = 0: the backward writes zeros over the whole map gradient."""
    lib = _lib.load()
    d, h, w, c = 3, 4, 5, 6
    n = d * h * w * c
    buf, dfm = _dev_slice(torch.full((n,), float("nan")), device, 4)
    bounds = torch.zeros(6, dtype=torch.int32, device=device)
    dout = torch.zeros(8, device=device)
    assert lib.cfun_roi_align3d_bwd(ops.ptr(dout), ops.ptr(bounds), ops.ptr(dfm), 0, d, h, w, c, 2, 2, 2, ops.stream(dfm)) == CFUN_OK
    assert bool((dfm == 0).all()) and _canary_intact(buf, 4, n)


def check_roi_overlap(device, seed=440):
    """40 RoIs that all cover one voxel: its gradient is a 40-term sum in RoI order -- held to float64 under the rule and
    bit-identical across two runs (no atomics)."""
    d, h, w, c = 8, 9, 10, 4
    gen = _gen(seed)
    fm = randn(gen, d, h, w, c)
    lo = torch.rand(40, 3, generator=gen) * 0.45
    hi = 0.55 + torch.rand(40, 3, generator=gen) * 0.45
    boxes = torch.cat([lo, hi], dim=1)
    want, _ = _check_roi("roi 40 overlapping", device, fm, boxes, (3, 2, 4), seed, bwd_seg=c, twice=True)
    centre = np.array([d // 2, h // 2, w // 2])
    assert bool(((want[:, :3] <= centre) & (want[:, 3:] > centre)).all()), "every RoI has to cover the centre voxel"


ROI_SLAB_CUTS = (tuple(range(10)), (0, 3, 4, 9), (0, 1, 9), (0, 5, 9), (0, 9))


def check_roi_slabs(device, seed=450):
    """RoIAlign on depth slabs of a 9-plane map: every one-plane slab, and cuts that fall between a sample's two source
    planes.  The shares sum to the whole and the gradients concatenate to the whole's -- under the rule, against float64."""
    gen = _gen(seed)
    d, h, w, c = 9, 7, 6, 8
    fm = randn(gen, d, h, w, c)
    boxes = torch.tensor([[0.0, 0.0, 0.0, 1.0, 1.0, 1.0], [0.1, 0.2, 0.3, 0.6, 0.9, 0.8], [0.4, 0.0, 0.5, 0.45, 0.3, 0.55],
                          [-0.2, -0.1, 0.0, 0.5, 1.2, 0.7], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [0.3, 0.1, 0.1, 0.9, 0.8, 0.9]])
    pool = (4, 3, 5)               # 4 samples over up to 9 planes: source indices 8/3, 16/3 lie between planes
    gy = randn(gen, boxes.shape[0], *pool, c)
    o64, g64, o32, g32 = _roi_refs(fm, boxes, pool, gy)
    full, b_full, _ = _roi_run(device, fm, boxes, pool, gy)
    for cuts in ROI_SLAB_CUTS:
        total, grads = None, []
        for z0, z1 in zip(cuts[:-1], cuts[1:]):
            part, b, grad = _roi_run(device, fm[z0:z1], boxes, pool, gy, slab=(z0, d))
            assert torch.equal(b.cpu(), b_full.cpu())                  # the crop bounds are those of the whole map
            grads.append(grad)
            total = part if total is None else total + part
        case = "roi slabs %s" % ("one-plane" if len(cuts) == d + 1 else "-".join(map(str, cuts)))
        hold(case, "sum of shares", total, o64, o32)
        hold(case, "dfm", torch.cat(grads, 0), g64, g32, seg=h * w * c)          # per plane
        if len(cuts) == 2:
            assert bits_equal(total, full)


# ========================================================================================== C. NMS
NMS_SIZES = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1088, 1137, 1138, 2047, 2048, 2049, 4095, 4096)
NMS_SCAN_SIZES = tuple(n for n in NMS_SIZES if n <= 129) + (1025,)         # the child's list (CFUN_NMS_SCAN_LDS=0)
NMS_THR = 0.3


def nms_inputs(n, seed=500, levels=None):
    """Clustered boxes: about six to a cluster, cluster membership independent of the index and of the score, so the boxes a
    kept box suppresses are spread over the whole sorted order -- across 64-bit words and 16-row prefetch chunks."""
    rs = np.random.RandomState(seed + n)
    nc = max(1, n // 6)
    centres = rs.rand(nc, 3) * 0.8 + 0.1
    ctr = centres[rs.randint(0, nc, n)] + rs.randn(n, 3) * 0.01
    half = 0.05 + rs.rand(n, 3) * 0.02
    boxes = np.concatenate([ctr - half, ctr + half], axis=1).astype(np.float32)
    scores = rs.rand(n).astype(np.float32)
    if levels:
        scores = (np.floor(scores * levels) / levels).astype(np.float32)
    else:
        assert np.unique(scores).size == n
    return boxes, scores


def nms_ref(boxes, scores, threshold, max_num):
    """orc.nms with the documented order of tied scores (higher score first, then higher original index)
    restated with a STABLE sort -- numpy's default argsort is not stable for long inputs.  Returns (keep, crossed): crossed =
    some kept box suppressed a box in another 64-bit word / another 16-row chunk of the sorted order."""
    boxes, scores = np.asarray(boxes, np.float32), np.asarray(scores, np.float32)
    n = boxes.shape[0]
    z1, y1, x1, z2, y2, x2 = [boxes[:, i] for i in range(6)]
    volume = (z2 - z1) * (y2 - y1) * (x2 - x1)
    order = np.argsort(scores, kind="stable")[::-1]
    alive = np.ones(n, dtype=bool)
    pick, crossed = [], [False, False]
    for pos in range(n):
        i = order[pos]
        if not alive[i]:
            continue
        pick.append(i)
        if len(pick) >= max_num:
            break
        rest = order[pos + 1:]
        iz1 = np.maximum(z1[i], z1[rest]); iz2 = np.minimum(z2[i], z2[rest])
        iy1 = np.maximum(y1[i], y1[rest]); iy2 = np.minimum(y2[i], y2[rest])
        ix1 = np.maximum(x1[i], x1[rest]); ix2 = np.minimum(x2[i], x2[rest])
        inter = np.maximum(ix2 - ix1, 0) * np.maximum(iy2 - iy1, 0) * np.maximum(iz2 - iz1, 0)
        union = volume[i] + volume[rest] - inter
        hit = (inter / (union + np.float32(1e-6))) > np.float32(threshold)
        where = np.nonzero(hit & alive[rest])[0] + pos + 1
        crossed[0] |= bool((where // 64 != pos // 64).any())
        crossed[1] |= bool((where // NMS_CH != pos // NMS_CH).any())
        alive[rest[hit]] = False
    return np.array(pick, dtype=np.int32), tuple(crossed)


def _nms_run(device, boxes, scores, thr, max_num):
    keep, count = ops.nms3d(torch.from_numpy(boxes).to(device), torch.from_numpy(scores).to(device), thr, max_num)
    got = keep[:int(count.item())].cpu().numpy()
    assert got.dtype == np.int32
    return got


def check_nms_size(device, n):
    boxes, scores = nms_inputs(n)
    want, crossed = nms_ref(boxes, scores, NMS_THR, n)
    np.testing.assert_array_equal(want, orc.nms(boxes, scores, NMS_THR, n))          # untied scores: the oracle itself
    assert n < 12 or 1 < want.size < n
    # suppression crosses the 16-row prefetch chunks and the 64-bit words of the sorted order
    assert (n < 63 or crossed[1]) and (n < 127 or crossed[0]), (n, crossed)
    np.testing.assert_array_equal(_nms_run(device, boxes, scores, NMS_THR, n), want)


def check_nms_max_num(device, n=1025):
    boxes, scores = nms_inputs(n)
    survivors = orc.nms(boxes, scores, NMS_THR, n).size
    for max_num in (0, 1, survivors - 1, survivors, survivors + 1, n + 5):
        want = orc.nms(boxes, scores, NMS_THR, max_num)
        np.testing.assert_array_equal(want, nms_ref(boxes, scores, NMS_THR, max_num)[0])
        np.testing.assert_array_equal(_nms_run(device, boxes, scores, NMS_THR, max_num), want, err_msg="max_num=%d" % max_num)


def check_nms_empty_and_limits(device):
    """n = 0: count 0; n = 4097: CFUN_EINVAL; a workspace one byte short: CFUN_EWORKSPACE -- keep and count untouched."""
    lib = _lib.load()
    keep, count = ops.nms3d(torch.zeros(0, 6, device=device), torch.zeros(0, device=device), 0.5, 10)
    assert int(count.item()) == 0
    n = 100
    boxes, scores = (torch.from_numpy(a).to(device) for a in nms_inputs(n))
    keep = torch.full((NMS_MAX_N + 8,), -7, dtype=torch.int32, device=device)
    count = torch.full((4,), -7, dtype=torch.int32, device=device)
    nb = int(lib.cfun_nms3d_workspace_bytes(n))
    ws = torch.zeros(int(lib.cfun_nms3d_workspace_bytes(NMS_MAX_N + 1)) + 256, dtype=torch.uint8, device=device)
    st = ops.stream(boxes)
    big_b, big_s = torch.zeros(NMS_MAX_N + 1, 6, device=device), torch.zeros(NMS_MAX_N + 1, device=device)
    assert lib.cfun_nms3d(ops.ptr(big_b), ops.ptr(big_s), NMS_MAX_N + 1, 0.5, 10, ops.ptr(keep), ops.ptr(count), ops.ptr(ws),
                          ws.numel(), st) == CFUN_EINVAL
    assert lib.cfun_nms3d(ops.ptr(boxes), ops.ptr(scores), n, 0.5, 10, ops.ptr(keep), ops.ptr(count), ops.ptr(ws), nb - 1,
                          st) == CFUN_EWORKSPACE
    assert bool((keep == -7).all()) and bool((count == -7).all())
    assert lib.cfun_nms3d(ops.ptr(boxes), ops.ptr(scores), n, 0.5, 10, ops.ptr(keep), ops.ptr(count), ops.ptr(ws), nb, st) == CFUN_OK
    assert int(count[0]) == 10 and bool((count[1:] == -7).all()) and bool((keep[10:] == -7).all())


def check_nms_thresholds(device):
    # threshold 0: touching boxes (zero intersection: IoU 0 is not > 0) survive; a sliver of overlap does not
    n = 70
    z = np.arange(n, dtype=np.float32)
    boxes = np.stack([z, 0 * z, 0 * z, z + 1, 0 * z + 1, 0 * z + 1], axis=1).astype(np.float32)
    scores = np.linspace(1.0, 0.1, n).astype(np.float32)
    want = orc.nms(boxes, scores, 0.0, n)
    assert want.size == n
    np.testing.assert_array_equal(_nms_run(device, boxes, scores, 0.0, n), want)
    boxes[1::2, 0] -= 0.001                                                   # odd boxes now reach into their left neighbour
    want = orc.nms(boxes, scores, 0.0, n)
    assert want.size == n // 2
    np.testing.assert_array_equal(_nms_run(device, boxes, scores, 0.0, n), want)
    # threshold >= 1: nothing is suppressed (IoU <= v / (v + 1e-6) < 1), exact duplicates included
    n = NMS_MAX_N
    boxes, scores = nms_inputs(n)
    boxes[1::2] = boxes[0::2]
    order = np.argsort(scores, kind="stable")[::-1].astype(np.int32)
    for thr in (1.0, 1.5):
        np.testing.assert_array_equal(orc.nms(boxes, scores, thr, n), order)
        np.testing.assert_array_equal(_nms_run(device, boxes, scores, thr, n), order)
    # exact duplicates at an ordinary threshold: the later of each pair in score order goes
    boxes, scores = nms_inputs(129)
    boxes[1::2] = boxes[0:-1:2]
    want = orc.nms(boxes, scores, NMS_THR, 129)
    np.testing.assert_array_equal(_nms_run(device, boxes, scores, NMS_THR, 129), want)


def check_nms_chain(device):
    """A suppresses B, B would suppress C, A does not: C is kept (suppression is by KEPT boxes only)."""
    def box(z):
        return [z, 0.0, 0.0, z + 1.0, 1.0, 1.0]
    boxes = np.array([box(0.0), box(0.4), box(0.8)], np.float32)              # IoU 0.6/1.4 = 0.43 neighbours, 0.2/1.8 = 0.11 ends
    for perm in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        b = boxes[list(perm)]
        scores = np.array([0.9, 0.8, 0.7], np.float32)[list(perm)]
        want = orc.nms(b, scores, NMS_THR, 3)
        assert want.tolist() == [perm.index(0), perm.index(2)]
        np.testing.assert_array_equal(_nms_run(device, b, scores, NMS_THR, 3), want)


def check_nms_ties(device, n):
    """Scores quantised to 8 levels: the order of equal scores is the documented one (higher original index first)."""
    boxes, scores = nms_inputs(n, levels=8)
    assert np.unique(scores).size <= 8
    want, _ = nms_ref(boxes, scores, NMS_THR, n)
    flipped = nms_ref(boxes[::-1], scores[::-1], NMS_THR, n)[0]
    assert not np.array_equal(n - 1 - flipped, want), "the tie rule does not show in this input"
    np.testing.assert_array_equal(_nms_run(device, boxes, scores, NMS_THR, n), want)


def check_nms_row_scan_child(device, tmp_path):
    """The row-by-row scan (k_nms_scan) at small n: ONE fresh child process with CFUN_NMS_SCAN_LDS=0 (the knob is read once
    per process) runs NMS_SCAN_SIZES and reports its keep lists; compared here.  Which kernel serves a size in THIS process
    is not assumed anywhere."""
    out = os.path.join(str(tmp_path), "nms_row_scan.npz")
    env = dict(os.environ, CFUN_NMS_SCAN_LDS="0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = root + os.pathsep + os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "head_nms_worker.py"), device, out],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    got = dict(np.load(out))
    assert int(got["knob"]) == 0
    for n in NMS_SCAN_SIZES:
        boxes, scores = nms_inputs(n)
        np.testing.assert_array_equal(got["keep_%d" % n], nms_ref(boxes, scores, NMS_THR, n)[0], err_msg="n=%d" % n)
        cut = max(1, n // 20)
        np.testing.assert_array_equal(got["cut_%d" % n], nms_ref(boxes, scores, NMS_THR, cut)[0], err_msg="n=%d max_num=%d" % (n, cut))
    boxes, scores = nms_inputs(65, levels=8)
    np.testing.assert_array_equal(got["ties_65"], nms_ref(boxes, scores, NMS_THR, 65)[0])


def nms_worker_main(device, out):
    """The child's side of check_nms_row_scan_child."""
    res = {"knob": np.int32(int(os.environ.get("CFUN_NMS_SCAN_LDS", "1")))}
    for n in NMS_SCAN_SIZES:
        boxes, scores = nms_inputs(n)
        res["keep_%d" % n] = _nms_run(device, boxes, scores, NMS_THR, n)
        res["cut_%d" % n] = _nms_run(device, boxes, scores, NMS_THR, max(1, n // 20))
    boxes, scores = nms_inputs(65, levels=8)
    res["ties_65"] = _nms_run(device, boxes, scores, NMS_THR, 65)
    np.savez(out, **res)


# ========================================================================================== D. targets and inference tail
# module_cases.check_unmold_golden's two numbers, not new ones: the class map is exact wherever the top two classes differ by
# more than its tie margin, and the share of voxels inside the boxes left out that way is at most its cap
UNMOLD_TIE_MARGIN = 1e-5
UNMOLD_TIE_SHARE = 1e-3


def _interp(mask, size, dt):
    """F.interpolate(trilinear, align_corners=False) of one detection's [md,mh,mw,C] probabilities to ``size`` -> [*size, C]."""
    m = mask.to(dt).permute(3, 0, 1, 2).unsqueeze(0)
    return F.interpolate(m, size=tuple(size), mode="trilinear", align_corners=False)[0].permute(1, 2, 3, 0)


def _overlap_ref(masks, boxes, dhw, dt):
    """orc.unmold_mask_overlap in ``dt``: add + count in detection order, add / (count + fp32(1e-6)), clip."""
    c = masks.shape[-1]
    add = torch.zeros(tuple(dhw) + (c,), dtype=dt)
    cnt = torch.zeros(tuple(dhw) + (1,), dtype=dt)
    for m, b in zip(masks, boxes):
        z1, y1, x1, z2, y2, x2 = [int(v) for v in b]
        add[z1:z2, y1:y2, x1:x2] += _interp(m, (z2 - z1, y2 - y1, x2 - x1), dt)
        cnt[z1:z2, y1:y2, x1:x2] += 1.0
    eps = torch.tensor(1e-6, dtype=torch.float32).to(dt)
    return (add / (cnt + eps)).clamp(0.0, 1.0), cnt[..., 0]


def _hold_class_map(case, labels, ref64, inside):
    """labels exact wherever the float64 top two differ by more than the golden test's tie margin; the share left out at most
    that test's cap of the voxels inside the boxes -- a property of the INPUT, checked on the reference alone."""
    margin, share = UNMOLD_TIE_MARGIN, UNMOLD_TIE_SHARE
    c = ref64.shape[-1]
    want = ref64.argmax(dim=-1)
    if c > 1:
        top2 = torch.topk(ref64, 2, dim=-1).values
        tie = ((top2[..., 0] - top2[..., 1]) < margin) & inside
    else:
        tie = torch.zeros_like(inside)
    assert int(tie.sum()) <= share * int(inside.sum()), "%s: %d near-ties among %d voxels: choose other inputs" % (case, int(tie.sum()), int(inside.sum()))
    got = labels.cpu().long()
    bad = (got != want) & ~tie
    assert not bool(bad.any()), "%s: %d labels differ outside the tie margin, first at %s" % (case, int(bad.sum()), torch.nonzero(bad)[0].tolist())
    assert bool((got[~inside] == 0).all())
    return int(tie.sum())


def _probs(gen, *shape):
    return torch.softmax(3.0 * randn(gen, *shape), dim=-1)


UNMOLD_C = (1, 2, 3, 7, 8, 9, 255)
UNMOLD_MASK = (5, 6, 7)
UNMOLD_DHW = (12, 14, 16)
# one voxel thick per axis, smaller than the mask, equal to it, larger than it
UNMOLD_BOXES = ((3, 2, 1, 4, 8, 8), (1, 5, 2, 6, 6, 9), (2, 3, 7, 7, 9, 8), (4, 4, 4, 7, 8, 9), (6, 7, 8, 11, 13, 15),
                (0, 0, 0, 11, 13, 15), (1, 1, 1, 12, 14, 16))


def check_unmold_argmax(device, c, seed=600):
    """cfun_unmold_argmax: k_unmold_argmax<8> for C = 8, <0> for every other C."""
    gen = _gen(seed + c)
    probs = _probs(gen, *UNMOLD_MASK, c)
    for box in UNMOLD_BOXES:
        labels = ops.unmold_argmax(probs.to(device), box, UNMOLD_DHW)
        ref64, cnt = _overlap_ref(probs[None], [box], UNMOLD_DHW, torch.float64)
        _hold_class_map("unmold_argmax C=%d box=%s" % (c, box), labels, ref64, cnt > 0)
        if c > 1:
            assert bool((labels != 0).any())


def check_unmold_argmax_constant(device):
    """Constant probabilities 1 / C: every channel interpolates to the same value, the first maximum wins -- label 0."""
    for c in (2, 4, 8):
        probs = torch.full(UNMOLD_MASK + (c,), 1.0 / c)
        for box in UNMOLD_BOXES[3:]:
            labels = ops.unmold_argmax(probs.to(device), box, UNMOLD_DHW)
            assert bool((labels == 0).all()), (c, box)


def check_unmold_refusals(device):
    lib = _lib.load()
    d, h, w = UNMOLD_DHW
    md, mh, mw = UNMOLD_MASK
    out = torch.full((d * h * w,), 9, dtype=torch.uint8, device=device)
    full = torch.full((d * h * w * 4,), 555.0, device=device)
    probs = torch.zeros(md * mh * mw * 256 * 2, device=device)
    st = ops.stream(probs)
    i6 = C.c_int32 * 6

    def argmax(c, box):
        return lib.cfun_unmold_argmax(ops.ptr(probs), ops.ptr(out), d, h, w, md, mh, mw, c, i6(*box), st)
    assert argmax(256, (0, 0, 0, 2, 2, 2)) == CFUN_EINVAL
    assert argmax(0, (0, 0, 0, 2, 2, 2)) == CFUN_EINVAL
    for box in ((-1, 0, 0, 2, 2, 2), (0, 0, 0, d + 1, 2, 2), (0, 0, 0, 2, h + 1, 2), (0, 0, 2, 2, 2, w + 1)):
        assert argmax(3, box) == CFUN_EINVAL, box
    one = [0, 0, 0, 1, 1, 1]

    def overlap(n, c, boxes=None):
        boxes = boxes if boxes is not None else one * max(n, 1)
        return lib.cfun_unmold_overlap(ops.ptr(probs), (C.c_int32 * len(boxes))(*boxes), n, ops.ptr(out), ops.ptr(full), d, h, w,
                                       1, 1, 1, c, st)
    for c in (1, 4, 5, 7, 9):                           # classes outside {2, 3, 8}
        assert overlap(1, c) == CFUN_EINVAL, c
    assert overlap(MAX_OVERLAP_BOXES + 1, 3) == CFUN_EINVAL
    assert overlap(1, 3, [0, 0, 0, d + 1, 1, 1]) == CFUN_EINVAL
    assert bool((out == 9).all()) and bool((full == 555.0).all()), "a refused call wrote its output"
    assert overlap(MAX_OVERLAP_BOXES, 3) == CFUN_OK


def check_unmold_overlap(device, c, seed=620):
    """cfun_unmold_overlap: the averaged + clipped probabilities under the rule (n = 1: the plain align_corners=False
    resampling; several overlapping boxes: sums in detection order), the class map exact outside the tie margin."""
    gen = _gen(seed + c)
    for boxes in ([b] for b in UNMOLD_BOXES):
        masks = _probs(gen, 1, *UNMOLD_MASK, c)
        labels, full = ops.unmold_overlap(masks.to(device), boxes, UNMOLD_DHW, want_full=True)
        r64, cnt = _overlap_ref(masks, boxes, UNMOLD_DHW, torch.float64)
        r32, _ = _overlap_ref(masks, boxes, UNMOLD_DHW, torch.float32)
        case = "unmold_overlap C=%d n=1 box=%s" % (c, boxes[0])
        hold(case, "full", full, r64, r32)
        _hold_class_map(case, labels, r64, cnt > 0)
    boxes = list(UNMOLD_BOXES)
    masks = _probs(gen, len(boxes), *UNMOLD_MASK, c)
    labels, full = ops.unmold_overlap(masks.to(device), boxes, UNMOLD_DHW, want_full=True)
    r64, cnt = _overlap_ref(masks, boxes, UNMOLD_DHW, torch.float64)
    r32, _ = _overlap_ref(masks, boxes, UNMOLD_DHW, torch.float32)
    np.testing.assert_array_equal(r32.numpy(), orc.unmold_mask_overlap(masks.numpy(), boxes, [1] + list(UNMOLD_DHW)))   # the oracle
    assert int(cnt.max()) >= 4
    case = "unmold_overlap C=%d n=%d" % (c, len(boxes))
    hold(case, "full", full, r64, r32, seg=UNMOLD_DHW[1] * UNMOLD_DHW[2] * c)
    _hold_class_map(case, labels, r64, cnt > 0)
    assert torch.equal(labels, ops.unmold_overlap(masks.to(device), boxes, UNMOLD_DHW))     # labels only: the same map


def check_unmold_overlap_counts(device, seed=630):
    """n = 64 boxes that all cover one voxel (sum / (64 + 1e-6), clipped); n = 0: zeros."""
    gen = _gen(seed)
    d, h, w = 6, 7, 8
    n, c = MAX_OVERLAP_BOXES, 3
    lo = torch.randint(0, 3, (n, 3), generator=gen)
    hi = torch.randint(4, 7, (n, 3), generator=gen)
    boxes = torch.cat([lo, hi], dim=1).tolist()
    masks = _probs(gen, n, 2, 3, 2, c)
    labels, full = ops.unmold_overlap(masks.to(device), boxes, (d, h, w), want_full=True)
    r64, cnt = _overlap_ref(masks, boxes, (d, h, w), torch.float64)
    r32, _ = _overlap_ref(masks, boxes, (d, h, w), torch.float32)
    assert int(cnt[3, 3, 3]) == n
    hold("unmold_overlap n=64", "full", full, r64, r32, seg=c)
    _hold_class_map("unmold_overlap n=64", labels, r64, cnt > 0)
    labels, full = ops.unmold_overlap(torch.zeros(0, 2, 2, 2, c, device=device), [], (d, h, w), want_full=True)
    assert bool((labels == 0).all()) and bool((full == 0).all())


UNMOLD_BIG_DHW = (65, 255, 257)


def check_unmold_sweeps(device, seed=640):
    """A volume of 4.26 M voxels: two sweeps of the 8192-block grid and a ragged third, labels only.  One box runs through
    every sweep (argmax); a box in the head and one in the tail (overlap)."""
    d, h, w = UNMOLD_BIG_DHW
    total = d * h * w
    assert 2 * UNMOLD_SWEEP < total < 3 * UNMOLD_SWEEP
    gen = _gen(seed)

    def sweeps_hold_labels(labels):
        flat = labels.reshape(-1)
        for s in range(3):
            assert bool((flat[s * UNMOLD_SWEEP:(s + 1) * UNMOLD_SWEEP] != 0).any()), "sweep %d holds no label" % s

    for c in (8, 5):                                                    # <8> and <0>
        probs = _probs(gen, 5, 6, 7, c)
        box = (0, 200, 30, d, 255, 90)                                  # (the third sweep is plane 64 from row y = 2 on)
        labels = ops.unmold_argmax(probs.to(device), box, (d, h, w))
        r64, cnt = _overlap_ref(probs[None], [box], (d, h, w), torch.float64)
        _hold_class_map("unmold_argmax sweeps C=%d" % c, labels, r64, cnt > 0)
        sweeps_hold_labels(labels)
    boxes = [(0, 10, 20, 9, 60, 80), (30, 100, 100, 40, 150, 170), (60, 180, 190, 65, 255, 257)]
    masks = _probs(gen, 3, 4, 5, 6, 3)
    labels = ops.unmold_overlap(masks.to(device), boxes, (d, h, w))
    r64, cnt = _overlap_ref(masks, boxes, (d, h, w), torch.float64)
    _hold_class_map("unmold_overlap sweeps", labels, r64, cnt > 0)
    sweeps_hold_labels(labels)


def _mask_target_ref(lab, rois, shape, classes):
    """orc.mask_targets(...).argmax(1) per RoI; a RoI on whose crop the oracle itself raises (an empty crop: its nearest
    resize indexes an empty axis) is returned as None."""
    onehot = torch.stack([(lab == k) for k in range(classes)], dim=0).float()
    out = []
    for i in range(rois.shape[0]):
        try:
            out.append(orc.mask_targets(rois[i:i + 1], onehot, shape).argmax(1)[0].to(torch.uint8))
        except (IndexError, RuntimeError):
            out.append(None)
    return out


def _py_crop_empty(lab_shape, roi):
    for a, s in enumerate(lab_shape):
        lo, hi = int(np.float32(s) * np.float32(roi[a])), int(np.float32(s) * np.float32(roi[3 + a]))
        lo, hi, _ = slice(lo, hi).indices(s)
        if hi <= lo:
            return True
    return False


def _check_mask_targets(case, device, lab, rois, shape, classes):
    ref = _mask_target_ref(lab, rois, shape, classes)
    out = ops.mask_target_labels(lab.to(torch.uint8).to(device), rois.to(device), shape).cpu()
    raised = []
    for i, want in enumerate(ref):
        empty = _py_crop_empty(lab.shape, rois[i].tolist())
        assert (want is None) == empty, "%s RoI %d: the oracle raises exactly on empty crops" % (case, i)
        if want is None:
            raised.append(i)
            assert bool((out[i] == 0).all()), "%s RoI %d: an empty crop gives zeros" % (case, i)
        else:
            assert torch.equal(out[i], want), "%s RoI %d %s" % (case, i, rois[i].tolist())
    return raised


def check_mask_target_sweeps(device, seed=650):
    """Two sweeps of the 4096-block grid and a ragged third: R = 9, mask 62 x 62 x 61."""
    shape = (62, 62, 61)
    total = 9 * shape[0] * shape[1] * shape[2]
    assert 2 * MASK_TARGET_SWEEP < total < 3 * MASK_TARGET_SWEEP
    gen = _gen(seed)
    lab = torch.randint(0, 3, (12, 20, 17), generator=gen, dtype=torch.int64)
    lo = torch.rand(9, 3, generator=gen) * 0.6
    rois = torch.cat([lo, (lo + 0.08 + torch.rand(9, 3, generator=gen) * 0.35).clamp(max=1.0)], dim=1)
    rois[0] = torch.tensor([0.0, 0.0, 0.0, 1.0, 1.0, 1.0])
    assert _check_mask_targets("mask targets sweeps", device, lab, rois, shape, 3) == []


def check_mask_target_coordinates(device, seed=651):
    """Coordinates at k / D and one ulp either side (int() truncation of the fp32 product), small negatives that truncate to
    0, and negatives <= -1 / D, which the oracle's gt_masks[:, z1:z2, ...] wraps in python slice fashion.  Left out: the RoIs
    whose crop is empty, on which the oracle raises (named by the return value); the kernel gives zeros there."""
    gen = _gen(seed)
    dims = (12, 20, 17)
    lab = torch.randint(0, 5, dims, generator=gen, dtype=torch.int64)
    rows = []
    for k in (1, 3, 7):
        for step in (0, -1, 1):
            lo = [_ulp(k / s, step) if step else float(np.float32(k / s)) for s in dims]
            hi = [_ulp((k + 4) / s, step) if step else float(np.float32((k + 4) / s)) for s in dims]
            rows.append(lo + hi)
    rows += [[-0.01, -0.02, -0.03, 0.5, 0.6, 0.7],                    # truncate to 0
             [-1.0 / 12, 0.0, 0.0, 1.0, 1.0, 1.0],                    # z1 = -1 -> the last plane alone
             [-3.0 / 12, -2.0 / 20, -5.0 / 17, 1.0, 1.0, 1.0],        # the last 3 / 2 / 5
             [-0.5, 0.0, 0.0, -2.0 / 12, 1.0, 1.0],                   # both ends wrap: planes 6 .. 9
             [0.0, 0.0, 0.0, -1.0 / 12, -1.0 / 20, -1.0 / 17],        # hi = -1 -> all but the last
             [-2.0, -2.0, -2.0, 0.5, 0.5, 0.5],                       # lo + S < 0 -> 0
             [0.1, 0.1, 0.1, 1.5, 2.0, 1.2],                          # hi > S clamps
             [-1.0 / 12, 0.0, 0.0, 0.5, 1.0, 1.0],                    # wraps past z2: empty, the oracle raises
             [0.5, 0.5, 0.5, 0.5, 0.9, 0.9]]                          # empty
    rois = torch.tensor(rows, dtype=torch.float32)
    for shape in ((8, 8, 8), (5, 9, 7)):
        raised = _check_mask_targets("mask targets coordinates", device, lab, rois, shape, 5)
        assert raised == [len(rows) - 2, len(rows) - 1], raised


def _resize_ref(vol, out_dims, order, frame, offset, clip, dt):
    """cfun_resize3d restated: the volume sits at ``offset`` inside a zero frame; order 0 reads frame index
    floor((o + 0.5) * P / m) (always in float64: an index), order 1 samples the frame at c = (o + 0.5) * P / m - 0.5 with
    linear weights, zeros outside [0, P) -- coordinates and weights in ``dt``."""
    frame = tuple(frame) if frame is not None else tuple(vol.shape)
    offset = tuple(offset) if offset is not None else (0, 0, 0)
    f = torch.zeros(tuple(p + 2 for p in frame), dtype=dt)                      # one zero voxel all round: the constant 0
    f[tuple(slice(1 + o, 1 + o + n) for o, n in zip(offset, vol.shape))] = vol.to(dt)
    if order == 0:
        idx = [torch.floor((torch.arange(m, dtype=torch.float64) + 0.5) * (p / m)).long().clamp(0, p - 1) + 1
               for m, p in zip(out_dims, frame)]
        return f[idx[0][:, None, None], idx[1][None, :, None], idx[2][None, None, :]]
    i0, w1 = [], []
    for m, p in zip(out_dims, frame):
        c = (torch.arange(m, dtype=dt) + 0.5) * (torch.tensor(p, dtype=dt) / torch.tensor(m, dtype=dt)) - 0.5
        fl = torch.floor(c)
        i0.append(fl.long() + 1)
        w1.append(c - fl)
    out = torch.zeros(tuple(out_dims), dtype=dt)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                wz, wy, wx = ((w if s else 1.0 - w) for w, s in zip(w1, (dz, dy, dx)))
                v = f[(i0[0] + dz)[:, None, None], (i0[1] + dy)[None, :, None], (i0[2] + dx)[None, None, :]]
                out += (wz[:, None, None] * wy[None, :, None] * wx[None, None, :]) * v
    if clip:
        out = out.clamp(float(vol.min()), float(vol.max()))
    return out


RESIZE_CASES = {
    # name: (source dims, out dims, frame, offset, clip)
    "up_noninteger": ((5, 7, 6), (8, 9, 11), None, None, False),
    "down_noninteger": ((11, 13, 9), (4, 5, 7), None, None, False),
    "extent_1_in": ((1, 6, 1), (3, 4, 5), None, None, False),
    "extent_1_out": ((5, 6, 7), (1, 4, 1), None, None, False),
    "clip": ((5, 7, 6), (9, 8, 13), None, None, True),
    "frame_offset": ((5, 7, 6), (9, 11, 10), (8, 12, 7), (2, 3, 1), False),
    "frame_offset_clip_down": ((9, 7, 8), (5, 6, 4), (14, 9, 11), (5, 0, 3), True),
}
RESIZE_BIG_OUT = (129, 255, 257)           # 8 454 015 outputs: two sweeps of the 16384-block grid and a ragged third


def check_resize(device, name, seed=700):
    dims, out_dims, frame, offset, clip = RESIZE_CASES[name]
    gen = _gen(seed + len(name))
    vol = randn(gen, *dims)
    if clip:
        # an all-positive source: the samples that blend in the constant 0 of the border fall below its minimum, so the clamp
        # to the source's range changes outputs -- asserted on the reference, or dropping clip_minmax could not be seen
        vol = vol.abs() + 0.5
        plain, clipped = (_resize_ref(vol, out_dims, 1, frame, offset, c, torch.float64) for c in (False, True))
        assert int((plain != clipped).sum()) > 0 and bool((clipped >= float(vol.min())).all()), name + ": the clip is a no-op"
    # the dense [D,H,W] volume, and the same values as a permuted view of a [H,W,D] array read in place
    hwd = vol.permute(1, 2, 0).contiguous().to(device)
    for tag, src in (("dense", vol.to(device)), ("permuted view", hwd.permute(2, 0, 1))):
        assert tag == "dense" or not src.is_contiguous() or 1 in dims
        case = "resize %s %s" % (name, tag)
        got0 = ops.resize3d(src, out_dims, order=0, frame=frame, offset=offset)
        assert bits_equal(got0, _resize_ref(vol, out_dims, 0, frame, offset, False, torch.float32)), case + ": order 0"
        got1 = ops.resize3d(src, out_dims, order=1, frame=frame, offset=offset, clip=clip)
        hold(case, "order 1", got1, _resize_ref(vol, out_dims, 1, frame, offset, clip, torch.float64),
             _resize_ref(vol, out_dims, 1, frame, offset, clip, torch.float32), seg=out_dims[1] * out_dims[2])


def check_resize_sweeps(device, seed=710):
    total = RESIZE_BIG_OUT[0] * RESIZE_BIG_OUT[1] * RESIZE_BIG_OUT[2]
    assert 2 * RESIZE_SWEEP < total < 3 * RESIZE_SWEEP
    gen = _gen(seed)
    vol = randn(gen, 21, 31, 33)
    src = vol.to(device)
    got0 = ops.resize3d(src, RESIZE_BIG_OUT, order=0)
    assert bits_equal(got0, _resize_ref(vol, RESIZE_BIG_OUT, 0, None, None, False, torch.float32)), "resize sweeps: order 0"
    del got0
    got1 = ops.resize3d(src, RESIZE_BIG_OUT, order=1)
    hold("resize sweeps", "order 1", got1, _resize_ref(vol, RESIZE_BIG_OUT, 1, None, None, False, torch.float64),
         _resize_ref(vol, RESIZE_BIG_OUT, 1, None, None, False, torch.float32), seg=RESIZE_SWEEP)
