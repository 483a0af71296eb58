"""Memory-bound tier: the non-conv kernels of the step's path (csrc/elementwise.hip, loss.hip, loss_fused.hip) against
float64 at the edges their one kernel-level case each in tests/kernel_cases.py does not reach.  Shared by the CPU tier
(HIP emulator, tests/test_membound_emu.py) and the GPU tier (tests/test_membound_gpu.py).

The rule (``hold``) is the product-shape tier's: for every compared tensor there are three evaluations of the same fp32
inputs -- the float64 reference, the torch-CPU fp32 evaluation of that reference, and the kernel.  With e32 the error of the
fp32 evaluation against float64 and ek the kernel's,

    ek <= bench.GRAD_FP64_FACTOR * e32 + bench.GRAD_FP64_FLOOR              (product_shapes.bound)

in two metrics: max-abs error over max-abs of the whole reference tensor (kernel_cases.rel_err), and the same per SEGMENT --
per (n, channel) for the norm kernels, per launch-stride segment [k*S, (k+1)*S) for the flat kernels, S = the elements one
grid sweep covers -- so that an error confined to the second sweep, or to one channel, has to clear the bound on its own.
Where a kernel promises more than the rule (a copy, one correctly rounded operation, an fp64 accumulation rounded once) the
promise is asserted instead (``hold_fp64_sum``, bit-for-bit compares).

Groups: A launch geometry, B value range of norm / activation / pooling, C optimizer tail, D mask losses on trained-looking
inputs.  Every input is seeded here; nothing is read from disk."""
import ctypes as C
import math
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

from product_shapes import bound          # bench.GRAD_FP64_FACTOR * e32 + bench.GRAD_FP64_FLOOR: imported, never copied
from cfun_amd import _lib, loss_ops, ops
from cfun_amd._lib import ACT_LRELU, ACT_NONE, ACT_RELU
from kernel_cases import _gen, randn
from oracle import cfun_oracle as orc

CFUN_OK, CFUN_EINVAL, CFUN_EALIGN = 0, -1, -3           # include/cfun_hip.h

# ---- launch constants, next to the kernel lines they come from (csrc/elementwise.hip).  check_launch_constants() reads each of
# those lines from the source file, which ships with the package, and compares the number in it with the constant here; where
# the library lets one observe the constant from outside (kNormBlocks, the widest strided row, the workspace of the channel
# sum, the direct / reduce switch) it checks that too.  A change of the source then fails a plain assertion instead of moving
# a case silently off the edge it was sized for.
K_BLOCK = 256                    # constexpr int kBlock = 256;
EW_GRID_CAP = 256 * 8            # ew_grid(): if (b > 256 * 8) b = 256 * 8;   -- 2048 blocks, grid-stride the rest
SWEEP = EW_GRID_CAP * K_BLOCK    # work items one sweep of an ew_grid() launch covers (524 288)
SWEEP4 = 4 * SWEEP               # ... in floats for the float4 kernels k_lrelu_fwd / k_lrelu_bwd / k_add
TAIL = 1024                      # for (from = n4 * 4; from < n; from += 1024): one 1024-thread block per tail launch
K_NORM_BLOCKS = 512              # constexpr int kNormBlocks = 512;
NORM_SWEEP = K_NORM_BLOCKS * K_BLOCK      # elements one sweep of k_sumsq_partials covers (131 072)
SUM_DIRECT_MAX = 4096            # sum_direct_max(): 1 << 12 rows for the one-launch k_channel_sum_direct
APPLY_VOX_PER_THREAD = 4         # apply_blocks(): b = ceil(V / (lanes * 4))
MAX_GROUPS = K_BLOCK             # if (C / 4 > kBlock) return CFUN_EINVAL;  (C / vec_of(C) > kBlock for the norm entries)
SLOPE = float(np.float32(ops.LRELU_SLOPE))       # the slope as the C ABI receives it (a float argument)
EPS = 1e-5

# ---- the parity table: every hold() appends a row; the GPU tier prints it (profiles/membound_parity.txt is such a run)
REPORT = []


def report_lines():
    """One line per (case, tensor, metric); the flat and strided activation cases, which are asserted bit for bit against
    torch fp32 (so ek = e32 in every row), are folded into one line per tensor and metric: the row nearest to its bound."""
    rows, folded = [], {}
    for row in REPORT:
        case, what, metric = row[:3]
        fam = case.split()[0] if case.split()[0] in ("flat", "strided") else None
        if fam is None:
            rows.append(row)
            continue
        key = (fam, what, metric)
        if key not in folded:
            folded[key] = [row, 0]
            rows.append(key)
        folded[key][1] += 1
        if row[4] / row[5] > folded[key][0][4] / folded[key][0][5]:
            folded[key][0] = row
    out = []
    for row in rows:
        if row in folded:
            (case, what, metric, e32, ek, bnd), count = folded[row]
            case = "%s (worst of %d cases: %s)" % (row[0], count, case[len(row[0]) + 1:])
        else:
            case, what, metric, e32, ek, bnd = row
        out.append("%-66s %-26s %-7s e32 %.3e  ek %.3e  bound %.3e  ek/e32 %-8s %.3f of bound"
                   % (case, what, metric, e32, ek, bnd, ("%.2f" % (ek / e32)) if e32 > 0 else ("0" if ek == 0 else "inf"),
                      ek / bnd))
    return out


# ------------------------------------------------------------------------------------------ the rule
def _d(t):
    return t.detach().cpu().double()


def _seg_max(a, seg, start=0):
    """max of |a| per segment.  seg = int S: flat segments [k*S, (k+1)*S) of the flattened tensor, whose element 0 sits at
    offset ``start`` of the launch (a parameter inside an arena); seg = "nc": per (n, channel) of an [N, ..., C] tensor."""
    if seg == "nc":
        n, c = a.shape[0], a.shape[-1]
        return a.reshape(n, -1, c).amax(dim=1).reshape(-1)
    flat = a.reshape(-1)
    front = start % seg
    total = front + flat.numel()
    pad = (-total) % seg
    # (padding with zeros leaves a segment's maximum alone; a NaN anywhere in a segment makes its maximum NaN)
    flat = torch.cat([flat.new_zeros(front), flat, flat.new_zeros(pad)])
    return flat.reshape(-1, seg).amax(dim=1)


def hold(case, what, got, ref64, ref32, seg=None, start=0, keep=None):
    """The rule, whole-tensor and per segment.  ``keep``: a boolean mask of the elements that are compared (the LeakyReLU
    kink band and torch's own NaNs are taken out by the caller, who also bounds their share)."""
    assert tuple(got.shape) == tuple(ref64.shape) == tuple(ref32.shape), (case, what, got.shape, ref64.shape, ref32.shape)
    g, r, s = _d(got), _d(ref64), _d(ref32)
    dk, d3, ra = (g - r).abs(), (s - r).abs(), r.abs()
    if keep is not None:
        keep = keep.cpu()
        zero = torch.zeros((), dtype=torch.float64)
        dk, d3, ra = torch.where(keep, dk, zero), torch.where(keep, d3, zero), torch.where(keep, ra, zero)
    whole = float(ra.max()) if ra.numel() else 0.0
    ek, e32 = float(dk.max()) / (whole + 1e-30), float(d3.max()) / (whole + 1e-30)
    REPORT.append((case, what, "whole", e32, ek, bound(e32)))
    assert ek <= bound(e32), ("%s %s: whole-tensor error %.3e above the bound %.3e (the fp32 reference is %.3e from float64)"
                              % (case, what, ek, bound(e32), e32))
    if seg is None or not ra.numel():
        return
    mk, m3, mr = _seg_max(dk, seg, start), _seg_max(d3, seg, start), _seg_max(ra, seg, start)
    # A segment whose reference is (about) zero -- a constant channel's output, a zero gradient channel -- would make the
    # bound 0/0: there the denominator is the whole tensor's max-abs.
    den = torch.where(mr > 1e-6 * whole, mr, torch.full_like(mr, whole)) + 1e-30
    eks, e3s = mk / den, m3 / den
    # the reported segment is the one nearest to its bound as a RATIO (a segment that holds a NaN first: caught below)
    ratio = eks / bound(e3s)
    worst = int(torch.argmax(torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)))
    REPORT.append((case, what, "segment", float(e3s[worst]), float(eks[worst]), bound(float(e3s[worst]))))
    bad = ~(eks <= bound(e3s))
    assert not bool(bad.any()), ("%s %s: %d of %d segments (%s) above the bound, first %d: error %.3e, bound %.3e"
                                 % (case, what, int(bad.sum()), bad.numel(), seg, int(torch.nonzero(bad)[0]),
                                    float(eks[bad][0]), bound(float(e3s[bad][0]))))


def hold_fp64_sum(case, what, got, ref64, terms, abs_sum):
    """The contract of a reduction accumulated in fp64 and rounded to fp32 once (cfun_channel_sum, the statistics' mean, the
    gradient norm): |out - ref64| <= 2^-23 |ref64| + terms * 2^-52 * sum|terms|.  Derived, not measured: one rounding to fp32
    is at most half an ulp (2^-24 relative; 2^-23 leaves the reference's own last bit), and ``terms`` fp64 additions in any
    order lose at most terms * 2^-53 of the sum of magnitudes."""
    g, r, a = _d(got), _d(ref64), _d(abs_sum)
    lim = 2.0 ** -23 * r.abs() + terms * 2.0 ** -52 * a
    err = (g - r).abs()
    bad = ~(err <= lim)
    REPORT.append((case, what, "fp64sum", 0.0, float((err / (r.abs() + 1e-300)).max()) if r.numel() else 0.0, 2.0 ** -23))
    assert not bool(bad.any()), ("%s %s: %d of %d outside the fp64-accumulation contract, first %d: |err| %.3e > %.3e"
                                 % (case, what, int(bad.sum()), bad.numel(), int(torch.nonzero(bad.reshape(-1))[0]),
                                    float(err[bad][0]), float(lim[bad][0])))


def bits_equal(a, b):
    """Bit for bit, the sign of a zero and the payload-free NaNs included."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _dev_slice(values, device, off, room=8):
    """``values`` (1-D fp32) placed at element ``off`` of a fresh allocation: the slice's pointer is 4 * off bytes past a
    16-byte boundary.  Returns (whole buffer, the slice); the rest of the buffer is a canary of 777s."""
    buf = torch.full((values.numel() + room,), 777.0, dtype=torch.float32, device=device)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + values.numel()]
    view.copy_(values)
    return buf, view


def _canary_intact(buf, off, n):
    return bool((buf[:off] == 777.0).all()) and bool((buf[off + n:] == 777.0).all())


def _lrelu(x, slope):
    return torch.where(x > 0, x, x * slope)


def _lrelu_grad(x, dy, slope):
    return torch.where(x > 0, dy, dy * slope)


# ========================================================================================== A. launch geometry
def check_launch_constants(device):
    """The constants above against what the library lets one observe."""
    lib = _lib.load()
    src = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", "elementwise.hip")).read()

    def one(pattern):
        found = re.findall(pattern, src, re.S)
        assert len(found) >= 1 and len(set(found)) == 1, "elementwise.hip: %r matches %s" % (pattern, found)
        return found[0]

    assert int(one(r"constexpr int kBlock = (\d+);")) == K_BLOCK
    # ew_grid(): the cap of every grid-stride launch -- what FLAT_BIG_N, ACT_BWD_NVOX, POOL_SHAPE, HALO_SHAPE and SGD_N are sized by
    body = one(r"inline unsigned ew_grid\(int64_t work_items\) \{(.*?)\n\}")
    assert re.search(r"\(work_items \+ kBlock - 1\) / kBlock;", body), "ew_grid(): one work item per thread is assumed"
    cap = re.findall(r"if \(b > (\d+) \* (\d+)\) b = (\d+) \* (\d+);", body)
    assert len(cap) == 1 and cap[0][:2] == cap[0][2:] and int(cap[0][0]) * int(cap[0][1]) == EW_GRID_CAP, cap
    # every entry that launches through ew_grid() strides by the whole grid
    assert len(re.findall(r"i \+= \(int64_t\)gridDim\.x \* kBlock\)", src)) >= 10
    # the scalar tail launches of cfun_lrelu_fwd / _bwd / cfun_add: one 1024-thread block per 1024 elements
    assert set(re.findall(r"for \(int64_t from = n4 \* 4; from < n; from \+= (\d+)\)", src)) == {str(TAIL)}
    assert set(re.findall(r"k_\w+_tail, dim3\(1\), dim3\((\d+)\)", src)) == {str(TAIL)}
    assert len(re.findall(r"for \(int64_t from = n4 \* 4; from < n; from \+= \d+\)", src)) == 3
    # apply_blocks(): voxels per thread of the per-sample apply kernels, and its own cap
    body = one(r"inline unsigned apply_blocks\(int64_t V, int lanes\) \{(.*?)\n\}")
    per = re.findall(r"\(V \+ \(int64_t\)lanes \* (\d+) - 1\) / \(\(int64_t\)lanes \* (\d+)\);", body)
    assert per == [(str(APPLY_VOX_PER_THREAD),) * 2], per
    assert int(one(r"constexpr int kNormBlocks = (\d+);")) == K_NORM_BLOCKS
    assert re.search(r"hipLaunchKernelGGL\(k_sumsq_partials, dim3\(kNormBlocks\), dim3\(kBlock\)", src)
    assert 1 << int(one(r"lim = \(int64_t\)1 << \(e \? atoi\(e\) : (\d+)\);")) == SUM_DIRECT_MAX
    assert "CFUN_SUM_DIRECT_LOG2" not in os.environ, "the cases are sized for the default direct / reduce switch"
    assert len(re.findall(r"if \(C / 4 > kBlock\) return CFUN_EINVAL;", src)) == 3
    assert SWEEP == EW_GRID_CAP * K_BLOCK and SWEEP4 == 4 * SWEEP and NORM_SWEEP == K_NORM_BLOCKS * K_BLOCK
    assert int(lib.cfun_sumsq_partials_count()) == K_NORM_BLOCKS
    # kBlock: the widest row the strided activation takes is kBlock float4 groups
    t = torch.zeros(4 * (MAX_GROUPS + 1) * 2, device=device)
    assert lib.cfun_lrelu_fwd_strided(ops.ptr(t), ops.ptr(t), 1, 4 * MAX_GROUPS, 4 * MAX_GROUPS, 4 * MAX_GROUPS, SLOPE,
                                      ops.stream(t)) == CFUN_OK
    assert lib.cfun_lrelu_fwd_strided(ops.ptr(t), ops.ptr(t), 1, 4 * (MAX_GROUPS + 1), 4 * (MAX_GROUPS + 1), 4 * (MAX_GROUPS + 1),
                                      SLOPE, ops.stream(t)) == CFUN_EINVAL
    # reduce_plan(): lanes = kBlock / CG, blocks = min(ceil(1024 / N), ceil(V / (16 * lanes))); the workspace of the channel
    # sum is blocks * C doubles rounded up to 256 bytes -- readable through cfun_channel_sum_workspace_bytes
    for v, c in ((1, 4), (SUM_DIRECT_MAX + 1, 16), (20000, 1024), (20000, 3), (100000, 4)):
        cg = c // (1 if c % 4 else 4)
        lanes = K_BLOCK // cg
        blocks = min(1024, max(1, -(-v // (16 * lanes))))
        assert int(lib.cfun_channel_sum_workspace_bytes(v, c)) == -(-(blocks * c * 8) // 256) * 256, (v, c)
    # sum_direct_max() = 4096 is not observable from outside (both paths give the same sums to the last bit or two); it is
    # pinned by check_channel_sum's rows 4096 / 4097, which differ in the workspace they poison: see there.


FLAT_SMALL_N = (1, 3, 4, 5, 1023, 1025, 2051)
FLAT_BIG_N = 2 * SWEEP4 + 4 * 77 + 3         # two full sweeps of float4s, a ragged third, a 3-element scalar tail


def _flat_inputs(n, seed):
    gen = _gen(seed)
    x, dy, b = randn(gen, n), randn(gen, n), randn(gen, n)
    # the kink and the values next to it: +0, -0, the smallest denormals and normals of either sign (x > 0 is exact in any
    # precision, so no band is needed; the derivative at 0 is the slope, as in torch)
    special = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 1.17549435e-38, -1.17549435e-38],
                           dtype=torch.float32)
    k = min(n, special.numel())
    pos = torch.randperm(n, generator=gen)[:k]
    x[pos] = special[:k]
    return x, dy, b


def check_flat_elementwise(device, n, offs=(0, 0, 0), seed=101):
    """cfun_lrelu_fwd / cfun_lrelu_bwd / cfun_add at the C ABI on n elements; offs = element offsets of (first input, second
    input, output) from a 16-byte boundary -- any non-zero offset must send the whole call down the scalar path (one
    1024-thread launch per 1024 elements).  One operation per element, correctly rounded: bit for bit against torch fp32, and
    the rule per sweep segment against float64."""
    lib = _lib.load()
    case = "flat n=%d offs=%s" % (n, "".join(map(str, offs)))
    x, dy, b = _flat_inputs(n, seed)
    o_a, o_b, o_out = offs
    _, xd = _dev_slice(x, device, o_a)
    _, dyd = _dev_slice(dy, device, o_b)
    _, bd = _dev_slice(b, device, o_b)
    st = ops.stream(xd)
    nan = torch.full((n,), float("nan"))
    slope32 = torch.tensor(SLOPE, dtype=torch.float32)
    # forward: (x, y)
    ybuf, y = _dev_slice(nan, device, o_out)
    assert lib.cfun_lrelu_fwd(ops.ptr(xd), ops.ptr(y), n, SLOPE, st) == CFUN_OK
    ref32 = _lrelu(x, slope32)
    assert bits_equal(y, ref32), case + ": lrelu forward differs from torch fp32 bit for bit"
    hold(case, "lrelu y", y, _lrelu(x.double(), SLOPE), ref32, seg=SWEEP4)
    assert _canary_intact(ybuf, o_out, n), case + ": lrelu forward wrote outside its n elements"
    # backward: (x, dy, dx)
    dbuf, dx = _dev_slice(nan, device, o_out)
    assert lib.cfun_lrelu_bwd(ops.ptr(xd), ops.ptr(dyd), ops.ptr(dx), n, SLOPE, st) == CFUN_OK
    ref32 = _lrelu_grad(x, dy, slope32)
    assert bits_equal(dx, ref32), case + ": lrelu backward differs from torch fp32 bit for bit"
    hold(case, "lrelu dx", dx, _lrelu_grad(x.double(), dy.double(), SLOPE), ref32, seg=SWEEP4)
    assert _canary_intact(dbuf, o_out, n), case + ": lrelu backward wrote outside its n elements"
    # add: (a, b, out)
    obuf, out = _dev_slice(nan, device, o_out)
    assert lib.cfun_add(ops.ptr(xd), ops.ptr(bd), ops.ptr(out), n, st) == CFUN_OK
    assert bits_equal(out, x + b), case + ": add differs from torch fp32 bit for bit"
    hold(case, "add", out, x.double() + b.double(), x + b, seg=SWEEP4)
    assert _canary_intact(obuf, o_out, n), case + ": add wrote outside its n elements"


def check_flat_through_ops(device, seed=102):
    """The same three kernels through ops (autograd) on a tensor past one sweep -- the wrappers' own sizes and pointers."""
    gen = _gen(seed)
    n = SWEEP4 + 4 * 77 + 3
    x, gy, b = randn(gen, n), randn(gen, n), randn(gen, n)
    xd = x.clone().to(device).requires_grad_(True)
    y = ops.lrelu(xd)
    y.backward(gy.to(device))
    slope32 = torch.tensor(SLOPE, dtype=torch.float32)
    hold("ops.lrelu n=%d" % n, "y", y, _lrelu(x.double(), SLOPE), _lrelu(x, slope32), seg=SWEEP4)
    hold("ops.lrelu n=%d" % n, "dx", xd.grad, _lrelu_grad(x.double(), gy.double(), SLOPE), _lrelu_grad(x, gy, slope32), seg=SWEEP4)
    hold("ops.add n=%d" % n, "out", ops.add(x.to(device), b.to(device)), x.double() + b.double(), x + b, seg=SWEEP4)


STRIDED_C = (4, 20, 40, 1024)        # kBlock / (C / 4) = 256, 51 (one idle thread), 25 (six idle), 1 voxel lanes per block


def _strided_nvox(c):
    lanes = K_BLOCK // (c // 4)
    one = lanes * APPLY_VOX_PER_THREAD - 1 if lanes > 1 else 3        # apply_blocks() = 1
    several = 3 * lanes * APPLY_VOX_PER_THREAD + lanes + 1            # 4 blocks, the last one ragged, uneven trip counts
    assert -(-one // (lanes * APPLY_VOX_PER_THREAD)) == 1 and -(-several // (lanes * APPLY_VOX_PER_THREAD)) == 4
    return one, several


def check_lrelu_strided(device, c, seed=103):
    """cfun_lrelu_fwd_strided / _bwd_strided / _bwd_add at the C ABI: rows of C floats inside rows of ``rs`` floats, the
    channel range at the first and at the last columns.  Bit for bit against torch fp32 (one operation per element, plus one
    addition for _bwd_add), the rule per channel, and not a float of the wide rows outside the range touched."""
    lib = _lib.load()
    gen = _gen(seed + c)
    slope32 = torch.tensor(SLOPE, dtype=torch.float32)
    for nvox in _strided_nvox(c):
        x, dy, add = randn(gen, nvox, c), randn(gen, nvox, c), randn(gen, nvox, c)
        x[0, 0], x[nvox - 1, c - 1] = 0.0, -0.0
        y32, dx32 = _lrelu(x, slope32), _lrelu_grad(x, dy, slope32)
        y64, dx64 = _lrelu(x.double(), SLOPE), _lrelu_grad(x.double(), dy.double(), SLOPE)
        xd, dyd, addd = x.to(device), dy.to(device), add.to(device)
        st = ops.stream(xd)
        for rs in (c, c + 4, 3 * c):
            for c0 in sorted({0, rs - c}):
                case = "strided C=%d nvox=%d rs=%d c0=%d" % (c, nvox, rs, c0)
                fill = randn(gen, nvox, rs)
                # forward, dense x -> wide y; then wide x -> dense y
                wide = fill.clone().to(device)
                assert lib.cfun_lrelu_fwd_strided(ops.ptr(xd), ops.ptr_raw(wide[:, c0:c0 + c]), nvox, c, c, rs, SLOPE, st) == CFUN_OK
                got = wide[:, c0:c0 + c].cpu()
                assert bits_equal(got, y32), case + ": forward into the wide rows"
                hold(case, "y (wide y)", got[None], y64[None], y32[None], seg="nc")
                wide[:, c0:c0 + c] = fill[:, c0:c0 + c].to(device)
                assert torch.equal(wide.cpu(), fill), case + ": forward wrote outside the channel range"
                wide[:, c0:c0 + c] = xd
                y = torch.full((nvox, c), float("nan"), device=device)
                assert lib.cfun_lrelu_fwd_strided(ops.ptr_raw(wide[:, c0:c0 + c]), ops.ptr(y), nvox, c, rs, c, SLOPE, st) == CFUN_OK
                assert bits_equal(y, y32), case + ": forward out of the wide rows"
                # backward: the gradient is the channel range of the wide rows
                wide[:, c0:c0 + c] = dyd
                dyv = wide[:, c0:c0 + c]
                dx = torch.full((nvox, c), float("nan"), device=device)
                assert lib.cfun_lrelu_bwd_strided(ops.ptr(xd), ops.ptr_raw(dyv), ops.ptr(dx), nvox, c, rs, SLOPE, st) == CFUN_OK
                assert bits_equal(dx, dx32), case + ": backward"
                hold(case, "dx", dx[None], dx64[None], dx32[None], seg="nc")
                # (rs == C takes the flat k_lrelu_bwd with its add operand, rs > C the strided kernel's)
                for a_t, a_ref in ((addd, add), (None, None)):
                    dx = torch.full((nvox, c), float("nan"), device=device)
                    assert lib.cfun_lrelu_bwd_add(ops.ptr(xd), ops.ptr_raw(dyv), ops.ptr(a_t), ops.ptr(dx), nvox, c, rs, SLOPE, st) == CFUN_OK
                    want32 = dx32 if a_ref is None else dx32 + a_ref
                    want64 = dx64 if a_ref is None else _lrelu_grad(x.double(), dy.double(), SLOPE) + a_ref.double()
                    assert bits_equal(dx, want32), case + ": backward + add"
                    hold(case, "dx + add" if a_ref is not None else "dx (add = NULL)", dx[None], want64[None], want32[None], seg="nc")


def check_lrelu_strided_too_wide(device):
    """C = 1028 is 257 float4 groups, one more than a block has threads: CFUN_EINVAL from all three entries, nothing written."""
    lib = _lib.load()
    c = 4 * (MAX_GROUPS + 1)
    x = torch.ones(2, c, device=device)
    out = torch.full((2, c), 777.0, device=device)
    st = ops.stream(x)
    assert lib.cfun_lrelu_fwd_strided(ops.ptr(x), ops.ptr(out), 2, c, c, c, SLOPE, st) == CFUN_EINVAL
    assert lib.cfun_lrelu_bwd_strided(ops.ptr(x), ops.ptr(x), ops.ptr(out), 2, c, c, SLOPE, st) == CFUN_EINVAL
    assert lib.cfun_lrelu_bwd_add(ops.ptr(x), ops.ptr(x), ops.ptr(x), ops.ptr(out), 2, c, c, SLOPE, st) == CFUN_EINVAL
    assert bool((out == 777.0).all())


ACT_BWD_C = 7
ACT_BWD_N = 3
# total = nvox * C has to be a multiple of C = 7 and of N = 3: the smallest such total that is at least 2 * SWEEP + 77
ACT_BWD_NVOX = -(-(2 * SWEEP + 77) // (ACT_BWD_C * ACT_BWD_N)) * ACT_BWD_N


def check_act_bwd(device, seed=104):
    """cfun_act_bwd: g = dy * act'(y) * scale over two sweeps and a ragged third, C = 7, 3 samples whose voxel count does not
    divide the sweep; every activation x every scale mode (none, per channel, per (sample, channel))."""
    lib = _lib.load()
    gen = _gen(seed)
    c, n, nvox = ACT_BWD_C, ACT_BWD_N, ACT_BWD_NVOX
    per = nvox // n
    assert nvox * c >= 2 * SWEEP + 77 and nvox * c < 2 * SWEEP + 77 + c * n and SWEEP % per != 0
    y, dy = randn(gen, nvox, c), randn(gen, nvox, c)
    y[::1013] = 0.0                    # exact zeros: !(y > 0) takes the negative branch
    sc1, sc2 = torch.rand(c, generator=gen) + 0.5, torch.rand(n, c, generator=gen) + 0.5
    yd, dyd = y.to(device), dy.to(device)
    slope32 = torch.tensor(SLOPE, dtype=torch.float32)
    for act in (ACT_NONE, ACT_RELU, ACT_LRELU):
        for mode, scale in ((0, None), (1, sc1), (2, sc2)):
            def ref(dt, slope):
                d = dy.to(dt)
                if act == ACT_RELU:
                    d = torch.where(y > 0, d, torch.zeros((), dtype=dt))
                elif act == ACT_LRELU:
                    d = torch.where(y > 0, d, d * slope)
                if mode == 1:
                    d = d * scale.to(dt)
                elif mode == 2:
                    d = (d.reshape(n, per, c) * scale.to(dt)[:, None, :]).reshape(nvox, c)
                return d
            g = torch.full((nvox, c), float("nan"), device=device)
            assert lib.cfun_act_bwd(ops.ptr(yd), ops.ptr(dyd), ops.ptr(None if scale is None else scale.to(device)), ops.ptr(g),
                                    nvox, c, per, act, SLOPE, mode, ops.stream(yd)) == CFUN_OK
            r32 = ref(torch.float32, slope32)
            case = "act_bwd act=%d scale_mode=%d" % (act, mode)
            assert bits_equal(g, r32), case + ": differs from torch fp32 bit for bit (at most two correctly rounded products)"
            hold(case, "g", g, ref(torch.float64, SLOPE), r32, seg=SWEEP)
    assert lib.cfun_act_bwd(ops.ptr(yd), ops.ptr(dyd), None, ops.ptr(yd), nvox, c, per, ACT_NONE, SLOPE, 1, ops.stream(yd)) == CFUN_EINVAL


# N, D, H, W, C pairwise different so that a swapped axis in the index decomposition cannot cancel; more than two sweeps of
# work items.  POOL_SHAPE is the LOW-resolution side (pool output, upsample-backward output); the other side has 8x the voxels.
POOL_SHAPE = (3, 10, 14, 16, 157)             # 1 055 040 work items (C odd: the VEC = 1 form), 33.8 MB on the 2x side
POOL_SHAPE_VEC4 = (3, 10, 14, 16, 628)        # C = 4 * 157: 1 055 040 float4 work items of the VEC = 4 upsample backward
HALO_SHAPE = (2, 7, 24, 29, 157)              # with planes z in [1, 6): 2 * 5 * 24 * 29 * 157 = 1 092 720 work items


def _pairwise_different(shape):
    return len(set(shape)) == len(shape)


def check_upsample2_bwd(device, shape=POOL_SHAPE, seed=105):
    """cfun_upsample2_bwd: lo[n,z,y,x,c] = the sum of the 8 hi voxels; the rule per sweep segment."""
    lib = _lib.load()
    n, d, h, w, c = shape
    vec = 1 if c % 4 else 4
    assert _pairwise_different(shape) and n * d * h * w * (c // vec) > 2 * SWEEP
    gen = _gen(seed)
    hi = randn(gen, n, 2 * d, 2 * h, 2 * w, c)
    hid = hi.to(device)
    lo = torch.full(shape, float("nan"), device=device)
    assert lib.cfun_upsample2_bwd(ops.ptr(hid), ops.ptr(lo), n, d, h, w, c, ops.stream(hid)) == CFUN_OK
    v = hi.view(n, d, 2, h, 2, w, 2, c)
    hold("upsample2_bwd %s" % (shape,), "lo", lo, v.double().sum(dim=(2, 4, 6)), v.sum(dim=(2, 4, 6)), seg=SWEEP * vec)


def _torch_pool(x):
    """torch CPU max_pool3d of NDHWC x: (y, k) with k = 4*dz + 2*dy + dx the position of the maximum inside its window --
    torch's own choice among ties (the first in (d, h, w) order) and NaNs (propagated; the last NaN of a window)."""
    n, d, h, w, c = x.shape
    y, flat = F.max_pool3d(x.permute(0, 4, 1, 2, 3), 2, 2, return_indices=True)
    z, r = flat // (h * w), flat % (h * w)
    k = (z % 2) * 4 + ((r // w) % 2) * 2 + (r % w) % 2
    return y.permute(0, 2, 3, 4, 1).contiguous(), k.permute(0, 2, 3, 4, 1).contiguous().to(torch.uint8)


def check_maxpool_exact(device, x, gy, case):
    """cfun_maxpool2_fwd / _bwd at the C ABI against torch CPU with NO tie mask: y bit for bit (NaNs included), the saved
    index equal to torch's choice, dx bit for bit.  A copy has no rounding: the contract is equality, stronger than the rule."""
    lib = _lib.load()
    n, d, h, w, c = x.shape
    do, ho, wo = d // 2, h // 2, w // 2
    xr = x.clone().requires_grad_(True)
    yr = F.max_pool3d(xr.permute(0, 4, 1, 2, 3), 2, 2).permute(0, 2, 3, 4, 1)
    yr.backward(gy)
    y_t, k_t = _torch_pool(x)
    xd, gyd = x.to(device), gy.to(device)
    y = torch.full((n, do, ho, wo, c), 777.0, device=device)
    idx = torch.full((n, do, ho, wo, c), 255, dtype=torch.uint8, device=device)
    st = ops.stream(xd)
    assert lib.cfun_maxpool2_fwd(ops.ptr(xd), ops.ptr(y), ops.ptr(idx), n, do, ho, wo, c, st) == CFUN_OK
    assert torch.equal(torch.isnan(y.cpu()), torch.isnan(y_t)), case + ": NaNs are not where torch puts them"
    assert bits_equal(torch.nan_to_num(y.cpu(), nan=12345.0), torch.nan_to_num(y_t, nan=12345.0)), case + ": pooled values differ from torch"
    mism = idx.cpu() != k_t
    assert not bool(mism.any()), (case + ": %d of %d windows route to another element than torch (first maximum in (d, h, w) "
                                  "order; a NaN wins)" % (int(mism.sum()), mism.numel()))
    dx = torch.full(tuple(x.shape), float("nan"), device=device)
    assert lib.cfun_maxpool2_bwd(ops.ptr(gyd), ops.ptr(idx), ops.ptr(dx), n, do, ho, wo, c, st) == CFUN_OK
    assert bits_equal(dx, xr.grad), case + ": dx differs from torch (no tie mask)"
    # and through ops (autograd)
    xa = x.clone().to(device).requires_grad_(True)
    ops.maxpool2(xa).backward(gyd)
    assert bits_equal(xa.grad, xr.grad), case + ": ops.maxpool2 dx differs from torch (no tie mask)"


def check_maxpool_geometry(device, seed=106):
    n, d, h, w, c = POOL_SHAPE
    assert _pairwise_different(POOL_SHAPE) and n * d * h * w * c > 2 * SWEEP
    gen = _gen(seed)
    check_maxpool_exact(device, randn(gen, n, 2 * d, 2 * h, 2 * w, c), randn(gen, n, d, h, w, c), "maxpool %s" % (POOL_SHAPE,))


def check_halo_geometry(device, seed=107):
    """cfun_halo_pack / _unpack: planes [1, 6) of 7, more than two sweeps; copies, so bit for bit, and the planes outside
    the range untouched."""
    n, d, h, w, c = HALO_SHAPE
    z0, planes = 1, 5
    assert _pairwise_different(HALO_SHAPE) and n * planes * h * w * c > 2 * SWEEP
    gen = _gen(seed)
    x = randn(gen, *HALO_SHAPE)
    xd = x.to(device)
    buf = ops.halo_pack(xd, z0, planes)
    assert bits_equal(buf, x[:, z0:z0 + planes]), "halo_pack over two sweeps"
    dst = torch.full(HALO_SHAPE, 777.0, device=device)
    ops.halo_unpack(buf, dst, z0)
    got = dst.cpu()
    assert bits_equal(got[:, z0:z0 + planes], x[:, z0:z0 + planes]), "halo_unpack over two sweeps"
    assert bool((got[:, :z0] == 777.0).all()) and bool((got[:, z0 + planes:] == 777.0).all()), "halo_unpack left its planes"


CHANNEL_SUM_ROWS = (1, 63, 64, 65, SUM_DIRECT_MAX, SUM_DIRECT_MAX + 1, 20000)
CHANNEL_SUM_C = (1, 3, 16, 20, 36, 1024)


def check_channel_sum(device, rows, c, seed=108):
    """cfun_channel_sum (through ops.channel_sum): 4096 rows is the last size of the one-launch k_channel_sum_direct, 4097 the
    first of reduce + finalize; C = 20 leaves the direct kernel's second block half empty; C in {1, 3} is the scalar reduce.
    fp64 accumulators, one rounding: the fp64-sum contract.  Columns offset by up to 1e4 of their spread, so an fp32
    accumulation (1e-7 * rows * 1e4) is far outside it."""
    gen = _gen(seed + 7 * rows + c)
    g = randn(gen, rows, c) + (torch.arange(c, dtype=torch.float32) % 5 - 2.0) * 5e3
    out = ops.channel_sum(g.to(device))
    case = "channel_sum rows=%d C=%d" % (rows, c)
    hold_fp64_sum(case, "sum", out, g.double().sum(0), rows, g.double().abs().sum(0))
    hold(case, "sum", out, g.double().sum(0), g.sum(0))


def check_channel_sum_paths(device):
    """sum_direct_max() = 4096: the direct kernel never touches the workspace, reduce + finalize writes its partial sums
    there -- so the switch between them shows in a poisoned workspace."""
    lib = _lib.load()
    for rows, direct in ((SUM_DIRECT_MAX, True), (SUM_DIRECT_MAX + 1, False)):
        g = torch.ones(rows, 16, device=device)
        out = torch.empty(16, device=device)
        ws = torch.full((int(lib.cfun_channel_sum_workspace_bytes(rows, 16)),), 0xA5, dtype=torch.uint8, device=device)
        assert lib.cfun_channel_sum(ops.ptr(g), ops.ptr(out), rows, 16, ops.ptr(ws), ws.numel(), ops.stream(g)) == CFUN_OK
        assert bool((out == float(rows)).all())
        assert bool((ws == 0xA5).all()) == direct, "rows=%d: expected the %s path" % (rows, "direct" if direct else "reduce")


# ------------------------------------------------------------------------------------------ InstanceNorm + LeakyReLU
KINK_SHARE_CAP = 1e-3      # at most this share of a case's elements may sit in the LeakyReLU kink band (see norm_keep)


def norm_ref(x, dy, dtype):
    """LeakyReLU(InstanceNorm(x)) of x [N, V, C] (biased variance, eps 1e-5) and its autograd gradient, in ``dtype``; written
    out (not F.instance_norm) so that V = 1 is defined: var = 0, rstd = eps^-1/2, y = 0."""
    xr = x.detach().clone().to(dtype).requires_grad_(True)
    mean = xr.mean(1, keepdim=True)
    var = xr.var(1, unbiased=False, keepdim=True)
    rstd = torch.rsqrt(var + EPS)
    xh = (xr - mean) * rstd
    y = F.leaky_relu(xh, SLOPE)
    y.backward(dy.to(dtype))
    stats = torch.stack([mean.detach()[:, 0], rstd.detach()[:, 0]], dim=-1)
    return y.detach(), xr.grad, stats, xh.detach()


def norm_keep(x, stats64, xh64):
    """The elements whose LeakyReLU branch is decided: all but those with 0 < |xhat64| <= 4 * 2^-24 * (|x| + |mean|) * rstd,
    in float64.  Inside that band an fp32 evaluation may legitimately land on the other side of 0 and take the other slope
    (dx changes by about 0.99 * dy * rstd).  xhat64 == 0 exactly -- a constant channel, V = 1 -- is NOT in the band: there
    every arithmetic computes an exact 0 and the derivative is the slope, as in torch."""
    mean, rstd = stats64[..., 0][:, None, :], stats64[..., 1][:, None, :]
    band = 4.0 * 2.0 ** -24 * (x.double().abs() + mean.abs()) * rstd
    a = xh64.abs()
    return ~((a > 0) & (a <= band))


def run_norm_abi(device, x, dy, add):
    """Every InstanceNorm entry of the C ABI on x, dy, add [N, V, C]: returns (stats, y, dx, dx + add); the strided forms and
    the depth-sharded pair (bwd_means + bwd_apply with the single rank's means) must reproduce them bit for bit -- they are
    the same kernels with another row stride."""
    lib = _lib.load()
    n, v, c = x.shape
    xd, dyd, addd = x.to(device), dy.to(device), add.to(device)
    st = ops.stream(xd)
    nb = int(lib.cfun_instnorm_workspace_bytes(n, v, c))
    assert nb > 0

    def ws():
        return _lib.workspace(nb, xd)

    def fresh():
        return torch.full((n, v, c), float("nan"), device=device)

    stats = torch.full((n, c, 2), float("nan"), device=device)
    w = ws()
    assert lib.cfun_instnorm_stats(ops.ptr(xd), ops.ptr(stats), n, v, c, EPS, ops.ptr(w), w.numel(), st) == CFUN_OK
    y = fresh()
    assert lib.cfun_instnorm_lrelu_fwd(ops.ptr(xd), ops.ptr(stats), ops.ptr(y), n, v, c, SLOPE, st) == CFUN_OK
    dx = fresh()
    w = ws()
    assert lib.cfun_instnorm_lrelu_bwd(ops.ptr(xd), ops.ptr(stats), ops.ptr(dyd), ops.ptr(dx), n, v, c, SLOPE, ops.ptr(w), w.numel(), st) == CFUN_OK
    dxa = fresh()
    w = ws()
    assert lib.cfun_instnorm_lrelu_bwd_add(ops.ptr(xd), ops.ptr(stats), ops.ptr(dyd), ops.ptr(addd), ops.ptr(dxa), n, v, c, c, SLOPE,
                                           ops.ptr(w), w.numel(), st) == CFUN_OK
    strides = [(c, 0)] + ([(c + 4, 0), (3 * c, 2 * c)] if c % 4 == 0 else [])
    for rs, c0 in strides:
        what = "C=%d V=%d rs=%d c0=%d" % (c, v, rs, c0)
        wide = torch.full((n, v, rs), 777.0, device=device)
        view = wide[..., c0:c0 + c]
        if rs != c:
            assert lib.cfun_instnorm_lrelu_fwd_strided(ops.ptr(xd), ops.ptr(stats), ops.ptr_raw(view), n, v, c, rs, SLOPE, st) == CFUN_OK
            assert bits_equal(view.contiguous(), y), what + ": strided forward differs from the dense one"
            view.fill_(777.0)
            assert bool((wide == 777.0).all()), what + ": strided forward wrote outside the channel range"
        view.copy_(dyd)
        d2 = fresh()
        w = ws()
        assert lib.cfun_instnorm_lrelu_bwd_strided(ops.ptr(xd), ops.ptr(stats), ops.ptr_raw(view), ops.ptr(d2), n, v, c, rs, SLOPE,
                                                   ops.ptr(w), w.numel(), st) == CFUN_OK
        assert bits_equal(d2, dx), what + ": strided backward differs from the dense one"
        means = torch.full((n, c, 2), float("nan"), device=device)
        d3 = fresh()
        w = ws()
        assert lib.cfun_instnorm_bwd_means(ops.ptr(xd), ops.ptr(stats), ops.ptr_raw(view), ops.ptr(means), n, v, c, rs, SLOPE, ops.ptr(w),
                                           w.numel(), st) == CFUN_OK
        assert lib.cfun_instnorm_lrelu_bwd_apply(ops.ptr(xd), ops.ptr(stats), ops.ptr(means), ops.ptr_raw(view), ops.ptr(d3), n, v, c, rs,
                                                 SLOPE, st) == CFUN_OK
        assert bits_equal(d3, dx), what + ": bwd_means + bwd_apply differ from the one-call backward"
    return stats, y, dx, dxa


def check_norm(device, case, x, dy, add, through_ops=True):
    """x, dy, add [N, V, C] fp32.  y, dx, dx + add per (n, channel) under the rule (dx outside the kink band, whose share is
    capped); the mean under the fp64-sum contract, mean and rstd each on its own under the rule."""
    n, v, c = x.shape
    y64, dx64, st64, xh64 = norm_ref(x, dy, torch.float64)
    y32, dx32, st32, _ = norm_ref(x, dy, torch.float32)
    stats, y, dx, dxa = run_norm_abi(device, x, dy, add)
    keep = norm_keep(x, st64, xh64)
    share = 1.0 - float(keep.double().mean())
    assert share <= KINK_SHARE_CAP, "%s: %.3e of the elements sit in the kink band (cap %.0e)" % (case, share, KINK_SHARE_CAP)
    hold_fp64_sum(case, "mean", stats[..., 0], st64[..., 0], v, x.double().abs().mean(1))
    hold(case, "mean", stats[..., 0], st64[..., 0], st32[..., 0], seg=1)
    hold(case, "rstd", stats[..., 1], st64[..., 1], st32[..., 1], seg=1)
    hold(case, "y", y, y64, y32, seg="nc")
    hold(case, "dx", dx, dx64, dx32, seg="nc", keep=keep)
    hold(case, "dx + add", dxa, dx64 + add.double(), dx32 + add, seg="nc", keep=keep)
    if through_ops and v > 1:          # (the wrapper refuses V = 1 as InstanceNorm3d does when training)
        xd = x.detach().clone().to(device).requires_grad_(True)
        yo = ops.instnorm_lrelu(xd.view(n, v, 1, 1, c))
        yo.backward(dy.to(device).view(n, v, 1, 1, c))
        assert bits_equal(yo.view(n, v, c), y) and bits_equal(xd.grad, dx), case + ": ops.instnorm_lrelu differs from the C ABI calls"


NORM_GEOMETRY = [(2, v, c) for c in (1, 255, 1024) for v in (1, 2, 17)] + [(1025, 16, 4), (1025, 16, 3)]
# C = 1: one scalar group, 256 voxel lanes; C = 255: 255 scalar groups, ONE lane and one idle thread; C = 1024: 256 float4
# groups, one lane.  N = 1025 > 1024: reduce_plan's want = ceil(1024 / N) becomes 1 block per sample.


def check_norm_geometry(device, n, v, c, seed=110):
    gen = _gen(seed + 1000 * n + 10 * v + c)
    # V = 2 is ill-conditioned at unit spread whatever computes it: xhat = +-(1 - eps * rstd^2)^1/2, so dx = rstd * (gn1 - gn2) / 2 *
    # eps * rstd^2 is what is left after terms 1 / (eps * rstd^2) = 2e5 times larger cancel -- rounding noise in ANY fp32
    # evaluation (torch's own is 4e-4 ... 1e-2 from float64 there), and two elements per channel are no measure of noise.
    # These cases are about the launch, so the spread is eps^1/2: eps * rstd^2 is about 1/2 and nothing cancels.
    spread = 2.0 if v != 2 else EPS ** 0.5
    x = randn(gen, n, v, c) * spread + randn(gen, 1, 1, c)
    check_norm(device, "norm geometry N=%d V=%d C=%d" % (n, v, c), x, randn(gen, n, v, c), randn(gen, n, v, c))


# ========================================================================================== B. value range
NORM_RANGE_SHAPES = {"c8": (2, (16, 16, 16), 8), "c3": (2, (16, 16, 16), 3)}
# per (n, channel), mixed within one tensor: (kind, mean, sigma); mean / sigma in {0, 10, 1e2, 1e3} (1e4 would put 4e-3 of the
# elements into the kink band, above the cap), a constant channel (a value with few mantissa bits: every sum of it is exact
# in fp32 and fp64, so xhat is exactly 0 in every arithmetic) and a channel constant except for a single voxel
NORM_KINDS = (("ratio", 1e3, 1.0), ("const", 2.5, 0.0), ("single", 2.5, 0.0), ("ratio", 0.0, 1.0), ("ratio", 50.0, 0.5),
              ("ratio", 10.0, 1.0), ("ratio", -20.0, 0.02), ("ratio", 1e3, 1e2))


def check_norm_range(device, n, dhw, c, seed=120):
    gen = _gen(seed + c)
    v = dhw[0] * dhw[1] * dhw[2]
    x = torch.empty(n, v, c)
    for i in range(n):
        for j in range(c):
            kind, mean, sigma = NORM_KINDS[(i * 3 + j) % len(NORM_KINDS)]
            if kind == "ratio":
                x[i, :, j] = mean + sigma * randn(gen, v)
            else:
                x[i, :, j] = mean
                if kind == "single":
                    x[i, v // 3, j] = mean + 1.5
    dy = randn(gen, n, v, c)
    dy[..., c - 1] = 0.0                         # one gradient channel identically zero
    check_norm(device, "norm range %s C=%d" % (dhw, c), x, dy, randn(gen, n, v, c))


def maxpool_value_cases(seed=130):
    """(name, x, gy): a constant input (every window a full tie), a ReLU-sparse one (most windows tie at 0, some hold one
    positive value late in the scan), NaNs (one in a window, two in a window, a whole window)."""
    gen = _gen(seed)
    shape, oshape = (2, 4, 6, 8, 5), (2, 2, 3, 4, 5)
    out = [("constant", torch.full(shape, 1.25), randn(gen, *oshape)),
           ("relu_sparse", F.relu(randn(gen, *shape) - 1.0), randn(gen, *oshape)),
           ("all_zero_signed", torch.zeros(shape) * torch.where(randn(gen, *shape) > 0, 1.0, -1.0), randn(gen, *oshape))]
    x = randn(gen, *shape)
    x[0, 1, 2, 3, 0] = float("nan")                                  # one NaN in a window
    x[1, 0, 0, 0, 1] = x[1, 1, 1, 0, 1] = float("nan")               # two in one window: torch keeps the LAST
    x[1, 2:4, 4:6, 6:8, 4] = float("nan")                            # a whole window
    out.append(("nan", x, randn(gen, *oshape)))
    return out


def check_maxpool_values(device):
    for name, x, gy in maxpool_value_cases():
        check_maxpool_exact(device, x, gy, "maxpool " + name)


# ========================================================================================== alignment contract
def _refused(rc_want, call, outs, what):
    for o in outs:
        o.fill_(777.0)
    rc = call()
    assert rc == rc_want, "%s: returned %d, expected %d" % (what, rc, rc_want)
    for o in outs:
        assert bool((o == 777.0).all()), what + ": refused the call but wrote its output"


def check_alignment_contract(device, seed=140):
    """Every entry of elementwise.hip that tests cfun_aligned16, with each pointer in turn 4 bytes past a 16-byte boundary:
    CFUN_EALIGN and an untouched output from those that need float4 accesses (C % 4 == 0), the right answer from the forms
    that promise a scalar path (C % 4 != 0; cfun_lrelu_fwd / _bwd / cfun_add are in check_flat_elementwise)."""
    lib = _lib.load()
    gen = _gen(seed)
    n, v, c = 2, 5, 8
    nvox = n * v

    def mis(t):         # the same values, one float past a 16-byte boundary
        return _dev_slice(t.reshape(-1), device, 1)[1].view(t.shape)

    x, dy, add = randn(gen, n, v, c), randn(gen, n, v, c), randn(gen, n, v, c)
    xa, dya, adda = x.to(device), dy.to(device), add.to(device)
    xm, dym, addm = mis(x), mis(dy), mis(add)
    outa, outm = torch.empty(n, v, c, device=device), mis(torch.empty(n, v, c))
    st = ops.stream(xa)
    P = ops.ptr
    for xs, ys, o in ((xm, None, outa), (xa, None, outm)):
        _refused(CFUN_EALIGN, lambda: lib.cfun_lrelu_fwd_strided(P(xs), P(o), nvox, c, c, c, SLOPE, st), [outa, outm], "lrelu_fwd_strided")
    for xs, ds, as_, o in ((xm, dya, adda, outa), (xa, dym, adda, outa), (xa, dya, addm, outa), (xa, dya, adda, outm)):
        _refused(CFUN_EALIGN, lambda: lib.cfun_lrelu_bwd_add(P(xs), P(ds), P(as_), P(o), nvox, c, c, SLOPE, st), [outa, outm], "lrelu_bwd_add")
        if as_ is adda:
            _refused(CFUN_EALIGN, lambda: lib.cfun_lrelu_bwd_strided(P(xs), P(ds), P(o), nvox, c, c, SLOPE, st), [outa, outm], "lrelu_bwd_strided")
    # channel sum and the statistics
    s_out = torch.empty(c, device=device)
    ws = _lib.workspace(max(int(lib.cfun_channel_sum_workspace_bytes(nvox, c)), int(lib.cfun_instnorm_workspace_bytes(n, v, c))), xa)
    _refused(CFUN_EALIGN, lambda: lib.cfun_channel_sum(P(xm), P(s_out), nvox, c, P(ws), ws.numel(), st), [s_out], "channel_sum")
    stats = torch.empty(n, c, 2, device=device)
    _refused(CFUN_EALIGN, lambda: lib.cfun_instnorm_stats(P(xm), P(stats), n, v, c, EPS, P(ws), ws.numel(), st), [stats], "instnorm_stats")
    assert lib.cfun_instnorm_stats(P(xa), P(stats), n, v, c, EPS, P(ws), ws.numel(), st) == CFUN_OK
    good = stats.clone()
    for xs, o in ((xm, outa), (xa, outm)):
        _refused(CFUN_EALIGN, lambda: lib.cfun_instnorm_lrelu_fwd_strided(P(xs), P(good), P(o), n, v, c, c, SLOPE, st), [outa, outm],
                 "instnorm_lrelu_fwd_strided")
        _refused(CFUN_EALIGN, lambda: lib.cfun_instnorm_lrelu_fwd(P(xs), P(good), P(o), n, v, c, SLOPE, st), [outa, outm], "instnorm_lrelu_fwd")
    means = torch.empty(n, c, 2, device=device)
    for xs, ds, as_, o in ((xm, dya, adda, outa), (xa, dym, adda, outa), (xa, dya, addm, outa), (xa, dya, adda, outm)):
        _refused(CFUN_EALIGN, lambda: lib.cfun_instnorm_lrelu_bwd_add(P(xs), P(good), P(ds), P(as_), P(o), n, v, c, c, SLOPE, P(ws), ws.numel(), st),
                 [outa, outm], "instnorm_lrelu_bwd_add")
        if as_ is adda:
            _refused(CFUN_EALIGN, lambda: lib.cfun_instnorm_lrelu_bwd(P(xs), P(good), P(ds), P(o), n, v, c, SLOPE, P(ws), ws.numel(), st),
                     [outa, outm], "instnorm_lrelu_bwd")
            _refused(CFUN_EALIGN, lambda: lib.cfun_instnorm_lrelu_bwd_strided(P(xs), P(good), P(ds), P(o), n, v, c, c, SLOPE, P(ws), ws.numel(), st),
                     [outa, outm], "instnorm_lrelu_bwd_strided")
            _refused(CFUN_EALIGN, lambda: lib.cfun_instnorm_lrelu_bwd_apply(P(xs), P(good), P(good), P(ds), P(o), n, v, c, c, SLOPE, st),
                     [outa, outm], "instnorm_lrelu_bwd_apply")
            if o is outa:
                _refused(CFUN_EALIGN, lambda: lib.cfun_instnorm_bwd_means(P(xs), P(good), P(ds), P(means), n, v, c, c, SLOPE, P(ws), ws.numel(), st),
                         [means], "instnorm_bwd_means")
    # upsample backward, VEC = 4
    hi = randn(gen, 1, 2, 4, 6, c)
    lo_a, lo_m = torch.empty(1, 1, 2, 3, c, device=device), mis(torch.empty(1, 1, 2, 3, c))
    for h_, l_ in ((mis(hi), lo_a), (hi.to(device), lo_m)):
        _refused(CFUN_EALIGN, lambda: lib.cfun_upsample2_bwd(P(h_), P(l_), 1, 1, 2, 3, c, st), [lo_a, lo_m], "upsample2_bwd")
    # the scalar forms (C % 4 != 0) take any 4-byte-aligned pointer: same bits as from aligned ones
    c = 3
    x, dy, add = randn(gen, n, v, c), randn(gen, n, v, c), randn(gen, n, v, c)
    res = []
    for place in (lambda t: t.to(device), mis):
        xs, ds, as_ = place(x), place(dy), place(add)
        s_out, stats = place(torch.zeros(c)), place(torch.zeros(n, c, 2))
        y, dx = place(torch.zeros(n, v, c)), place(torch.zeros(n, v, c))
        ws = _lib.workspace(max(int(lib.cfun_channel_sum_workspace_bytes(nvox, c)), int(lib.cfun_instnorm_workspace_bytes(n, v, c))), xa)
        assert lib.cfun_channel_sum(P(xs), P(s_out), nvox, c, P(ws), ws.numel(), st) == CFUN_OK
        assert lib.cfun_instnorm_stats(P(xs), P(stats), n, v, c, EPS, P(ws), ws.numel(), st) == CFUN_OK
        assert lib.cfun_instnorm_lrelu_fwd(P(xs), P(stats), P(y), n, v, c, SLOPE, st) == CFUN_OK
        assert lib.cfun_instnorm_lrelu_bwd_add(P(xs), P(stats), P(ds), P(as_), P(dx), n, v, c, c, SLOPE, P(ws), ws.numel(), st) == CFUN_OK
        hi = randn(_gen(seed + 1), 1, 2, 4, 6, c)
        his, lo = place(hi), place(torch.zeros(1, 1, 2, 3, c))
        assert lib.cfun_upsample2_bwd(P(his), P(lo), 1, 1, 2, 3, c, st) == CFUN_OK
        res.append([t.cpu().clone() for t in (s_out, stats, y, dx, lo)])
    for a, b, nm in zip(res[0], res[1], ("channel_sum", "stats", "y", "dx", "upsample lo")):
        assert bits_equal(a, b), "C = 3 %s: a misaligned pointer changes the result" % nm
    assert torch.allclose(res[0][0].double(), x.double().reshape(-1, c).sum(0), rtol=1e-6, atol=1e-6)
    assert torch.allclose(res[0][4].double(), hi.double().view(1, 1, 2, 2, 2, 3, 2, c).sum(dim=(2, 4, 6)), rtol=1e-6, atol=1e-6)


# ========================================================================================== C. optimizer tail
SUMSQ_N = (0, 1, 255, 256, NORM_SWEEP, 2 * NORM_SWEEP + 77)


def _spread(gen, n):
    """Magnitudes over 1e-20 ... 1e18: the squares span 1e-40 ... 1e36, more than fp32 holds next to one another."""
    return randn(gen, n) * torch.pow(10.0, torch.rand(n, generator=gen, dtype=torch.float64) * 38.0 - 20.0).float()


def _block_sumsq(g):
    """What block b of k_sumsq_partials owns: the elements i with (i mod 131072) // 256 == b; (sum of squares, count)."""
    sq = g.double() ** 2
    pad = (-sq.numel()) % NORM_SWEEP
    sq = torch.cat([sq, sq.new_zeros(pad)]).reshape(-1, K_NORM_BLOCKS, K_BLOCK)
    return sq.sum(dim=(0, 2)), sq.shape[0] * K_BLOCK


def check_sumsq_norm(device, n_a, n_b, seed=150):
    """cfun_sumsq_partials on two arenas (the second one's partials at partials[512:]) + cfun_norm_finalize over all 1024:
    every fp64 partial within terms * 2^-52 of the exact sum of its block's squares, the norm within the fp64-sum contract
    carried through the square root."""
    lib = _lib.load()
    gen = _gen(seed + n_a + 3 * n_b)
    arenas = [_spread(gen, n_a), _spread(gen, n_b)]
    partials = torch.full((2 * K_NORM_BLOCKS,), float("nan"), dtype=torch.float64, device=device)
    norm = torch.full((1,), float("nan"), device=device)
    case = "sumsq n=(%d, %d)" % (n_a, n_b)
    total = 0.0
    for i, g in enumerate(arenas):
        gd = g.to(device) if g.numel() else torch.zeros(1, device=device)
        assert lib.cfun_sumsq_partials(ops.ptr(gd), g.numel(), ops.ptr(partials[i * K_NORM_BLOCKS:]), ops.stream(gd)) == CFUN_OK
        ref, terms = _block_sumsq(g) if g.numel() else (torch.zeros(K_NORM_BLOCKS, dtype=torch.float64), 1)
        got = partials[i * K_NORM_BLOCKS:(i + 1) * K_NORM_BLOCKS].cpu()
        lim = terms * 2.0 ** -52 * ref
        bad = ~((got - ref).abs() <= lim)
        assert not bool(bad.any()), ("%s arena %d: %d partial sums outside terms * 2^-52 of their fp64 value, first block %d: "
                                     "%.17g vs %.17g" % (case, i, int(bad.sum()), int(torch.nonzero(bad)[0]), float(got[bad][0]),
                                                         float(ref[bad][0])))
        total += math.fsum((g.double() ** 2).tolist()) if g.numel() else 0.0
    assert lib.cfun_norm_finalize(ops.ptr(partials), 2 * K_NORM_BLOCKS, ops.ptr(norm), ops.stream(norm)) == CFUN_OK
    ref = math.sqrt(total)
    # sqrt halves a relative error: the sum's (n + 1024) * 2^-52, then one rounding to fp32
    lim = 2.0 ** -23 * ref + 0.5 * (n_a + n_b + 2 * K_NORM_BLOCKS) * 2.0 ** -52 * ref
    got = float(norm.cpu()[0])
    REPORT.append((case, "norm", "fp64sum", 0.0, abs(got - ref) / (ref + 1e-300), 2.0 ** -23))
    assert abs(got - ref) <= lim, "%s: norm %.9g, float64 %.17g: |err| %.3e > %.3e" % (case, got, ref, abs(got - ref), lim)


SGD_N = 2 * SWEEP + 77


def _sgd_ref64(p, m, g, lr, mom, wd, max_norm, first):
    """The kernel's formula in float64: g' = g * min(1, max_norm / (|g| + 1e-6)); d = g' + wd * p; m = first ? d : mom * m + d;
    p -= lr * m."""
    coef = 1.0
    if max_norm > 0:
        coef = min(1.0, max_norm / (math.sqrt(math.fsum((g.double() ** 2).tolist())) + 1e-6))
    d = g.double() * coef + wd * p
    m = d if first else mom * m + d
    return p - lr * m, m


def _device_norm(lib, gd):
    partials = torch.zeros(K_NORM_BLOCKS, dtype=torch.float64, device=gd.device)
    norm = torch.zeros(1, device=gd.device)
    assert lib.cfun_sumsq_partials(ops.ptr(gd), gd.numel(), ops.ptr(partials), ops.stream(gd)) == CFUN_OK
    assert lib.cfun_norm_finalize(ops.ptr(partials), K_NORM_BLOCKS, ops.ptr(norm), ops.stream(gd)) == CFUN_OK
    return norm


SGD_RUNS = {
    # name: (weight decay, per step: (gradient scale, clip)); clip: None = max_norm 0 with a NULL norm pointer, "at" = max_norm
    # set to the gradient's own fp32 norm, "above" = to the next float below it (the norm a hair above max_norm), a number = that
    "wd_boundary": (1e-4, ((1.0, "at"), (1.0, "above"), (0.0, 5.0))),      # step 3: a zero gradient, coefficient 1
    "nowd_clip": (0.0, ((1.0, None), (40.0, 5.0), (1e-3, 5.0))),           # no clip; norm >> 5; norm << 5
}


def check_sgd_step(device, name, n=SGD_N, seed=160):
    """cfun_sgd_momentum_step over two sweeps and a ragged third, three steps (first_step 1, 0, 0): the kernel's formula in
    float64 is the reference, torch's own clip_grad_norm_ + SGD on the same arena gives e32; p and m after every step, whole
    and per sweep."""
    lib = _lib.load()
    wd, steps = SGD_RUNS[name]
    lr, mom = 0.01, 0.9
    gen = _gen(seed)
    p0 = randn(gen, n)
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.SGD([pt], lr=lr, momentum=mom, weight_decay=wd)
    p64, m64 = p0.double(), torch.zeros(n, dtype=torch.float64)
    # (the momentum starts as NaN: first_step = 1 must overwrite it without reading it -- zeros would make the two branches of
    # `first ? d : momentum * m + d` the same bits)
    pd, md = p0.clone().to(device), torch.full((n,), float("nan"), device=device)
    for k, (gscale, clip) in enumerate(steps):
        g = randn(gen, n) * gscale
        gd = g.to(device)
        norm = _device_norm(lib, gd)
        if clip == "at":
            max_norm = float(norm.cpu()[0])
        elif clip == "above":
            max_norm = float(np.nextafter(np.float32(float(norm.cpu()[0])), np.float32(0.0)))
        else:
            max_norm = 0.0 if clip is None else float(clip)
        assert lib.cfun_sgd_momentum_step(ops.ptr(pd), ops.ptr(gd), ops.ptr(md), n, lr, mom, wd, max_norm,
                                          None if clip is None else ops.ptr(norm), 1 if k == 0 else 0, ops.stream(pd)) == CFUN_OK
        p64, m64 = _sgd_ref64(p64, m64, g, lr, mom, wd, max_norm, k == 0)
        pt.grad = g.clone()
        if clip is not None:
            torch.nn.utils.clip_grad_norm_([pt], max_norm)
        opt.step()
        m32 = opt.state[pt]["momentum_buffer"]
        case = "sgd %s step %d" % (name, k)
        hold(case, "p", pd, p64, pt.detach(), seg=SWEEP)
        hold(case, "m", md, m64, m32, seg=SWEEP)
    # a clip without a norm to clip by is an argument error, and nothing moves
    before = pd.clone()
    assert lib.cfun_sgd_momentum_step(ops.ptr(pd), ops.ptr(gd), ops.ptr(md), n, lr, mom, wd, 5.0, None, 0, ops.stream(pd)) == CFUN_EINVAL
    assert torch.equal(pd, before)


def check_flat_sgd_over_cap(device, seed=170):
    """FlatSGD with one parameter of 1.1 M elements among small ones in ONE arena (past the 2048-block cap of the update launch
    and the 131 072-element sweep of the sum of squares), three steps against torch; per parameter and, inside the large one,
    per sweep of the arena's launch."""
    from cfun_amd import optim
    gen = _gen(seed)
    shapes = [(7, 3), (1100, 1000), (5,), (16, 8, 1, 1, 1)]
    assert shapes[1][0] * shapes[1][1] > 2 * SWEEP
    ref = [randn(gen, *s).requires_grad_(True) for s in shapes]
    mine = [r.detach().clone().to(device).requires_grad_(True) for r in ref]
    opt_ref = torch.optim.SGD([{"params": ref, "weight_decay": 1e-4}], lr=0.01, momentum=0.9)
    opt = optim.FlatSGD([("w%d" % i, p) for i, p in enumerate(mine)], lr=0.01, momentum=0.9, weight_decay=1e-4, clip_norm=5.0,
                        bucket_bytes=64 << 20)
    assert len(opt.param_arenas) == 1
    for m in opt.momentum_arenas:          # the first step must not read the momentum it initialises (see check_sgd_step)
        m.fill_(float("nan"))
    offsets = {id(p): off for p, _, off in opt._slots}
    p64 = [r.detach().double() for r in ref]
    m64 = [torch.zeros_like(q) for q in p64]
    for k, gscale in enumerate((0.02, 1e-4, 1.0)):        # norm >> 5 (clipped), << 5, >> 5
        grads = [randn(gen, *s) * gscale for s in shapes]
        opt_ref.zero_grad()
        opt.zero_grad()
        for r, g in zip(ref, grads):
            r.grad = g.clone()
        torch.autograd.backward([(m * g.to(device)).sum() for m, g in zip(mine, grads)])
        norm64 = math.sqrt(math.fsum(v for g in grads for v in (g.double() ** 2).reshape(-1).tolist()))
        total = torch.nn.utils.clip_grad_norm_(ref, 5.0)
        opt_ref.step()
        opt.step()
        assert abs(float(opt.grad_norm[0]) - norm64) <= 2.0 ** -22 * norm64, (float(opt.grad_norm[0]), norm64, float(total))
        coef = min(1.0, 5.0 / (norm64 + 1e-6))
        for i, (r, m) in enumerate(zip(ref, mine)):
            d = grads[i].double() * coef + 1e-4 * p64[i]
            m64[i] = d if k == 0 else 0.9 * m64[i] + d
            p64[i] = p64[i] - 0.01 * m64[i]
            hold("FlatSGD over the cap, step %d" % k, "w%d %s" % (i, tuple(shapes[i])), m.detach(), p64[i], r.detach(), seg=SWEEP,
                 start=offsets[id(m)])


# ========================================================================================== D. mask losses, trained-looking inputs
MASK_RANGE_SHAPES = {"c8": (2, 8, 9, 12, 17), "c3": (1, 3, 12, 6, 10)}        # (n, C, D, H, W)
MASK_RANGE_SIGMAS = (15.0, 40.0)
NAN_SHARE_CAP = 0.10           # at most this share of the voxels may carry a NaN in torch's own fp32 gradient (flat case)
# Random logits at sigma = 40 saturate: some Sobel responses are exact zeros in fp32 only (edge_ambiguous_voxels), and each takes
# its 27 inputs out of the gradient comparison.  That share is a property of the inputs, not of any kernel (10.05 % of the
# voxels at C = 8, sigma = 40, none in the other three cases); the cap sits just above that share.  In check_edge_flat_logits the
# set holds the whole planted region: there the 10 % cap on torch's own NaN share is what bounds the exclusion.
AMBIGUOUS_SHARE_CAP = 0.12
LITS_WEIGHTS = (1.0, 1.0, 100.0)


def _onehot(lab, c):
    return torch.stack([(lab == k) for k in range(c)], dim=1).double()


def _mask_refs(lg, lab, dtype, lits=False):
    """CE, softmax, edge loss and their gradients w.r.t. the logits [n, C, D, H, W] in ``dtype``, by torch autograd."""
    c = lg.shape[1]
    x = lg.detach().clone().to(dtype).requires_grad_(True)
    onehot = _onehot(lab, c)
    ce = F.cross_entropy(x, lab)
    probs = torch.softmax(x, dim=1)
    edge = orc.edge_loss(onehot, probs)[0]
    out = {"ce": ce.detach(), "probs": probs.detach(), "edge": edge.detach(),
           "dce": torch.autograd.grad(ce, x, retain_graph=True)[0], "dedge": torch.autograd.grad(edge, x, retain_graph=True)[0]}
    out["dboth"] = 0.7 * out["dce"] + 1.3 * out["dedge"]
    if lits:
        wce = F.cross_entropy(x, lab, weight=torch.tensor(LITS_WEIGHTS, dtype=dtype))
        raw = orc.edge_loss_raw(onehot, probs)[0]
        out.update(wce=wce.detach(), raw=raw.detach(), dwce=torch.autograd.grad(wce, x, retain_graph=True)[0],
                   draw=torch.autograd.grad(raw, x)[0])
    return out


def _ncdhw(t):
    return t.detach().permute(0, 4, 1, 2, 3)


def edge_ambiguous_voxels(probs64):
    """Voxels [n, 1, D, H, W] whose edge-loss gradient an fp32 evaluation may legitimately turn into NaN / inf: the inputs of
    every Sobel output whose response (p0, p1) may come out as exactly (0, 0) in fp32 -- the square root's derivative there is
    inf, times 0 -- although it is not zero in float64.  Saturated probabilities do that: 1 + 1e-20 is 1 in fp32, and whether
    the ones then cancel depends on the order of the 18 additions.  Criterion, in float64 and from the number format alone:
    |p_j| <= 24 * 2^-24 * sum|w_i p_i| for j = 0 and 1 (17 roundings of the sum plus a few ulp on each probability), or the
    sum of squares at or below 2^-125 (fp32 squares underflow; v_rsq_f32 takes a denormal for 0).  All classes of such a voxel
    are taken out (the softmax backward mixes them); the caller caps the share and requires torch's own fp32 gradient to be
    finite everywhere else, which keeps the criterion honest."""
    n, c, d, h, w = probs64.shape
    k = orc.sobel_stack().double()[:2]
    x = probs64[:, 1:].reshape(n * (c - 1), 1, d, h, w)
    p, s = F.conv3d(x, k), F.conv3d(x.abs(), k.abs())
    tau = 24.0 * 2.0 ** -24 * s
    amb = ((p.abs() <= tau).all(dim=1)) | (2.0 * p[:, 0] ** 2 + p[:, 1] ** 2 <= 2.0 ** -125)
    spread = F.max_pool3d(F.pad(amb.double()[:, None], (2, 2, 2, 2, 2, 2)), 3, 1)[:, 0]
    return spread.reshape(n, c - 1, d, h, w).amax(dim=1, keepdim=True) > 0


def _hold_finite(case, what, got, r64, r32, ambiguous=None):
    """The rule wherever torch's fp32 gradient (and the float64 one) is finite; there the kernel must be finite too (a NaN
    of the kernel inside the compared set fails the comparison).  ``ambiguous``: see edge_ambiguous_voxels."""
    keep = torch.isfinite(r32) & torch.isfinite(r64)
    if ambiguous is not None:
        assert bool(keep[~ambiguous.expand_as(keep)].all()), "%s %s: torch's own gradient is not finite outside the ambiguous set" % (case, what)
        keep = keep & ~ambiguous
    hold(case, what, got, torch.nan_to_num(r64), torch.nan_to_num(r32), keep=keep)
    return keep


def run_mask_forms(device, case, lg, labels, r64, r32, lits=False):
    """Every form of the mask losses on logits lg [n, C, D, H, W] / labels uint8 [n, D, H, W] against the two references."""
    c = lg.shape[1]
    ld = lg.permute(0, 2, 3, 4, 1).contiguous().to(device).requires_grad_(True)
    labd = labels.to(device)
    amb = edge_ambiguous_voxels(r64["probs"])
    share = float(amb.double().mean())
    assert share <= AMBIGUOUS_SHARE_CAP, "%s: %.3f of the voxels may turn NaN in fp32 (cap %.2f)" % (case, share, AMBIGUOUS_SHARE_CAP)

    def scalar(what, got, key):
        assert bool(torch.isfinite(got.detach()).all()), "%s %s: not finite" % (case, what)
        hold(case, what, got.reshape(1), r64[key].reshape(1), r32[key].reshape(1))

    # the separate kernels
    ce = ops.mask_cross_entropy(ld, labd)
    ce.backward()
    scalar("CE", ce, "ce")
    _hold_finite(case, "dCE/dlogits", _ncdhw(ld.grad), r64["dce"], r32["dce"])
    ld.grad = None
    probs = ops.softmax_channels(ld)
    hold(case, "softmax", _ncdhw(probs), r64["probs"], r32["probs"])
    el = ops.edge_loss(probs, labd)
    el.backward()
    scalar("edge", el, "edge")
    _hold_finite(case, "dEdge/dlogits", _ncdhw(ld.grad), r64["dedge"], r32["dedge"], amb)
    ld.grad = None
    # one backward for both (cfun_mask_losses_bwd_saved)
    ce2, el2 = ops.mask_losses(ld, ops.softmax_channels(ld), labd)
    scalar("mask_losses CE", ce2, "ce")
    scalar("mask_losses edge", el2, "edge")
    (0.7 * ce2 + 1.3 * el2).backward()
    _hold_finite(case, "mask_losses d/dlogits", _ncdhw(ld.grad), r64["dboth"], r32["dboth"], amb)
    ld.grad = None
    # one pass each way (cfun_mask_fused_fwd / _bwd: __expf / __logf on the device)
    if ops.mask_losses_fused_supported(ld):
        ce3, el3, p3 = ops.mask_losses_fused(ld, labd)
        scalar("fused CE", ce3, "ce")
        scalar("fused edge", el3, "edge")
        hold(case, "fused softmax", _ncdhw(p3), r64["probs"], r32["probs"])
        (0.7 * ce3 + 1.3 * el3).backward()
        _hold_finite(case, "fused d/dlogits", _ncdhw(ld.grad), r64["dboth"], r32["dboth"], amb)
        ld.grad = None
    else:
        assert c not in (3, 8), "the fused mask losses must take C = %d" % c
    if lits:      # the LiTS fork: class-weighted CE, MSE on the raw Sobel responses
        wce = ops.mask_cross_entropy(ld, labd, weight=np.asarray(LITS_WEIGHTS, dtype=np.float32))
        wce.backward()
        scalar("weighted CE", wce, "wce")
        _hold_finite(case, "weighted dCE/dlogits", _ncdhw(ld.grad), r64["dwce"], r32["dwce"])
        ld.grad = None
        raw = ops.edge_loss_raw(ops.softmax_channels(ld), labd)
        raw.backward()
        scalar("raw-Sobel edge", raw, "raw")
        _hold_finite(case, "raw-Sobel dEdge/dlogits", _ncdhw(ld.grad), r64["draw"], r32["draw"])
        ld.grad = None


def check_mask_losses_range(device, shape, sigma, seed=180):
    """Logits of a trained head: N(0, sigma^2) with sigma in {15, 40}, plus planted voxels -- all classes equal; one class
    ahead by 100 and labelled (CE = 0 to fp32); one class ahead by 100 and ANOTHER labelled (that voxel's CE is 100) -- in
    the interior, on the first and on the last voxel of the volume."""
    n, c, d, h, w = shape
    gen = _gen(seed + int(sigma) + c)
    lg = randn(gen, n, c, d, h, w) * sigma
    lab = torch.randint(0, c, (n, d, h, w), generator=gen, dtype=torch.int64)
    spots = [(0, 0, 0, 0), (0, 1, 2, 3), (0, d // 2, h // 2, w // 2), (n - 1, d - 1, h - 1, w - 1), (n - 1, d - 2, 1, w - 2),
             (n - 1, 3, h - 1, 0)]
    for i, (s, z, y, x) in enumerate(spots):
        kind = i % 3
        lg[s, :, z, y, x] = float(i) - 2.5
        if kind:
            lead = (i + 1) % c
            lg[s, lead, z, y, x] += 100.0
            lab[s, z, y, x] = lead if kind == 1 else (lead + 1) % c
    lits = c == 3
    r64, r32 = _mask_refs(lg, lab, torch.float64, lits), _mask_refs(lg, lab, torch.float32, lits)
    run_mask_forms(device, "mask range C=%d sigma=%g" % (c, sigma), lg, lab.to(torch.uint8), r64, r32, lits)


FLAT_SHAPE = (2, 8, 9, 12, 17)
# 5x5x5 blocks (sample, z0, y0, x0, classes held constant there, labels flat over the block?): one in the interior, one in the
# volume's corner; two classes each at the same voxels, so that torch's NaN region is 2 * 125 of 3 672 voxels (6.8 %)
FLAT_BLOCKS = ((0, 2, 3, 5, (2, 3), True), (0, 0, 0, 12, (1, 5), False))


def _nan_voxel_share(g):          # g [n, C, D, H, W]
    return float(torch.isnan(g).any(dim=1).double().mean())


def check_edge_flat_probs(device, seed=190):
    """The edge loss on a prediction that is exactly flat in places: probabilities that are multiples of 1/256 (every Sobel
    sum is then exact in fp32 and fp64 in any order, so "exactly zero" means the same in the kernel and in the references),
    constant over the planted blocks.  There sqrt'(0) makes torch's gradient NaN; the kernels skip zero-weight taps, so
    their NaN set is smaller: no equality of the sets, but wherever torch fp32 is finite the kernel is finite and within
    the rule.  The forward loss is finite and within the rule."""
    n, c, d, h, w = FLAT_SHAPE
    gen = _gen(seed)
    probs = torch.randint(0, 257, (n, c, d, h, w), generator=gen).float() / 256.0
    lab = torch.randint(0, c, (n, d, h, w), generator=gen, dtype=torch.int64)
    for s, z0, y0, x0, classes, flat in FLAT_BLOCKS:
        for k in classes:
            probs[s, k, z0:z0 + 5, y0:y0 + 5, x0:x0 + 5] = (32.0 + 16.0 * k) / 256.0
        if flat:
            lab[s, z0:z0 + 5, y0:y0 + 5, x0:x0 + 5] = classes[0]
    lg = randn(gen, n, c, d, h, w)
    onehot = _onehot(lab, c)
    nvox = n * d * h * w

    def ref(dtype):
        p = probs.detach().clone().to(dtype).requires_grad_(True)
        e = orc.edge_loss(onehot, p)[0]
        dp = torch.autograd.grad(e, p)[0]
        # what cfun_mask_losses_bwd_saved documents: 0.7 * dCE + 1.3 * the edge gradient carried through the softmax backward
        # at the GIVEN probabilities
        both = 0.7 * (p.detach() - onehot.to(dtype)) / nvox + 1.3 * p.detach() * (dp - (dp * p.detach()).sum(1, keepdim=True))
        return e.detach(), dp, both

    e64, dp64, both64 = ref(torch.float64)
    e32, dp32, both32 = ref(torch.float32)
    share = _nan_voxel_share(dp32)
    assert 0.0 < share <= NAN_SHARE_CAP, "torch's own NaN share %.3f (cap %.2f): move the blocks" % (share, NAN_SHARE_CAP)
    assert torch.equal(torch.isnan(dp32), torch.isnan(dp64)), "exactly zero must mean the same in fp32 and float64"
    case = "edge flat probs"
    pd = probs.detach().permute(0, 2, 3, 4, 1).contiguous().to(device).requires_grad_(True)
    labd = lab.to(torch.uint8).to(device)
    el = ops.edge_loss(pd, labd)
    assert bool(torch.isfinite(el.detach())), case + ": the forward loss is not finite"
    hold(case, "edge", el.reshape(1), e64.reshape(1), e32.reshape(1))
    el.backward()
    keep = _hold_finite(case, "dEdge/dprobs", _ncdhw(pd.grad), dp64, dp32)
    assert float(keep.double().mean()) >= 1.0 - NAN_SHARE_CAP
    ld = lg.permute(0, 2, 3, 4, 1).contiguous().to(device).requires_grad_(True)
    ce2, el2 = ops.mask_losses(ld, pd.detach(), labd)
    hold(case, "mask_losses edge", el2.reshape(1), e64.reshape(1), e32.reshape(1))
    (0.7 * ce2 + 1.3 * el2).backward()
    _hold_finite(case, "mask_losses d/dlogits", _ncdhw(ld.grad), both64, both32)


def check_edge_flat_logits(device, seed=191):
    """The same through the logits, for the forms that compute their own softmax (mask_losses_fused among them): inside the
    blocks one class leads by 1000, so its probability is exactly 1 and the others' exactly 0 in fp32 AND float64
    (exp(-1000) underflows in both)."""
    n, c, d, h, w = FLAT_SHAPE
    gen = _gen(seed)
    lg = randn(gen, n, c, d, h, w) * 3.0
    lab = torch.randint(0, c, (n, d, h, w), generator=gen, dtype=torch.int64)
    for s, z0, y0, x0, classes, flat in FLAT_BLOCKS:
        lg[s, classes[0], z0:z0 + 5, y0:y0 + 5, x0:x0 + 5] += 1000.0
        if flat:
            lab[s, z0:z0 + 5, y0:y0 + 5, x0:x0 + 5] = classes[0]
    r64, r32 = _mask_refs(lg, lab, torch.float64), _mask_refs(lg, lab, torch.float32)
    share = _nan_voxel_share(r32["dedge"])
    assert 0.0 < share <= NAN_SHARE_CAP, "torch's own NaN share %.3f (cap %.2f): move the blocks" % (share, NAN_SHARE_CAP)
    run_mask_forms(device, "edge flat logits", lg, lab.to(torch.uint8), r64, r32)
