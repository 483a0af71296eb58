"""Cases of the heart sample path (cfun_amd.sample.resize_rotate_box / make_sample_heart, cfun_amd.native.mold_inputs_heart /
detect_heart; k_heart_gather, k_heart_finish and k_heart_apply in cfun_amd/csrc/sample_heart.hip) shared by
test_sample_heart_emu.py and test_sample_heart_gpu.py: the device against tests/sample_heart_ref.py.  Both sides run the header's
double operations in the header's order, so the un-normalised image, the labels, both boxes and the flag must be equal bit for
bit.  Only the ORDER of the z-score's two sums is the kernel's own: mean and variance are held to the worst-case bound of a double
sum of N terms (include/cfun_sample_heart.h, step 7), and the normalised image twice -- bit for bit against the kernel's own
statistics, and within that bound of the float64 z-score."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import guard
import sample_heart_ref as hr
import sample_ref as sr
from conftest import ROOT

EINVAL, EWORKSPACE = -1, -2
INT16, FLOAT32, FLOAT64 = 0, 1, 2
ELEM = {np.dtype(np.int16): INT16, np.dtype(np.float32): FLOAT32, np.dtype(np.float64): FLOAT64}
LABEL = {np.dtype(np.int8): 0, np.dtype(np.uint8): 1, np.dtype(np.int16): 2, np.dtype(np.int32): 3}


def tile_constants():
    """The tile constants as cfun_amd/csrc/sample_heart.hip states them; the shapes below are derived from these values."""
    txt = open(os.path.join(ROOT, "cfun_amd", "csrc", "sample_heart.hip")).read()
    m = re.search(r"constexpr int kHY = (\d+), kHX = (\d+), kHZ = (\d+), kHPitch = (\d+);", txt)
    assert m, "sample_heart.hip no longer states its tile constants in one line"
    return tuple(int(v) for v in m.groups())


HY, HX, HZ, HPITCH = tile_constants()
assert (HY, HX, HZ, HPITCH) == (64, 64, 2, 65), "the heart tile changed: re-derive the sweeps below from the new constants"
# either side of the tile and of the 4-wide store path: 1, 3 (scalar stores), 4 (one quad), 63, 64 (16-byte stores), 65 (two
# tiles, scalar), 68 (two tiles, 16-byte stores, a ragged second tile)
EDGE = [1, 3, 4, HX - 1, HX, HX + 1, HX + 4]
D_OUT = [1, HZ - 1, HZ, HZ + 1, 2 * HZ + 1]
# (source, output) as (H, W, D)
W_CASES = [((6, 40, 5), (5, w, 3)) for w in EDGE]
H_CASES = [((40, 6, 5), (h, 8, 3)) for h in EDGE]
D_CASES = [((6, 7, 9), (5, 8, d)) for d in sorted(set(D_OUT))]
# n / R below, at and above 1 on each axis separately (the other two axes keep n == R)
RATIO_CASES = [(tuple(n if k == ax else 9 for k in range(3)), tuple(20 if k == ax else 9 for k in range(3)))
               for ax in range(3) for n in (14, 20, 33)]
# 0, +-20 (the loader's range), two inside it, 45 and 90 on a non-square slice (whole corners leave), 180
ANGLES = [None, 0, 20, -20, 7, -13, 45, 90, 180]


def _rng(seed):
    return np.random.default_rng(seed)


def hu(shape, seed, dtype=np.int16):
    rng = _rng(seed)
    if np.dtype(dtype) == np.int16:
        return rng.integers(-1024, 1500, shape).astype(np.int16)
    return rng.normal(100.0, 350.0, shape).astype(dtype)


def blob(shape, seed, dtype=np.int16, kind="blob"):
    rng = _rng(seed)
    mask = np.zeros(shape, dtype)
    if kind == "blob":
        lo = [n // 4 for n in shape]
        hi = [max(l + 1, n - n // 5) for l, n in zip(lo, shape)]
        mask[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = rng.integers(0, 3, [b - a for a, b in zip(lo, hi)])
    elif kind == "full":
        mask[:] = rng.integers(1, 100, shape)
    elif kind == "plane":
        mask[1:-1, 1:-1, shape[2] // 2] = 2
    return mask


def fortran(arr, device):
    """The array on the device with H fastest: what nifti.load's reshape(order='F') gives."""
    t = torch.from_numpy(np.ascontiguousarray(arr.transpose(2, 1, 0))).to(device).permute(2, 1, 0)
    assert t.stride()[0] == 1 or arr.shape[0] == 1
    return t


def _bits(t):
    return t.cpu().view(torch.int32)


def check_zscore(s, z, stats, what=""):
    """s: the kernel's un-normalised float32 output, z: its normalised one, stats: the kernel's (mean, std).  The header's bounds,
    in float64 of ``s``: |mean - m64| <= N 2^-52 mean|s|, |var - v64| <= 4 N 2^-52 mean(s^2); z == float32((s - mean_k) / std_k)
    bit for bit; |z - z64| <= ulp32(z64) + N 2^-52 mean|s| / std."""
    s64 = s.cpu().numpy().astype(np.float64).reshape(-1)
    zk = z.cpu().numpy().reshape(-1)
    mean_k, std_k = [float(v) for v in stats.cpu()]
    n = s64.size
    if np.isnan(s64).any():
        assert np.isnan(zk).all() and np.isnan(mean_k) and np.isnan(std_k), what
        return
    if not s64.any():                                                         # the reference's 0 / 0
        assert np.isnan(zk).all() and mean_k == 0.0 and std_k == 0.0, what
        return
    m64, v64 = s64.mean(), s64.var()
    mabs, msq = np.abs(s64).mean(), (s64 * s64).mean()
    eps = n * 2.0 ** -52
    print("%s N %d: |mean - m64| %.3e (bound %.3e), |var - v64| %.3e (bound %.3e)"
          % (what, n, abs(mean_k - m64), eps * mabs, abs(std_k * std_k - v64), 4 * eps * msq))
    assert abs(mean_k - m64) <= eps * mabs, what
    assert abs(std_k * std_k - v64) <= 4 * eps * msq, what
    with np.errstate(invalid="ignore", divide="ignore"):
        own = ((s64 - mean_k) / std_k).astype(np.float32)
        z64 = (s64 - m64) / np.sqrt(v64)
    assert np.array_equal(zk.view(np.int32), own.view(np.int32)), what + ": normalised image against the kernel's own statistics"
    if v64 > 0:
        tol = np.spacing(np.abs(z64).astype(np.float32)).astype(np.float64) + eps * mabs / np.sqrt(v64)
        err = np.abs(zk.astype(np.float64) - z64)
        print("%s: worst |z - z64| / bound %.3f" % (what, float((err / tol).max())))
        assert (err <= tol).all(), what


def compare(got, want, what=""):
    img, lab, raw, box, empty = got[:5]
    r_img, r_lab, r_raw, r_box, r_empty = want
    assert img.dtype == torch.float32 and tuple(img.shape) == r_img.shape
    diff = _bits(img) != torch.from_numpy(r_img).view(torch.int32)
    assert not diff.any(), "image bits, %s: %d of %d differ" % (what, int(diff.sum()), diff.numel())
    if r_lab is None:
        assert lab is None and raw is None and box is None and empty is None
        return
    assert lab.dtype == torch.uint8 and raw.dtype == box.dtype == empty.dtype == torch.int32
    assert torch.equal(lab.cpu(), torch.from_numpy(r_lab)), "labels, " + what
    assert raw.cpu().tolist() == r_raw.tolist() and box.cpu().tolist() == r_box.tolist(), (what, raw, r_raw, box, r_box)
    assert empty.cpu().tolist() == [r_empty], what


def check_case(device, src, mask, out, angle=None, clip=True, truncate=None, t_image=None, t_mask=None, zs=True):
    """src / mask: numpy [H,W,D]; t_image / t_mask: the (possibly strided) device views holding the same values (default: the
    loader's Fortran order).  The pass without the z-score against the restatement, then with it against ``check_zscore``."""
    from cfun_amd import sample
    ti = fortran(src, device) if t_image is None else t_image
    tm = None if mask is None else (fortran(mask, device) if t_mask is None else t_mask)
    trunc = bool(np.issubdtype(src.dtype, np.integer)) if truncate is None else truncate
    what = "%s -> %s angle %r clip %r truncate %r" % (src.shape, tuple(out), angle, clip, trunc)
    got = sample.resize_rotate_box(ti, tm, out, angle, zscore=False, truncate=truncate, clip=clip)
    assert got[5] is None
    compare(got, hr.sample_heart(src, mask, out, angle, "range" if clip else None, trunc), what)
    if zs:
        gz = sample.resize_rotate_box(ti, tm, out, angle, zscore=True, truncate=truncate, clip=clip)
        check_zscore(got[0], gz[0], gz[5], what)
        if mask is not None:
            assert torch.equal(gz[1], got[1]) and torch.equal(gz[3], got[3]) and torch.equal(gz[4], got[4])
    return got[:5]


def check_sweep(device, pair):
    shape, out = pair
    src, mask = hu(shape, sum(out)), blob(shape, sum(out) + 1)
    for angle in (None, 13):
        check_case(device, src, mask, out, angle)


def check_ratios(device):
    for shape, out in RATIO_CASES:
        check_case(device, hu(shape, 30), blob(shape, 31), out, -13)


def check_extents_of_one(device):
    """n = 1 and R = 1 on every axis, and all of them at once."""
    for ax in range(3):
        n = tuple(1 if k == ax else 7 for k in range(3))
        check_case(device, hu(n, 32 + ax), blob(n, 35, kind="full"), (11, 8, 9), 7)
        check_case(device, hu((7, 8, 9), 36 + ax), blob((7, 8, 9), 39), tuple(1 if k == ax else 9 for k in range(3)), 7)
    check_case(device, hu((1, 1, 1), 40), blob((1, 1, 1), 41, kind="full"), (1, 1, 1), None)
    check_case(device, hu((1, 1, 1), 42), blob((1, 1, 1), 43, kind="full"), (6, 4, 7), -20)
    check_case(device, hu((6, 5, 4), 44), blob((6, 5, 4), 45), (1, 1, 1), 20)


def check_angles(device):
    """Every angle on a non-square slice (45 and 90 turn whole corners outside) and on an even square (90 and 180 are
    whole-pixel maps there).  Angle 0 and no rotation are bit-identical."""
    for shape, out in (((21, 18, 9), (30, 17, 5)), ((20, 20, 8), (24, 24, 6))):
        src, mask = hu(shape, 46), blob(shape, 47, kind="full")
        res = {a: check_case(device, src, mask, out, a) for a in ANGLES}
        assert all(torch.equal(p, q) for p, q in zip(res[None], res[0]))
        assert not torch.equal(res[7][0], res[None][0]) and not torch.equal(res[20][1], res[-20][1])
        corners = res[45][1].cpu()
        assert not corners[:, 0, 0].any() and not corners[:, -1, -1].any() and corners.any()


def check_dtypes(device):
    """int16, float32 and float64 images; int8, uint8, int16 and int32 labels; truncate on and off for each image type."""
    shape, out = (22, 19, 9), (29, 17, 7)
    for dt in (np.int16, np.float32, np.float64):
        src = hu(shape, 50, dt)
        for trunc in (True, False):
            check_case(device, src, blob(shape, 51), out, 13, truncate=trunc)
    src = hu(shape, 52)
    got = [check_case(device, src, blob(shape, 53).astype(dt), out, -13, zs=False) for dt in (np.int8, np.uint8, np.int16, np.int32)]
    assert all(torch.equal(got[0][1], g[1]) and torch.equal(got[0][3], g[3]) for g in got[1:])
    big = _rng(54).integers(128, 256, shape).astype(np.uint8)                   # the high bit of a byte is a value, not a sign
    check_case(device, src, big, out, 7, zs=False)
    neg = _rng(55).integers(-128, 128, shape).astype(np.int8)                   # ... and of an int8 a sign: stored, left out of the box
    check_case(device, src, neg, out, 7, zs=False)
    wide = _rng(56).integers(-300, 600, shape).astype(np.int16)                 # outside the precondition: the low 8 bits
    check_case(device, src, wide, out, 7, zs=False)
    check_case(device, src, wide.astype(np.int32), out, 7, zs=False)
    # dtypes the kernel does not read go through the wrapper's casts: a uint8 image is an integer (truncated), int64 labels
    from cfun_amd import sample
    u8 = _rng(57).integers(0, 256, shape).astype(np.uint8)
    g = sample.resize_rotate_box(torch.from_numpy(u8).to(device), torch.from_numpy(blob(shape, 53).astype(np.int64)).to(device), out, 13,
                                 zscore=False)
    compare(g, hr.sample_heart(u8.astype(np.float64), blob(shape, 53), out, 13, "range", True), "uint8 image, int64 labels")


def check_orders(device):
    """Fortran order (check_case's default), C order, a sliced C-ordered view and a sliced, offset Fortran view; image and label
    in DIFFERENT orders."""
    shape, out = (22, 19, 9), (21, 24, 10)
    src, mask = hu(shape, 60), blob(shape, 61)
    tc, mc_ = torch.from_numpy(src).to(device), torch.from_numpy(mask).to(device)
    assert tc.stride()[2] == 1
    check_case(device, src, mask, out, 13, t_image=tc, t_mask=mc_)
    check_case(device, src, mask, out, 13, t_image=tc)                          # C-ordered image, Fortran label
    big_i, big_m = hu((26, 41, 14), 62), blob((26, 41, 14), 63)
    sl = (slice(2, 24), slice(1, 39, 2), slice(3, 12))
    ti, tm = torch.from_numpy(big_i).to(device)[sl], torch.from_numpy(big_m).to(device)[sl]
    assert not ti.is_contiguous() and tuple(ti.shape) == shape
    check_case(device, np.ascontiguousarray(big_i[sl]), np.ascontiguousarray(big_m[sl]), out, -20, t_image=ti, t_mask=tm)
    tf, tg = fortran(big_i, device)[sl], fortran(big_m, device)[sl]
    assert tf.stride()[0] == 1 and tf.storage_offset() > 0
    check_case(device, np.ascontiguousarray(big_i[sl]), np.ascontiguousarray(big_m[sl]), out, -20, t_image=tf, t_mask=tg)


def check_clip(device):
    """clip absent, inactive (a source with both signs: a face blended with the zero outside stays inside the range) and active
    (an all-positive source: the faces blend below the minimum) -- shown on the reference."""
    shape, out = (14, 12, 9), (19, 17, 13)
    pos = _rng(64).integers(100, 260, shape).astype(np.int16)
    both = hu(shape, 65)
    for trunc in (True, False):
        plain = hr.sample_heart(pos, None, out, None, None, trunc)[0]
        assert (plain < pos.min()).any(), "test setup: the clip does not act"
        a = check_case(device, pos, None, out, 7, clip=False, truncate=trunc)
        b = check_case(device, pos, None, out, 7, clip=True, truncate=trunc)
        assert not torch.equal(a[0], b[0]) and float(b[0][b[0] != 0].min()) == float(pos.min())
        assert np.array_equal(hr.sample_heart(both, None, out, None, None, trunc)[0], hr.sample_heart(both, None, out, None, "range", trunc)[0])
        c = check_case(device, both, None, out, 7, clip=False, truncate=trunc)
        d = check_case(device, both, None, out, 7, clip=True, truncate=trunc)
        assert torch.equal(_bits(c[0]), _bits(d[0]))


def check_truncate_by_hand(device):
    """-1.5, -0.5, 0.5 and 2.5 through the kernel: toward zero, and no negative zero."""
    from cfun_amd import sample
    for pair, blends in (((-2.0, 4.0), [-1.5, -0.5, 2.5, 3.0]), ((2.0, -4.0), [1.5, 0.5, -2.5, -3.0])):
        src = torch.tensor(pair, dtype=torch.float64, device=device).reshape(2, 1, 1)
        g = sample.resize_rotate_box(src, None, (4, 1, 1), None, zscore=False, truncate=False, clip=False)[0]
        assert g.cpu().reshape(-1).tolist() == blends
        g = sample.resize_rotate_box(src, None, (4, 1, 1), None, zscore=False, truncate=True, clip=False)[0]
        assert g.cpu().reshape(-1).tolist() == [float(int(b)) for b in blends]
        assert not (_bits(g) == -2 ** 31).any()                                # no -0.0


def check_no_label(device):
    """label NULL: image and statistics as with a label, nothing else written (the wrapper passes NULL for all four)."""
    shape, out = (17, 15, 6), (20, 68, 5)
    src = hu(shape, 66)
    a = check_case(device, src, None, out, 13)
    b = check_case(device, src, blob(shape, 67), out, 13)
    assert a[1] is None and a[2] is None and torch.equal(_bits(a[0]), _bits(b[0]))


def check_boxes(device):
    """A label that reaches all six faces, a one-plane label (the zero box, not empty), an empty label."""
    shape = (16, 16, 10)
    src = hu(shape, 68)
    _, _, raw, box, empty = check_case(device, src, blob(shape, 69, kind="full"), (16, 16, 10), 90, zs=False)
    assert raw.cpu().tolist() == box.cpu().tolist() == [0, 0, 0, 10, 16, 16] and int(empty.cpu()) == 0
    _, _, raw, box, empty = check_case(device, src, blob(shape, 70, kind="plane"), (16, 16, 10), 7, zs=False)
    assert not raw.cpu().any() and not box.cpu().any() and int(empty.cpu()) == 0
    _, _, raw, _, _ = check_case(device, src, blob(shape, 70, kind="plane"), (16, 16, 25), 7, zs=False)      # the plane tripled
    assert raw.cpu().tolist()[3] - raw.cpu().tolist()[0] >= 2
    _, _, raw, box, empty = check_case(device, src, blob(shape, 71, kind="none"), (20, 70, 7), -13, zs=False)
    assert not raw.cpu().any() and not box.cpu().any() and int(empty.cpu()) == 1


def check_non_finite_and_zero(device):
    """A NaN source spreads through the blend, survives clip and cast and turns every normalised voxel NaN; the all-zero volume
    z-scores to NaN everywhere (the reference's 0 / 0)."""
    from cfun_amd import sample
    shape, out = (10, 9, 6), (14, 13, 9)
    src = hu(shape, 72, np.float32)
    src[3, 4, 2] = np.nan
    got = check_case(device, src, None, out, 13, clip=False, truncate=True)
    assert 1 < int(torch.isnan(got[0]).sum()) < got[0].numel() // 2
    z = sample.resize_rotate_box(fortran(src, device), None, out, 13, zscore=True, clip=False)
    assert bool(torch.isnan(z[0]).all()) and bool(torch.isnan(z[5]).all())
    zero = np.zeros(shape, np.int16)
    check_case(device, zero, blob(shape, 73), out, 13)
    z = sample.resize_rotate_box(fortran(zero, device), None, out, 13, zscore=True)
    assert bool(torch.isnan(z[0]).all()) and z[5].cpu().tolist()[0] == 0.0


def check_repeatable(device):
    from cfun_amd import sample
    shape, out = (33, 30, 12), (70, 68, 9)
    src, mask = hu(shape, 74), blob(shape, 75)
    ti, tm = fortran(src, device), fortran(mask, device)
    a = sample.resize_rotate_box(ti, tm, out, -13)
    b = sample.resize_rotate_box(ti, tm, out, -13)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[5].cpu().view(torch.int64), b[5].cpu().view(torch.int64))
    assert all(torch.equal(p, q) for p, q in zip(a[1:5], b[1:5]))
    check_case(device, src, mask, out, -13)


# --------------------------------------------------------------------------------------------------------- the C entry itself
OUTPUTS = (("image", torch.float32, -7.0), ("labels", torch.uint8, 201), ("raw_box", torch.int32, -77), ("box", torch.int32, -78),
           ("empty", torch.int32, -79), ("stats", torch.float64, -5.5), ("workspace", torch.uint8, 203))


def raw_call(device, src, mask, out, angle=7, clip=(0.0, 1.0), truncate=1, zscore=1, short=0, kind=None, lkind=None, null=(),
             margin=64):
    """cfun_sample_heart called directly, every output AND the workspace inside a larger buffer with ``margin`` canary elements
    either side, the workspace size passed ``short`` bytes below what cfun_sample_heart_workspace_bytes reports."""
    from cfun_amd import _lib, ops
    lib = _lib.load()
    ti, tm = fortran(src, device), fortran(mask, device)
    i64, i32 = C.c_int64 * 3, C.c_int32 * 3
    need = lib.cfun_sample_heart_workspace_bytes(i32(*out))
    n = min(max(1, abs(int(np.prod([float(v) for v in out])))), 1 << 20)
    counts = dict(image=n, labels=n, raw_box=6, box=6, empty=1, stats=2, workspace=max(int(need), 8))
    bufs, views = {}, {}
    for name, dt, canary in OUTPUTS:
        bufs[name] = torch.full((counts[name] + 2 * margin,), canary, dtype=dt, device=device)
        views[name] = bufs[name][margin:margin + counts[name]]
    before = {k: v.cpu().clone() for k, v in bufs.items()}
    clip_t = torch.tensor([float(clip[0]), float(clip[1])], dtype=torch.float64, device=device) if clip is not None else None
    c, s = sr.cos_sin(angle) if angle is not None else (1.0, 0.0)
    p = dict(image=ops.ptr_raw(ti), image_strides=i64(*ti.stride()), label=ops.ptr_raw(tm), label_strides=i64(*tm.stride()),
             dims=i32(*src.shape), out_dims=i32(*out), out_image=_lib.ptr(views["image"]), out_label=_lib.ptr(views["labels"]),
             raw_box=_lib.ptr(views["raw_box"]), box=_lib.ptr(views["box"]), empty=_lib.ptr(views["empty"]),
             stats=_lib.ptr(views["stats"]), workspace=_lib.ptr(views["workspace"]))
    for k in null:
        p[k] = None
    rc = lib.cfun_sample_heart(p["image"], p["image_strides"], ELEM[src.dtype] if kind is None else kind, p["label"], p["label_strides"],
                               LABEL[mask.dtype] if lkind is None else lkind, p["dims"], p["out_dims"], _lib.ptr(clip_t), truncate,
                               c, s, int(angle is not None), zscore, p["out_image"], p["out_label"], p["raw_box"], p["box"],
                               p["empty"], p["stats"], p["workspace"], max(int(need) - short, 0), _lib.stream(ti))
    return rc, views, bufs, before, need


def _canaries_intact(bufs, before, margin=64):
    for k, b in bufs.items():
        now = b.cpu()
        assert torch.equal(now[:margin], before[k][:margin]) and torch.equal(now[-margin:], before[k][-margin:]), "canary of " + k


def _untouched(bufs, before, what):
    for k, b in bufs.items():
        now, was = b.cpu(), before[k]
        same = torch.equal(now.view(torch.int64), was.view(torch.int64)) if now.dtype == torch.float64 else torch.equal(now, was)
        assert same, (what, k)


def check_refusals(device):
    """Every refusal of the header: the return code, and nothing written -- outputs, workspace and the canaries either side."""
    from cfun_amd import _lib
    shape, out = (10, 12, 5), (9, 8, 5)
    src, mask = hu(shape, 80), blob(shape, 81)
    clip = (float(src.min()), float(src.max()))
    rc, views, bufs, before, need = raw_call(device, src, mask, out, clip=clip)
    tiles = 1 * 1 * ((out[2] - 1) // HZ + 1)
    assert rc == 0 and need == tiles * (2 * 8 + 6 * 4)
    _canaries_intact(bufs, before)
    want = hr.sample_heart(src, mask, out, 7, clip, True)

    def shaped(v):
        return [v[k].reshape(out[2], out[0], out[1]) if k in ("image", "labels") else v[k] for k in ("image", "labels", "raw_box", "box", "empty")]

    got = shaped(views)
    assert got[2].cpu().tolist() == want[2].tolist() and got[3].cpu().tolist() == want[3].tolist()
    assert torch.equal(got[1].cpu(), torch.from_numpy(want[1]))
    rc, v0, b0, bf0, _ = raw_call(device, src, mask, out, clip=clip, zscore=0)
    assert rc == 0
    _canaries_intact(b0, bf0)
    compare(shaped(v0), want)
    _untouched({"stats": b0["stats"]}, bf0, "stats without zscore")
    check_zscore(v0["image"], views["image"], views["stats"], "raw call")
    # label NULL: image and stats written, the label's four outputs untouched -- and they may be NULL as well
    for null in (("label",), ("label", "label_strides", "out_label", "raw_box", "box", "empty")):
        rc, v1, b1, bf1, _ = raw_call(device, src, mask, out, clip=clip, null=null)
        assert rc == 0, null
        _untouched({k: b1[k] for k in ("labels", "raw_box", "box", "empty")}, bf1, null)
        _canaries_intact(b1, bf1)
        assert torch.equal(_bits(v1["image"]), _bits(views["image"]))
    rc, v1, b1, bf1, _ = raw_call(device, src, mask, out, clip=clip, zscore=0, null=("stats",))       # stats may be NULL without zscore
    assert rc == 0 and torch.equal(_bits(v1["image"]), _bits(v0["image"]))
    big = 2 ** 31 - 1
    bad = [dict(out=(0, 8, 5)), dict(out=(9, -1, 5)), dict(out=(9, 8, 0)),
           dict(out=(65536, 1, 1)),                                       # H' > 65535
           dict(out=(65535, big, big)),                                   # more tiles than one grid axis numbers
           dict(kind=3), dict(kind=-1), dict(lkind=4), dict(lkind=-1),
           dict(null=("stats",))] + \
          [dict(null=(k,)) for k in ("image", "image_strides", "label_strides", "dims", "out_dims", "out_image", "out_label", "raw_box",
                                     "box", "empty")]
    for kw in bad:
        args = dict(out=out)
        args.update(kw)
        rc, _, bufs, before, _ = raw_call(device, src, mask, args.pop("out"), clip=clip, **args)
        assert rc == EINVAL, (kw, rc)
        _untouched(bufs, before, kw)
    lib = _lib.load()
    i32 = C.c_int32 * 3
    for kw in (dict(short=1), dict(null=("workspace",))):
        rc, _, bufs, before, _ = raw_call(device, src, mask, out, clip=clip, **kw)
        assert rc == EWORKSPACE, (kw, rc)
        _untouched(bufs, before, kw)
    assert lib.cfun_sample_heart_workspace_bytes(i32(9, 0, 4)) == 0 and lib.cfun_sample_heart_workspace_bytes(i32(65535, big, big)) == 0
    assert lib.cfun_sample_heart_workspace_bytes(None) == 0


def check_bad_source_extent(device):
    """A non-positive source extent is refused before anything is read or written."""
    from cfun_amd import _lib, ops
    lib = _lib.load()
    src = fortran(hu((4, 4, 4), 82), device)
    out = torch.full((64,), -7.0, dtype=torch.float32, device=device)
    st = torch.full((2,), -5.5, dtype=torch.float64, device=device)
    ws = _lib.workspace(4096, src)
    i64, i32 = C.c_int64 * 3, C.c_int32 * 3
    for dims in ((4, 0, 4), (-1, 4, 4), (4, 4, 0)):
        rc = lib.cfun_sample_heart(ops.ptr_raw(src), i64(*src.stride()), INT16, None, None, 0, i32(*dims), i32(4, 4, 4), None, 1, 1.0, 0.0,
                                   0, 1, _lib.ptr(out), None, None, None, None, _lib.ptr(st), _lib.ptr(ws), 4096, _lib.stream(src))
        assert rc == EINVAL, dims
        assert bool((out == -7.0).all()) and bool((st == -5.5).all())


def check_wrapper_preconditions(device):
    from cfun_amd import sample
    src, mask = hu((10, 14, 5), 83), blob((10, 14, 5), 84)
    ti, tm = torch.from_numpy(src).to(device), torch.from_numpy(mask).to(device)
    with pytest.raises(ValueError, match="differ in shape"):
        sample.resize_rotate_box(ti, tm[:, :, :4], (8, 8, 4), 7)
    with pytest.raises(ValueError, match="label volume expected"):
        sample.resize_rotate_box(ti, ti.to(torch.float32), (8, 8, 4), 7)
    with pytest.raises(ValueError, match="unsupported extents"):
        sample.resize_rotate_box(ti, tm, (8, 0, 4), 7)
    with pytest.raises(ValueError, match="unsupported extents"):
        sample.resize_rotate_box(ti, tm, (65536, 1, 1), 7)
    with pytest.raises(ValueError, match=r"\[0, 255\]"):
        sample.resize_rotate_box(ti, tm + 300, (8, 8, 4), 7, strict=True)
    with pytest.raises(ValueError, match="empty"):
        sample.resize_rotate_box(ti, tm * 0, (8, 8, 4), 7, strict=True)


# ------------------------------------------------------------------------------------------------------------ end to end
def check_make_sample_heart_feeds_train_epoch(device, seed=2):
    """make_sample_heart on the tiny heart configuration from an int16 Fortran volume with int16 labels: labels, boxes and targets
    equal the restated sample's bit for bit, the image equals the restated un-normalised image normalised with the kernel's own
    statistics (which check_zscore holds to their bound), the dict feeds train_epoch for one step with finite losses, and the same
    step fed the restated sample gives the same losses bit for bit."""
    import copy
    import module_cases as mc
    from cfun_amd import sample, step, train
    cfg = mc.tiny_config("beginning")
    cfg.BATCH_SIZE = 1
    torch.manual_seed(seed)
    net = step.CFUNHotPath(cfg).to(device)
    b = cfg.UNET_MASK_BRANCH_CHANNEL
    gen = torch.Generator().manual_seed(1)
    masks = [torch.empty(cfg.TRAIN_ROIS_PER_IMAGE, c).bernoulli_(0.4, generator=gen) / 0.4 for c in (b, 2 * b, 4 * b, 8 * b, 16 * b)]
    net.mask.modified_u_net.dropout_masks = masks
    ref_net = copy.deepcopy(net)
    ref_net.mask.modified_u_net.dropout_masks = masks
    rng = _rng(seed)
    shape = (40, 36, 20)                                   # the loader's volume: not the network size
    image = np.asfortranarray(rng.integers(-1000, 1500, shape).astype(np.int16))
    mask = np.zeros(shape, np.int16, order="F")
    mask[8:32, 7:30, 3:17] = rng.integers(1, cfg.NUM_CLASSES, (24, 23, 14))
    anchors = net.anchors.to(device)
    keys = torch.from_numpy(rng.integers(0, 1 << 32, anchors.shape[0], dtype=np.uint64).astype(np.int64)).to(device)
    angle = 13.0
    s = sample.make_sample_heart(image, mask, angle, cfg, anchors, keys=keys, strict=True)

    mx, mn = int(cfg.IMAGE_MAX_DIM), int(cfg.IMAGE_MIN_DIM)
    dev = torch.device(device)
    r_img, r_lab, r_raw, r_box, r_empty = hr.sample_heart(image, mask, (mx, mx, mn), angle, "range", True)
    assert r_empty == 0
    match, bbox, counts = sr.build_rpn_targets(anchors.cpu().numpy(), r_box[None].astype(np.float64), cfg.RPN_TRAIN_ANCHORS_PER_IMAGE,
                                               cfg.RPN_BBOX_STD_DEV, keys.cpu().numpy())
    assert (match == 1).any()
    mean_k, std_k = [float(v) for v in s["stats"].cpu()]
    check_zscore(torch.from_numpy(r_img), s["image"][0, 0], s["stats"], "make_sample_heart")
    nfg = cfg.NUM_CLASSES - 1
    rs = dict(image=torch.from_numpy(((r_img.astype(np.float64) - mean_k) / std_k).astype(np.float32)).to(dev)[None, None],
              gt_class_ids=torch.arange(1, nfg + 1, device=dev), gt_boxes=torch.from_numpy(np.tile(r_box.astype(np.float32), (nfg, 1))).to(dev),
              gt_labels=torch.from_numpy(r_lab).to(dev), rpn_match=torch.from_numpy(match.reshape(1, -1, 1)).to(dev),
              rpn_bbox_t=torch.from_numpy(bbox.astype(np.float32)[None]).to(dev))
    for k in ("image", "gt_class_ids", "gt_boxes", "gt_labels", "rpn_match", "rpn_bbox_t"):
        assert s[k].dtype == rs[k].dtype and torch.equal(s[k], rs[k]), k
    assert s["raw_box"].cpu().tolist() == r_raw.tolist() and s["rpn_counts"].cpu().tolist() == counts.tolist()
    assert tuple(s["image"].shape) == (1, 1, mn, mx, mx)

    def one_step(n, smp):
        opt = train.make_optimizer(n, cfg, bucket_bytes=1 << 16)
        torch.manual_seed(11)                              # detection_target_layer's randperm draws
        return train.train_epoch(n, [smp], opt, 1, cfg)

    got, want = one_step(net, s), one_step(ref_net, rs)
    assert all(np.isfinite(v) for v in got), got
    assert got == want, (got, want)
    assert got[1] > 0 and got[2] > 0                       # the RPN losses saw the targets


def check_consistent_with_the_composed_route(device):
    """A float32 source with ``truncate`` off against ``make_sample`` (resize_image + resize_mask + rotate_and_box + mold_image):
    labels and boxes equal exactly; the image agrees within the bound head_cases applies to resize3d(order=1) against its float64
    reference (membound_cases.hold: error <= 3 x the float32 reference's own error + 2e-5, over the tensor's max-abs) -- the
    composed route resizes in float32, this pass in float64, so this pass stands in for the float64 reference and head_cases'
    float32 restatement of resize3d, rotated and z-scored in float64, for the float32 one."""
    import head_cases as hc
    import module_cases as mc
    from cfun_amd import sample, step
    cfg = mc.tiny_config("beginning")
    cfg.BATCH_SIZE = 1
    torch.manual_seed(0)
    net = step.CFUNHotPath(cfg).to(device)
    anchors = net.anchors.to(device)
    rng = _rng(5)
    shape = (40, 36, 20)
    image = rng.normal(0.0, 1.0, shape).astype(np.float32)
    mask = np.zeros(shape, np.int32)
    mask[8:32, 7:30, 3:17] = rng.integers(1, cfg.NUM_CLASSES, (24, 23, 14))
    keys = torch.from_numpy(rng.integers(0, 1 << 32, anchors.shape[0], dtype=np.uint64).astype(np.int64)).to(device)
    for angle in (13.0, None):
        a = sample.make_sample(image, mask, angle, cfg, anchors, keys=keys)
        b = sample.make_sample_heart(image, mask, angle, cfg, anchors, keys=keys)
        for k in ("gt_labels", "gt_boxes", "raw_box", "empty", "rpn_match", "rpn_bbox_t", "rpn_counts", "gt_class_ids"):
            assert torch.equal(a[k], b[k]), (angle, k)
        mx, mn = int(cfg.IMAGE_MAX_DIM), int(cfg.IMAGE_MIN_DIM)
        vol = torch.from_numpy(image)
        r32 = hc._resize_ref(vol, (mx, mx, mn), 1, None, None, True, torch.float32).numpy()
        r32 = sr.rotate_slices(r32, angle).transpose(2, 0, 1)
        ref32 = torch.from_numpy(hr.zscore(r32)[1])[None, None]
        hc.hold("make_sample vs make_sample_heart", "angle %r" % (angle,), a["image"], b["image"].double(), ref32)


def check_detect_heart(device):
    """mold_inputs_heart's triple: metas and windows equal utils.mold_inputs', the molded tensor is the restated image normalised
    with the kernel's statistics; detect_heart equals detect_molded fed that restated tensor."""
    import eval_cases as ec
    import module_cases as mc
    from cfun_amd import evaluate, native, sample, utils
    cfg = mc.tiny_config("beginning")
    net = ec._net(device, cfg, 2)
    shape = (40, 36, 20)
    image = np.asfortranarray(_rng(9).normal(0.0, 200.0, shape).astype(np.int16))[..., None]
    mx, mn = int(cfg.IMAGE_MAX_DIM), int(cfg.IMAGE_MIN_DIM)
    molded, metas, windows = native.mold_inputs_heart(cfg, [image], device=device)
    _, r_metas, r_windows = utils.mold_inputs(cfg, [image], device=device)
    assert np.array_equal(metas, r_metas) and np.array_equal(windows, r_windows)
    assert tuple(molded.shape) == (1, 1, mn, mx, mx) and molded.dtype == torch.float32
    r_img = hr.sample_heart(image[..., 0], None, (mx, mx, mn), None, "range", True)[0]
    z = sample.resize_rotate_box(torch.from_numpy(image[..., 0]).to(device), None, (mx, mx, mn), None, zscore=True)
    check_zscore(torch.from_numpy(r_img), molded[0, 0], z[5], "mold_inputs_heart")
    mean_k, std_k = [float(v) for v in z[5].cpu()]
    restated = torch.from_numpy(((r_img.astype(np.float64) - mean_k) / std_k).astype(np.float32)).to(device)[None, None]
    assert torch.equal(_bits(molded), _bits(restated))
    # float images are not truncated; a tensor goes in as well as an array
    f = image.astype(np.float32) + 0.25
    mf = native.mold_inputs_heart(cfg, [torch.from_numpy(f)], device=device)[0]
    zf = sample.resize_rotate_box(torch.from_numpy(f[..., 0]).to(device), None, (mx, mx, mn), None, zscore=True, truncate=False)
    assert torch.equal(_bits(mf[0, 0]), _bits(zf[0]))
    res = native.detect_heart(net, image)
    ref = evaluate.detect_molded(net, restated, tuple(float(v) for v in windows[0]), list(shape))
    assert not res["empty"] and res["mask_device"].any(), "test setup: no detection / an all-zero map"
    assert tuple(res["mask_device"].shape) == (shape[2], shape[0], shape[1]) and torch.equal(res["mask_device"], ref["mask_device"])
    for k in ("rois", "class_ids", "scores"):
        assert np.array_equal(np.asarray(res[k]), np.asarray(ref[k])), k
    with pytest.raises(ValueError, match="volume expected"):
        native.detect_heart(net, image[..., 0])


def check_gpu_shape(device):
    """GPU only: 512x512x224 int16 in Fortran order with int16 labels -> 320x320x192 at 13 degrees, truncate and zscore.  The
    un-normalised image and the labels are compared on the first plane, the last plane and three seeded planes of the restatement;
    statistics and the normalised image are held whole."""
    from cfun_amd import sample
    shape, out = (512, 512, 224), (320, 320, 192)
    rng = _rng(110)
    src = np.asfortranarray(rng.integers(-1024, 1500, shape, dtype=np.int16))
    mask = np.zeros(shape, np.int16, order="F")
    mask[100:400, 120:380, 40:170] = rng.integers(0, 3, (300, 260, 130))
    ti, tm = torch.from_numpy(src).to(device), torch.from_numpy(mask).to(device)
    assert ti.stride() == (1, 512, 512 * 512)
    raw = sample.resize_rotate_box(ti, tm, out, 13)
    plain = sample.resize_rotate_box(ti, tm, out, 13, zscore=False)
    planes = sorted({0, out[2] - 1} | set(int(v) for v in rng.choice(np.arange(1, out[2] - 1), 3, replace=False)))
    r_img, r_lab = hr.sample_heart(src, mask, out, 13, "range", True, planes=planes)[:2]
    assert torch.equal(_bits(plain[0][planes]), torch.from_numpy(r_img).view(torch.int32))
    assert torch.equal(plain[1][planes].cpu(), torch.from_numpy(r_lab)) and r_lab.any()
    assert torch.equal(plain[1], raw[1]) and torch.equal(plain[3], raw[3]) and int(raw[4].cpu()) == 0
    lab = plain[1].cpu().numpy()
    r_raw, r_empty = sr.extract_box(lab)
    assert raw[2].cpu().tolist() == r_raw.tolist() and raw[3].cpu().tolist() == sr.expand_box(r_raw, lab.shape).tolist()
    check_zscore(plain[0], raw[0], raw[5], "512x512x224 -> 320x320x192")


# ------------------------------------------------------------------------------------------------------------ accounting
def header_symbols():
    """The same parse as test_abi.header_symbols, on include/cfun_sample_heart.h."""
    txt = open(os.path.join(ROOT, "include", "cfun_sample_heart.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(cfun_[a-z0-9_]+)\s*\(", txt)))


NO_LAUNCH = {"cfun_sample_heart_workspace_bytes": "host-side query: launches nothing, touches no device memory"}


def check_coverage(tier):
    from cfun_amd import _lib
    assert header_symbols() == sorted(_lib.HEART_SAMPLE_EXPORTS) == ["cfun_sample_heart", "cfun_sample_heart_workspace_bytes"]
    for other in (_lib.EXPORTS, _lib.SAMPLE_EXPORTS, _lib.LITS_SAMPLE_EXPORTS, _lib.NATIVE_EXPORTS, _lib.TILE_EXPORTS, _lib.EVAL_EXPORTS,
                  _lib.CC_EXPORTS, _lib.SURFACE_EXPORTS, _lib.LESION_EXPORTS, _lib.FILL_EXPORTS, _lib.MORPH_EXPORTS):
        assert not set(_lib.HEART_SAMPLE_EXPORTS) & set(other)
    missed = sorted(set(_lib.HEART_SAMPLE_EXPORTS) - set(NO_LAUNCH) - guard.SEEN[tier])
    assert not missed, "heart sample entries that launch work but never ran under guard: %s" % missed
