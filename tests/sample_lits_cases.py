"""Cases of the LiTS sample path (cfun_amd.sample.frame_rotate_resize / make_sample_lits, k_lits_gather in
cfun_amd/csrc/sample.hip) shared by test_sample_lits_emu.py and test_sample_lits_gpu.py: the device against
tests/sample_lits_ref.py.  Both sides compute every index in float64 in the header's operation order and the image value in
float32 as two rounded operations, so image bits, labels, both boxes and the flag must be equal everywhere."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import guard
import sample_lits_ref as lr
import sample_ref as sr
from conftest import ROOT

EINVAL, EWORKSPACE = -1, -2


def tile_constants():
    """kTX, kTZ, kPitch as cfun_amd/csrc/sample.hip states them; the shapes below are derived from these values."""
    txt = open(os.path.join(ROOT, "cfun_amd", "csrc", "sample.hip")).read()
    m = re.search(r"constexpr int kTX = (\d+), kTZ = (\d+), kPitch = (\d+);", txt)
    assert m, "sample.hip no longer states its tile constants in one line"
    return tuple(int(v) for v in m.groups())


TX, TZ, PITCH = tile_constants()
assert (TX, TZ, PITCH) == (64, 64, 65), "the tile changed: re-derive W_OUT / D_OUT below from the new constants"
W_OUT = [TX - 1, TX, TX + 1, 2 * TX, 2 * TX + 2]        # 63 (scalar stores, ragged), 64 / 128 (16-byte stores), 65, 130 (two and
D_OUT = [1, TZ - 1, TZ, TZ + 1, 2 * TZ + 2]             # three tiles, ragged, 130 % 4 != 0); the same along z
ANGLES = [None, 0, 7, -13, 30, -30, 90, 180]

# (source, frame, output) as (H, W, D) for the W' sweep, H' = 1 throughout: x down-sampled (63 .. 65 from 90), up-sampled (128 /
# 130 from 90: several x share a source column); D' = 3 from 5 frame planes
W_CASES = [((5, 80, 4), (6, 90, 5), (1, w, 3)) for w in W_OUT]
# the D' sweep: z down-sampled by about 2.1 as at the product shape (63 .. 65 from 135), up-sampled (130 from 40: several output
# z share one source z), and D' = 1
D_CASES = [((6, 10, 120), (7, 12, 135), (3, 8, d)) for d in D_OUT[:4]] + [((6, 10, 33), (7, 12, 40), (3, 8, D_OUT[4]))]


def _rng(seed):
    return np.random.default_rng(seed)


def _volume(shape, seed, kind="blob", dtype=np.int8):
    rng = _rng(seed)
    image = rng.normal(0.0, 250.0, shape).astype(np.float32)            # HU: both clamps and the open interval are hit
    mask = np.zeros(shape, dtype)
    if kind == "blob":
        lo = [n // 4 for n in shape]
        hi = [max(l + 1, n - n // 5) for l, n in zip(lo, shape)]
        mask[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = rng.integers(0, 3, [b - a for a, b in zip(lo, hi)])
    elif kind == "full":
        mask[:] = rng.integers(1, 100, shape)
    elif kind == "plane":                                               # one source plane thick along z
        mask[1:-1, 1:-1, shape[2] // 2] = 2
    return image, mask


def check_case(device, image, mask, frame, out, angle=None, norm=True, t_image=None, t_mask=None):
    """image / mask: numpy [H,W,D]; t_image / t_mask: the (possibly strided) device views holding the same values."""
    from cfun_amd import sample
    ti = torch.from_numpy(image).to(device) if t_image is None else t_image
    tm = torch.from_numpy(mask).to(device) if t_mask is None else t_mask
    got = sample.frame_rotate_resize(ti, tm, frame, out, angle=angle, normalise=norm)
    want = lr.frame_rotate_resize(image, mask, frame, out, angle, norm)
    compare(got, want, "angle %r" % (angle,))
    return got


def compare(got, want, what=""):
    img, lab, raw, box, empty = got
    r_img, r_lab, r_raw, r_box, r_empty = want
    assert img.dtype == torch.float32 and lab.dtype == torch.uint8 and raw.dtype == box.dtype == empty.dtype == torch.int32
    assert tuple(img.shape) == tuple(lab.shape) == r_img.shape
    assert torch.equal(img.cpu().view(torch.int32), torch.from_numpy(r_img).view(torch.int32)), "image bits, " + what
    assert torch.equal(lab.cpu(), torch.from_numpy(r_lab)), "labels, " + what
    assert raw.cpu().tolist() == r_raw.tolist() and box.cpu().tolist() == r_box.tolist(), (what, raw, r_raw, box, r_box)
    assert empty.cpu().tolist() == [r_empty], what


def check_sweep(device, triple):
    shape, frame, out = triple
    image, mask = _volume(shape, sum(out))
    for angle in (None, 7, -30):
        check_case(device, image, mask, frame, out, angle)


def check_angles(device):
    """Every angle of the issue on a non-square frame with an odd pad difference on every axis, and on an even square (90 and
    180 are whole-pixel maps there).  Angle 0 and no map are bit-identical."""
    for shape, frame, out in (((21, 18, 9), (30, 27, 14), (16, 12, 6)), ((20, 20, 8), (24, 24, 10), (40, 40, 20))):
        image, mask = _volume(shape, 11)
        res = {a: check_case(device, image, mask, frame, out, a) for a in ANGLES}
        assert all(torch.equal(p, q) for p, q in zip(res[None], res[0]))
        assert not torch.equal(res[7][0], res[None][0]) and not torch.equal(res[30][1], res[-30][1])


def check_offsets_and_extents(device):
    """Offset 0 on every axis (frame = source: the source touches all six faces of the frame), frame = source = output (the
    identity), an odd pad difference, and a one-plane source."""
    image, mask = _volume((9, 7, 3), 12)
    for angle in (None, 13):
        check_case(device, image, mask, (9, 7, 3), (9, 7, 3), angle)
        check_case(device, image, mask, (9, 7, 3), (12, 5, 7), angle)
    got = check_case(device, image, mask, (9, 7, 3), (9, 7, 3), None, norm=False)
    assert torch.equal(got[0].cpu(), torch.from_numpy(image).permute(2, 0, 1))
    check_case(device, image, mask, (12, 10, 6), (11, 9, 5), -13)               # P - n = 3 on every axis
    image, mask = _volume((14, 11, 1), 13, "full")                              # source D = 1
    for out in ((10, 9, 1), (10, 9, 4)):
        check_case(device, image, mask, (16, 12, 1), out, 7)
        check_case(device, image, mask, (16, 12, 3), out, None)


def check_label_dtypes(device):
    shape, frame, out = (21, 18, 9), (30, 26, 14), (16, 12, 6)
    image, mask = _volume(shape, 14)
    got = [check_case(device, image, mask.astype(dt), frame, out, -13) for dt in (np.int8, np.uint8, np.int32)]
    assert all(torch.equal(got[0][1], g[1]) and torch.equal(got[0][3], g[3]) for g in got[1:])
    big = _rng(15).integers(128, 256, shape).astype(np.uint8)                   # the high bit of a byte is a value, not a sign
    check_case(device, image, big, frame, out, 7)
    wide = _rng(16).integers(-300, 600, shape).astype(np.int32)                 # outside the precondition: the low 8 bits
    check_case(device, image, wide, frame, out, 7)


def check_strided_sources(device):
    """Sources read in place through their strides: a Fortran-ordered pair (numpy's order='F': H fastest) and a sliced view."""
    shape, frame, out = (24, 20, 7), (30, 26, 9), (17, 15, 8)
    image, mask = _volume(shape, 17)
    ti = torch.from_numpy(np.ascontiguousarray(image.transpose(2, 1, 0))).to(device).permute(2, 1, 0)
    tm = torch.from_numpy(np.ascontiguousarray(mask.transpose(2, 1, 0))).to(device).permute(2, 1, 0)
    assert ti.stride() == (1, 24, 480) and tm.stride() == (1, 24, 480)
    check_case(device, image, mask, frame, out, 13, t_image=ti, t_mask=tm)
    big_i, big_m = _volume((26, 43, 10), 18)
    sl = (slice(1, 25), slice(2, 42, 2), slice(3, None))
    ti, tm = torch.from_numpy(big_i).to(device)[sl], torch.from_numpy(big_m).to(device)[sl]
    assert not ti.is_contiguous() and not tm.is_contiguous()
    check_case(device, np.ascontiguousarray(big_i[sl]), np.ascontiguousarray(big_m[sl]), frame, out, -20, t_image=ti, t_mask=tm)


def check_normalisation(device):
    """Normalisation off is a plain copy; on, the hand answers of the header and a NaN that stays a NaN."""
    shape, frame, out = (10, 12, 5), (12, 15, 6), (9, 10, 5)
    image, mask = _volume(shape, 19)
    image[:2, :6, 0] = np.array([300, -300, 301, -301, 0, np.nan], np.float32)
    image[4, 4, 2] = np.nan
    check_case(device, image, mask, frame, out, 7, norm=False)
    check_case(device, image, mask, frame, out, 7, norm=True)
    got = check_case(device, image, mask, shape, shape, None)
    assert got[0].cpu()[0, 0, :5].tolist() == [0.0, 1.0, 0.0, 1.0, 0.5] and bool(torch.isnan(got[0].cpu()[0, 0, 5]))


def check_boxes(device):
    """An empty label, a one-plane label, and a label that reaches all six faces after the rotation."""
    shape = (16, 16, 70)
    image, mask = _volume(shape, 20, "full")
    _, _, raw, box, empty = check_case(device, image, mask, shape, shape, 90)           # even square: a whole-pixel map
    assert raw.cpu().tolist() == box.cpu().tolist() == [0, 0, 0, 70, 16, 16] and int(empty.cpu()) == 0
    _, _, raw, box, _ = check_case(device, image, mask, (18, 18, 72), (20, 20, 66), 30)
    assert raw.cpu().tolist()[:3] != [0, 0, 0]                                          # the frame's padding shows
    image, mask = _volume((12, 10, 5), 21, "plane")
    _, _, raw, box, empty = check_case(device, image, mask, (12, 10, 5), (12, 10, 5), 7)
    assert not raw.cpu().any() and not box.cpu().any() and int(empty.cpu()) == 0        # one plane: the zero box, not "empty"
    check_case(device, image, mask, (14, 12, 5), (14, 12, 10), 7)                       # the plane doubled by the up-sampling
    image, mask = _volume((12, 10, 5), 22, "none")
    _, _, raw, box, empty = check_case(device, image, mask, (14, 12, 6), (9, 9, 4), -13)
    assert not raw.cpu().any() and not box.cpu().any() and int(empty.cpu()) == 1


def check_repeatable(device):
    from cfun_amd import sample
    shape, frame, out = (33, 40, 70), (40, 44, 75), (20, 68, 66)
    image, mask = _volume(shape, 23)
    ti, tm = torch.from_numpy(image).to(device), torch.from_numpy(mask).to(device)
    a = sample.frame_rotate_resize(ti, tm, frame, out, angle=-13)
    b = sample.frame_rotate_resize(ti, tm, frame, out, angle=-13)
    assert all(torch.equal(p.view(torch.int32) if p.dtype == torch.float32 else p, q.view(torch.int32) if q.dtype == torch.float32 else q)
               for p, q in zip(a, b))
    compare(a, lr.frame_rotate_resize(image, mask, frame, out, -13))


def agreeing_hu(n, seed):
    """HU values on which IEEE division by -600 and multiplication by the rounded reciprocal give the same float32 after the
    clamp.  utils.preprocess_image_lits is torch's ``x / python_scalar``: a true division on the host, but on the device torch
    multiplies by the scalar's rounded reciprocal (one bit looser, by torch's own note).  The rule of cfun_sample_lits.h is the
    division, and the kernel is held to it on unrestricted values by every other case; the comparison with the existing device
    route is about the geometry (frame, offset, index rule), so it draws its values from the set on which the two forms cannot
    differ -- computed here from float32 arithmetic alone, not from either implementation."""
    hu = np.arange(-1100, 1101, dtype=np.float32)
    k = hu - np.float32(300.0)
    a = np.clip(k / np.float32(-600.0), 0, 1)
    b = np.clip(k * (np.float32(1.0) / np.float32(-600.0)), 0, 1)
    pool = hu[a == b]
    inside = pool[(pool > -300) & (pool < 300)]
    assert inside.size > 100, "too few HU values inside the window agree: %d" % inside.size
    return np.concatenate([inside, pool])[_rng(seed).integers(0, inside.size + pool.size, n)]


def check_equals_the_existing_device_routes(device):
    """Without a map: the image equals utils.mold_inputs_lits (the inference side of the same data path) -- every voxel in value,
    and in bits except the sign of a zero -- and the labels equal ops.resize3d(order=0, frame=..., offset=...) of the label."""
    import types
    from cfun_amd import ops, utils
    for shape, frame, out in (((21, 18, 9), (30, 26, 14), (16, 12, 6)), ((33, 40, 70), (40, 44, 75), (20, 68, 66)),
                              ((20, 20, 8), (24, 24, 10), (40, 40, 20))):
        cfg = types.SimpleNamespace(PAD_IMAGE_SHAPE=list(frame), IMAGE_SHAPE=np.array(list(out) + [1]), IMAGE_MIN_DIM=out[2],
                                    IMAGE_MAX_DIM=out[0], NUM_CLASSES=3)
        image = agreeing_hu(int(np.prod(shape)), 24).reshape(shape).astype(np.float32)
        _, mask = _volume(shape, 25)
        got = check_case(device, image, mask, frame, out, None)
        molded, _, _ = utils.mold_inputs_lits(cfg, [image], device=device)
        bits = got[0].view(torch.int32) != molded[0, 0].view(torch.int32)
        print("%s: %d of %d voxels differ in value from mold_inputs_lits, %d in bits" % (shape, int((got[0] != molded[0, 0]).sum()),
                                                                                       bits.numel(), int(bits.sum())))
        assert torch.equal(got[0], molded[0, 0])
        # ... and bit for bit, but for the sign of a zero: HU 300 is 0 / -600 = -0.0, which the reference's masked assignments
        # and this pass leave alone, while torch's clamp on the device returns +0.0
        assert not (got[0][bits] != 0).any() and not (molded[0, 0][bits] != 0).any()
        off = lr.offsets(frame, shape)
        tm = torch.from_numpy(mask.astype(np.float32)).to(device).permute(2, 0, 1)
        rl = ops.resize3d(tm, (out[2], out[0], out[1]), order=0, frame=(frame[2], frame[0], frame[1]), offset=(off[2], off[0], off[1]))
        assert torch.equal(got[1], rl.to(torch.uint8))


# --------------------------------------------------------------------------------------------------------- the C entry itself
def raw_call(device, image, mask, frame, off, out, amap=None, norm=1, short=0, elem=None, null=None, margin=32):
    """cfun_sample_lits called directly, every output inside a larger buffer with ``margin`` canary elements either side and the
    workspace ``short`` bytes below what cfun_sample_lits_workspace_bytes reports.  Returns (rc, outputs, buffers, canary)."""
    from cfun_amd import _lib, ops
    lib = _lib.load()
    ti, tm = torch.from_numpy(image).to(device), torch.from_numpy(mask).to(device)
    i64, i32 = C.c_int64 * 3, C.c_int32 * 3
    need = lib.cfun_sample_lits_workspace_bytes(i32(*out))
    n = max(1, abs(int(np.prod(out))))
    bufs, views = {}, {}
    for name, count, dt, canary in (("image", n, torch.float32, -7.0), ("labels", n, torch.uint8, 201), ("raw_box", 6, torch.int32, -77),
                                    ("box", 6, torch.int32, -78), ("empty", 1, torch.int32, -79)):
        bufs[name] = torch.full((count + 2 * margin,), canary, dtype=dt, device=device)
        views[name] = bufs[name][margin:margin + count]
    before = {k: v.cpu().clone() for k, v in bufs.items()}
    ws = _lib.workspace(max(need - short, 0), ti)
    p = dict(image=ops.ptr_raw(ti), image_strides=i64(*ti.stride()), label=ops.ptr_raw(tm), label_strides=i64(*tm.stride()),
             dims=i32(*image.shape), frame=i32(*frame), offset=i32(*off), out_dims=i32(*out),
             out_image=_lib.ptr(views["image"]), out_label=_lib.ptr(views["labels"]), raw_box=_lib.ptr(views["raw_box"]),
             box=_lib.ptr(views["box"]), empty=_lib.ptr(views["empty"]), workspace=_lib.ptr(ws))
    if null:
        p[null] = None
    rc = lib.cfun_sample_lits(p["image"], p["image_strides"], p["label"], p["label_strides"], tm.element_size() if elem is None else elem,
                              p["dims"], p["frame"], p["offset"], p["out_dims"], (C.c_double * 6)(*amap) if amap is not None else None,
                              norm, p["out_image"], p["out_label"], p["raw_box"], p["box"], p["empty"], p["workspace"],
                              max(need - short, 0), _lib.stream(ti))
    return rc, views, bufs, before, need


def _canaries_intact(views, bufs, before, margin=32):
    for k, b in bufs.items():
        now = b.cpu()
        assert torch.equal(now[:margin], before[k][:margin]) and torch.equal(now[-margin:], before[k][-margin:]), "canary of " + k


def check_refusals(device):
    """Every refusal of the header: the return code, and nothing written -- outputs and the canaries either side of them."""
    shape, frame, off, out = (10, 12, 5), (14, 15, 6), (2, 1, 0), (9, 8, 4)
    image, mask = _volume(shape, 26)
    rc, views, bufs, before, need = raw_call(device, image, mask, frame, off, out, lr.rotation_map(7, 14, 15))
    assert rc == 0 and need == 6 * 4 * 9                                 # one workgroup per output row: 1 x H' x 1
    _canaries_intact(views, bufs, before)
    compare([views[k].reshape(4, 9, 8) if k in ("image", "labels") else views[k] for k in ("image", "labels", "raw_box", "box", "empty")],
            lr.frame_rotate_resize(image, mask, frame, out, 7, off=off))
    nan_map = (1.0, 0.0, float("nan"), 0.0, 1.0, 0.0)
    inf_map = (1.0, 0.0, 0.0, float("inf"), 1.0, 0.0)
    bad = [dict(frame=(9, 15, 6)), dict(frame=(14, 15, 4)),              # the source is larger than the frame
           dict(off=(5, 1, 0)), dict(off=(2, 4, 0)), dict(off=(2, 1, 2)),   # ... or does not fit at the offset
           dict(off=(-1, 1, 0)),
           dict(out=(0, 8, 4)), dict(out=(9, -1, 4)), dict(out=(9, 8, 0)), dict(frame=(14, 0, 6)),
           dict(out=(65536, 1, 1)),
           dict(elem=2), dict(elem=8), dict(elem=0),
           dict(amap=nan_map), dict(amap=inf_map)] + \
          [dict(null=k) for k in ("image", "image_strides", "label", "label_strides", "dims", "frame", "offset", "out_dims",
                                  "out_image", "out_label", "raw_box", "box", "empty")]
    for kw in bad:
        args = dict(frame=frame, off=off, out=out)
        args.update(kw)
        rc, views, bufs, before, _ = raw_call(device, image, mask, args.pop("frame"), args.pop("off"), args.pop("out"), **args)
        assert rc == EINVAL, (kw, rc)
        assert all(torch.equal(b.cpu(), before[k]) for k, b in bufs.items()), kw
    for kw in (dict(short=1), dict(null="workspace")):
        rc, views, bufs, before, _ = raw_call(device, image, mask, frame, off, out, **kw)
        assert rc == EWORKSPACE, (kw, rc)
        assert all(torch.equal(b.cpu(), before[k]) for k, b in bufs.items()), kw
    from cfun_amd import _lib
    assert _lib.load().cfun_sample_lits_workspace_bytes((C.c_int32 * 3)(9, 0, 4)) == 0


def check_far_faces(device):
    """The entry takes any offset that fits: a source pushed against the frame's far faces (offset = P - n), odd and even."""
    shape, frame, out = (10, 12, 5), (14, 15, 9), (13, 16, 7)
    image, mask = _volume(shape, 27, "full")
    off = tuple(p - n for p, n in zip(frame, shape))
    for amap in (None, lr.rotation_map(-13, 14, 15)):
        rc, views, bufs, before, _ = raw_call(device, image, mask, frame, off, out, amap)
        assert rc == 0
        _canaries_intact(views, bufs, before)
        want = lr.frame_rotate_resize(image, mask, frame, out, None, amap=amap, off=off)
        compare([views[k].reshape(7, 13, 16) if k in ("image", "labels") else views[k] for k in ("image", "labels", "raw_box", "box", "empty")],
                want)
        if amap is None:
            assert want[2].tolist()[3:] == [7, 13, 16]                   # the box reaches the output's far faces


def check_wrapper_preconditions(device):
    from cfun_amd import sample
    image, mask = _volume((10, 14, 5), 28)
    ti, tm = torch.from_numpy(image).to(device), torch.from_numpy(mask).to(device)
    with pytest.raises(ValueError, match="differ in shape"):
        sample.frame_rotate_resize(ti, tm[:, :, :4], (12, 16, 6), (8, 8, 4))
    with pytest.raises(ValueError, match="label volume expected"):
        sample.frame_rotate_resize(ti, ti, (12, 16, 6), (8, 8, 4))
    with pytest.raises(ValueError, match="does not fit"):
        sample.frame_rotate_resize(ti, tm, (12, 13, 6), (8, 8, 4))
    with pytest.raises(ValueError, match="unsupported extents"):
        sample.frame_rotate_resize(ti, tm, (12, 16, 6), (8, 0, 4))
    with pytest.raises(ValueError, match=r"\[0, 255\]"):
        sample.frame_rotate_resize(ti, tm.to(torch.int32) + 300, (12, 16, 6), (8, 8, 4), strict=True)
    with pytest.raises(ValueError, match="empty"):
        sample.frame_rotate_resize(ti, tm * 0, (12, 16, 6), (8, 8, 4), strict=True)


def check_draw_angle_and_config():
    from cfun_amd import config, sample
    cfg = config.LiTSConfig("beginning")
    assert tuple(cfg.ROTATE_ANGLE) == (-30, 31) and cfg.AUGMENTATION is True
    gen = torch.Generator().manual_seed(3)
    draws = [sample.draw_angle(cfg, gen) for _ in range(400)]
    assert all(isinstance(a, int) for a in draws) and min(draws) == -30 and max(draws) == 30
    gen2 = torch.Generator().manual_seed(3)
    assert draws[:5] == [int(torch.randint(-30, 31, (1,), generator=gen2)) for _ in range(5)]      # as the fork draws it
    assert isinstance(sample.draw_angle(cfg), int)


# ------------------------------------------------------------------------------------------------------------ end to end
def check_make_sample_lits_feeds_train_epoch(device, seed=2):
    """make_sample_lits on the tiny LiTS configuration: the sample's tensors equal the restated sample's (targets by sample_ref on
    the restated label) bit for bit, window and meta equal mold_inputs_lits', the dict feeds train_epoch for two steps with finite
    losses, and the same two steps fed the restated sample give the same losses bit for bit."""
    import copy
    import module_cases as mc
    from cfun_amd import sample, step, train, utils
    cfg = mc.tiny_lits_config("beginning")
    cfg.BATCH_SIZE = 1
    cfg.PAD_IMAGE_SHAPE = [44, 41, 24]
    torch.manual_seed(seed)
    net = step.CFUNHotPath(cfg).to(device)
    ref_net = copy.deepcopy(net)
    rng = _rng(seed)
    src = (36, 30, 17)                                     # the loader's volume: raw HU, int8 labels
    image = rng.normal(0.0, 250.0, src).astype(np.float32)
    mask = np.zeros(src, np.int8)
    mask[6:30, 5:26, 2:15] = rng.integers(1, cfg.NUM_CLASSES, (24, 21, 13))
    anchors = net.anchors.to(device)
    keys = torch.from_numpy(rng.integers(0, 1 << 32, anchors.shape[0], dtype=np.uint64).astype(np.int64)).to(device)
    angle = -13
    s = sample.make_sample_lits(image, mask, angle, cfg, anchors, keys=keys, strict=True)

    dev = torch.device(device)
    out = tuple(int(v) for v in cfg.IMAGE_SHAPE[:3])
    ref = lr.make_sample(image, mask, angle, cfg.PAD_IMAGE_SHAPE, out, cfg.NUM_CLASSES, anchors.cpu().numpy(),
                         cfg.RPN_TRAIN_ANCHORS_PER_IMAGE, cfg.RPN_BBOX_STD_DEV, keys.cpu().numpy())
    assert ref["empty"] == 0 and (ref["rpn_match"] == 1).any()
    keys6 = ("image", "gt_class_ids", "gt_boxes", "gt_labels", "rpn_match", "rpn_bbox_t")
    rs = {k: torch.from_numpy(np.ascontiguousarray(ref[k])).to(dev) for k in keys6}
    for k in keys6:
        assert s[k].dtype == rs[k].dtype and torch.equal(s[k], rs[k]), k
    assert tuple(s["image"].shape) == (1, 1, out[2], out[0], out[1])
    assert 0.0 <= float(s["image"].min()) and float(s["image"].max()) <= 1.0          # clamp-normalised, never z-scored
    _, metas, windows = utils.mold_inputs_lits(cfg, [image], device=device)
    assert tuple(windows[0]) == tuple(s["window"]) == lr.window(cfg.PAD_IMAGE_SHAPE, src, out, cfg.IMAGE_MIN_DIM, cfg.IMAGE_MAX_DIM)
    assert np.array_equal(metas[0], s["image_meta"])
    val = sample.make_sample_lits(torch.from_numpy(image), torch.from_numpy(mask.astype(np.int32)), None, cfg, anchors, keys=keys)
    want = lr.frame_rotate_resize(image, mask, cfg.PAD_IMAGE_SHAPE, out, None)          # the validation form, tensors, int32
    assert torch.equal(val["image"][0, 0].cpu(), torch.from_numpy(want[0])) and torch.equal(val["gt_labels"].cpu(), torch.from_numpy(want[1]))

    def two_steps(n, smp):
        opt = train.make_optimizer(n, cfg, bucket_bytes=1 << 16)
        torch.manual_seed(11)                              # detection_target_layer's randperm draws
        return train.train_epoch(n, [smp, smp], opt, 2, cfg)

    got, want = two_steps(net, s), two_steps(ref_net, rs)
    assert all(np.isfinite(v) for v in got), got
    assert got == want, (got, want)
    assert got[1] > 0 and got[2] > 0                       # the RPN losses saw the targets


def check_product_shape(device):
    """GPU only: the product frame 646x646x536 -> 256x320x320 from a 256x256x160 source with int8 labels at 17 degrees."""
    shape, frame, out = (256, 256, 160), (646, 646, 536), (320, 320, 256)
    rng = _rng(29)
    image = rng.normal(0.0, 250.0, shape).astype(np.float32)
    mask = np.zeros(shape, np.int8)
    mask[60:200, 50:190, 30:130] = rng.integers(0, 3, (140, 140, 100))
    got = check_case(device, image, mask, frame, out, 17)
    assert tuple(got[0].shape) == (256, 320, 320) and int(got[4].cpu()) == 0


# ------------------------------------------------------------------------------------------------------------ accounting
def header_symbols():
    """The same parse as test_abi.header_symbols, on include/cfun_sample_lits.h."""
    txt = open(os.path.join(ROOT, "include", "cfun_sample_lits.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(cfun_[a-z0-9_]+)\s*\(", txt)))


NO_LAUNCH = {"cfun_sample_lits_workspace_bytes": "host-side query: launches nothing, touches no device memory"}


def check_coverage(tier):
    from cfun_amd import _lib
    assert header_symbols() == sorted(_lib.LITS_SAMPLE_EXPORTS)
    for other in (_lib.EXPORTS, _lib.SAMPLE_EXPORTS):
        assert not set(_lib.LITS_SAMPLE_EXPORTS) & set(other)
    missed = sorted(set(_lib.LITS_SAMPLE_EXPORTS) - set(NO_LAUNCH) - guard.SEEN[tier])
    assert not missed, "LiTS sample entries that launch work but never ran under guard: %s" % missed
