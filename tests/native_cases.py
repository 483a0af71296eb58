"""Cases of the native-grid tier (cfun_amd.native; k_mold_native, k_map_tile and k_map_plain in cfun_amd/csrc/native.hip) shared
by test_native_emu.py and test_native_gpu.py: the device against tests/native_ref.py.  Both sides run the header's double
operations in the header's order, so every float32 bit of the molded volume and every byte of the map must be equal."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import guard
import native_ref as nr
from conftest import ROOT

EINVAL = -1
INT16, FLOAT32, FLOAT64 = 0, 1, 2
KIND = {np.dtype(np.int16): INT16, np.dtype(np.float32): FLOAT32, np.dtype(np.float64): FLOAT64}


def tile_constants():
    """The tile constants as cfun_amd/csrc/native.hip states them; the shapes below are derived from these values."""
    txt = open(os.path.join(ROOT, "cfun_amd", "csrc", "native.hip")).read()
    m = re.search(r"constexpr int kMY = (\d+), kMX = (\d+), kMZ = (\d+), kMPitch = (\d+);", txt)
    b = re.search(r"constexpr int kBA = (\d+), kBB = (\d+), kBPitch = (\d+);", txt)
    assert m and b, "native.hip no longer states its tile constants in one line each"
    return tuple(int(v) for v in m.groups()), tuple(int(v) for v in b.groups())


(MY, MX, MZ, MPITCH), (BA, BB, BPITCH) = tile_constants()
assert (MY, MX, MZ, MPITCH) == (64, 64, 4, 65), "the mold tile changed: re-derive the sweeps below from the new constants"
assert (BA, BB, BPITCH) == (128, 128, 132), "the byte tile changed: re-derive MAP_EDGES below from the new constants"
# one below, at and one above the tile; 2 * tile + 2 is three tiles, ragged, and not a multiple of 4 (the scalar store path);
# MX - 4 / MX / 2 * MX are multiples of 4 (the 16-byte store path), MX - 1 / MX + 1 are not
W_OUT = [MX - 4, MX - 1, MX, MX + 1, 2 * MX, 2 * MX + 2]
H_OUT = [MY - 1, MY, MY + 1, 2 * MY + 2]
D_OUT = [1, MZ - 1, MZ, MZ + 1, 2 * MZ + 1]
# (source, resampled, frame, output), each (H, W, D)
W_CASES = [((6, 40, 5), (7, 50, 6), (9, 60, 7), (5, w, 3)) for w in W_OUT]
H_CASES = [((40, 6, 5), (50, 7, 6), (60, 9, 7), (h, 8, 3)) for h in H_OUT]
D_CASES = [((6, 7, 20), (7, 9, 26), (9, 12, 30), (5, 8, d)) for d in D_OUT]
# n / R below, at and above 1 on each axis separately (the other two axes keep n == R)
RATIO_CASES = [(tuple(20 if k == ax else 9 for k in range(3)), tuple(r if k == ax else 9 for k in range(3)), (36, 36, 36), (17, 20, 13))
               for ax in range(3) for r in (14, 20, 33)]


def _rng(seed):
    return np.random.default_rng(seed)


def hu(shape, seed, dtype=np.int16):
    rng = _rng(seed)
    if np.dtype(dtype) == np.int16:
        return rng.integers(-1024, 1500, shape).astype(np.int16)       # both clamps of the window and its open interval
    return rng.normal(0.0, 350.0, shape).astype(dtype)


def fortran(arr, device):
    """The array on the device with H fastest: what nifti.load's reshape(order='F') gives."""
    t = torch.from_numpy(np.ascontiguousarray(arr.transpose(2, 1, 0))).to(device).permute(2, 1, 0)
    assert t.stride()[0] == 1
    return t


# ------------------------------------------------------------------------------------------------------------- the mold pass
def raw_mold(device, t_src, dims, resampled, frame, off, out, clip=None, norm=1, kind=None, null=None, margin=64):
    """cfun_mold_native called directly, the output inside a larger buffer with ``margin`` canary elements either side.
    Returns (rc, output view, buffer, buffer as it was before the call)."""
    from cfun_amd import _lib, ops
    lib = _lib.load()
    n = min(max(1, abs(int(np.prod([float(v) for v in out])))), 1 << 22)
    buf = torch.full((n + 2 * margin,), -7.0, dtype=torch.float32, device=device)
    view = buf[margin:margin + n]
    before = buf.cpu().clone()
    i64, i32 = C.c_int64 * 3, C.c_int32 * 3
    clip_t = torch.tensor([float(clip[0]), float(clip[1])], dtype=torch.float64, device=device) if clip is not None else None
    p = dict(src=ops.ptr_raw(t_src), src_strides=i64(*t_src.stride()), dims=i32(*dims), resampled=i32(*resampled), frame=i32(*frame),
             offset=i32(*off), out_dims=i32(*out), out=_lib.ptr(view))
    if null:
        p[null] = None
    rc = lib.cfun_mold_native(p["src"], p["src_strides"], KIND[np.dtype(str(t_src.dtype).split(".")[1])] if kind is None else kind,
                              p["dims"], p["resampled"], p["frame"], p["offset"], p["out_dims"], _lib.ptr(clip_t), norm, p["out"],
                              _lib.stream(t_src))
    return rc, view, buf, before


def canaries_intact(buf, before, margin=64):
    now = buf.cpu()
    assert torch.equal(now[:margin], before[:margin]) and torch.equal(now[-margin:], before[-margin:]), "canary"


def check_mold(device, src, resampled, frame, out, clip="range", norm=True, t_src=None, off=None, planes=None):
    """src: numpy [H,W,D]; t_src: the (possibly strided) device view holding the same values (default: Fortran order)."""
    t = fortran(src, device) if t_src is None else t_src
    rng_clip = (np.float64(src.min()), np.float64(src.max())) if isinstance(clip, str) else clip
    off = nr.offsets(frame, resampled) if off is None else off
    rc, view, buf, before = raw_mold(device, t, src.shape, resampled, frame, off, out, rng_clip, int(norm))
    assert rc == 0, rc
    canaries_intact(buf, before)
    got = view.reshape(out[2], out[0], out[1]).cpu()
    want = nr.mold_native(src, resampled, frame, out, rng_clip, norm, off, planes)
    if planes is not None:
        got = got[planes]
    diff = got.view(torch.int32) != torch.from_numpy(want).view(torch.int32)
    assert not diff.any(), "%d of %d voxels differ in bits: %s -> %s -> frame %s -> %s" % (int(diff.sum()), diff.numel(), src.shape,
                                                                                         resampled, frame, out)
    return got


def check_mold_sweep(device, quad):
    shape, resampled, frame, out = quad
    check_mold(device, hu(shape, sum(out)), resampled, frame, out)


def check_mold_ratios(device):
    for quad in RATIO_CASES:
        check_mold_sweep(device, quad)


def check_mold_extents_of_one(device):
    """R = 1 and n = 1 extents on every axis, and all of them at once."""
    for ax in range(3):
        n = tuple(1 if k == ax else 7 for k in range(3))
        big = tuple(5 if k == ax else 9 for k in range(3))
        check_mold(device, hu(n, 30 + ax), big, (12, 12, 12), (11, 8, 9))                 # n = 1: every output is 0.5 .. 1 of it
        check_mold(device, hu((7, 8, 9), 33 + ax), tuple(1 if k == ax else 9 for k in range(3)), (12, 12, 12), (11, 8, 9))   # R = 1
    check_mold(device, hu((1, 1, 1), 36), (1, 1, 1), (1, 1, 1), (1, 1, 1))
    check_mold(device, hu((1, 1, 1), 37), (3, 2, 4), (5, 5, 5), (6, 4, 7))


def check_mold_frame_fill_and_parity(device):
    """A resampled volume that fills the frame, one of a few voxels inside it, and both parities of P - R on every axis."""
    src = hu((12, 10, 8), 40)
    check_mold(device, src, (15, 13, 11), (15, 13, 11), (9, 12, 10))                      # fills the frame: no zero anywhere
    got = check_mold(device, src, (3, 2, 2), (40, 41, 39), (30, 32, 28), norm=False)
    assert int((got != 0).sum()) <= 3 * 2 * 2 * 2 and (got != 0).any()                    # a few voxels in a zero frame
    for p in ((19, 17, 15), (20, 18, 16)):                                                # P - R = 4, 4, 4 and 5, 5, 5
        check_mold(device, src, (15, 13, 11), p, (16, 20, 12))
    check_mold(device, src, (15, 13, 11), (20, 18, 16), (16, 20, 12), off=(5, 5, 5))      # pushed against the far faces
    check_mold(device, src, (15, 13, 11), (20, 18, 16), (16, 20, 12), off=(0, 0, 0))


def check_mold_dtypes_and_orders(device):
    """int16, float32 and float64 sources; Fortran (the fast tile's order), C order, a sliced view and an offset view."""
    quad = ((22, 19, 9), (29, 17, 14), (33, 20, 15), (21, 24, 10))
    shape, resampled, frame, out = quad
    for dt in (np.int16, np.float32, np.float64):
        src = hu(shape, 50, dt)
        check_mold(device, src, resampled, frame, out)                                    # Fortran
        tc = torch.from_numpy(src).to(device)
        assert tc.stride()[2] == 1
        check_mold(device, src, resampled, frame, out, t_src=tc)                          # C order: D fastest
    big = hu((26, 41, 14), 51)
    sl = (slice(2, 24), slice(1, 39, 2), slice(3, 12))
    tv = torch.from_numpy(big).to(device)[sl]
    assert not tv.is_contiguous() and tuple(tv.shape) == shape
    check_mold(device, np.ascontiguousarray(big[sl]), resampled, frame, out, t_src=tv)    # a sliced C-ordered view
    tf = fortran(big, device)[sl]
    assert tf.stride()[0] == 1 and tf.storage_offset() > 0
    check_mold(device, np.ascontiguousarray(big[sl]), resampled, frame, out, t_src=tf)    # a sliced, offset Fortran view


def check_mold_clip_and_normalise(device):
    """clip NULL, inactive (a range wider than every blend) and active (all-positive source: the faces blend below the minimum;
    and a range narrower than the data); normalise on and off for each."""
    quad = ((14, 12, 9), (19, 10, 13), (22, 14, 15), (22, 14, 15))         # output = frame: every resampled voxel is picked, faces too
    shape, resampled, frame, out = quad
    pos = _rng(60).integers(100, 260, shape).astype(np.int16)
    raw = nr.resample(pos, resampled)
    assert (raw < pos.min()).any(), "test setup: the clip does not act"
    for norm in (True, False):
        a = check_mold(device, pos, resampled, frame, out, clip=None, norm=norm)
        b = check_mold(device, pos, resampled, frame, out, clip=(-5000.0, 5000.0), norm=norm)
        c = check_mold(device, pos, resampled, frame, out, clip="range", norm=norm)
        d = check_mold(device, pos, resampled, frame, out, clip=(150.0, 200.0), norm=norm)
        assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(c, d)
    # normalisation off and no clip: the float32 of the blend itself; equal extents copy the voxel
    src = hu((9, 8, 7), 61)
    got = check_mold(device, src, src.shape, src.shape, src.shape, clip=None, norm=False)
    assert torch.equal(got, torch.from_numpy(src.astype(np.float32)).permute(2, 0, 1))
    got = check_mold(device, np.full((2, 2, 1), 0, np.int16), (2, 2, 1), (4, 4, 1), (4, 4, 1))
    assert got[0, 1:3, 1:3].tolist() == [[0.5, 0.5], [0.5, 0.5]] and float(got.sum()) == 2.0      # the frame's zero is not normalised


def check_mold_non_finite(device):
    """A float32 source with a NaN and an inf planted: they spread to every output whose taps touch them -- also through a
    weight of 0 -- and nowhere else."""
    shape, resampled, frame, out = (10, 9, 6), (14, 13, 9), (16, 14, 10), (16, 14, 10)
    src = hu(shape, 70, np.float32)
    src[3, 4, 2], src[7, 2, 4] = np.nan, np.inf
    want = nr.mold_native(src, resampled, frame, out, None, False)
    assert np.isnan(want).sum() > 1 and np.isinf(want).sum() > 1
    got = check_mold(device, src, resampled, frame, out, clip=None, norm=False)
    assert torch.equal(torch.isnan(got), torch.from_numpy(np.isnan(want)))
    check_mold(device, src, resampled, frame, out, clip=(-500.0, 500.0), norm=True)       # the NaN survives clip and clamp
    check_mold(device, src, shape, shape, shape, clip=None, norm=False)                   # n == R: weights of exactly 0 and 1


def check_mold_repeatable(device):
    quad = ((33, 30, 12), (41, 38, 19), (44, 40, 21), (70, 68, 9))
    shape, resampled, frame, out = quad
    src = hu(shape, 80)
    a = check_mold(device, src, resampled, frame, out)
    b = check_mold(device, src, resampled, frame, out)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def check_mold_refusals(device):
    """Every refusal of the header: the return code, and nothing written -- the output and the canaries either side of it."""
    shape, resampled, frame, off, out = (10, 12, 5), (12, 13, 6), (14, 15, 6), (1, 1, 0), (9, 8, 4)
    src = hu(shape, 90)
    t = fortran(src, device)
    rc, view, buf, before = raw_mold(device, t, shape, resampled, frame, off, out, (src.min(), src.max()))
    assert rc == 0
    canaries_intact(buf, before)
    big = 2 ** 31 - 1
    bad = [dict(frame=(11, 15, 6)), dict(frame=(14, 15, 5)),             # the resampled volume is larger than the frame
           dict(off=(3, 1, 0)), dict(off=(1, 3, 0)), dict(off=(1, 1, 1)),    # ... or does not fit at the offset
           dict(off=(-1, 1, 0)),
           dict(out=(0, 8, 4)), dict(out=(9, -1, 4)), dict(out=(9, 8, 0)), dict(frame=(14, 0, 6)),
           dict(resampled=(0, 13, 6)), dict(resampled=(12, 13, -2)), dict(dims=(10, 0, 5)), dict(dims=(-1, 12, 5)),
           dict(out=(big, big, big)),                                     # more tiles than one grid axis numbers
           dict(kind=3), dict(kind=-1)] + \
          [dict(null=k) for k in ("src", "src_strides", "dims", "resampled", "frame", "offset", "out_dims", "out")]
    for kw in bad:
        args = dict(dims=shape, resampled=resampled, frame=frame, off=off, out=out)
        args.update(kw)
        rc, view, buf, before = raw_mold(device, t, args.pop("dims"), args.pop("resampled"), args.pop("frame"), args.pop("off"),
                                         args.pop("out"), (0.0, 1.0), **args)
        assert rc == EINVAL, (kw, rc)
        assert torch.equal(buf.cpu(), before), kw


# ------------------------------------------------------------------------------------------------------------- the byte pass
# (source, output) as (H, W, D): the tile's a axis is the output's unit-stride axis (H' in Fortran order), b the source's (W)
MAP_EDGES = [((100, 150, 3), (h, w, 2)) for h, w in ((BA - 1, BB + 1), (BA, BB), (BA + 1, BB - 1), (2 * BA + 3, 30), (30, 2 * BB + 3))] + \
            [((150, 100, 2), (BA + 1, BB + 1, 3)), ((300, 290, 2), (BA - 1, BB - 1, 1))]


def rich_map(shape_hwd, seed):
    """A [D,H,W] uint8 map with every byte value, the high ones included."""
    h, w, d = shape_hwd
    return _rng(seed).integers(0, 256, (d, h, w)).astype(np.uint8)


def check_map(device, shape, out, seed=0):
    """native.map_resize in both output orders against the restatement."""
    from cfun_amd import native
    cmap = rich_map(shape, seed)
    want = nr.map_resize(cmap.transpose(1, 2, 0), out)
    t = torch.from_numpy(cmap).to(device)
    for order in (True, False):
        got = native.map_resize(t, out, fortran=order)
        assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(out)
        assert got.stride() == ((1, out[0], out[0] * out[1]) if order else (out[1] * out[2], out[2], 1))
        assert torch.equal(got.cpu(), torch.from_numpy(want)), (shape, out, order)
    assert (want >= 128).any()


def check_map_edges(device, pair):
    check_map(device, pair[0], pair[1], sum(pair[1]))


def check_map_extents_of_one(device):
    for shape, out in (((1, 9, 7), (5, 9, 7)), ((9, 1, 7), (9, 4, 7)), ((9, 7, 1), (9, 7, 3)), ((9, 7, 5), (1, 7, 5)),
                       ((9, 7, 5), (9, 1, 5)), ((9, 7, 5), (9, 7, 1)), ((1, 1, 1), (1, 1, 1)), ((1, 1, 1), (3, 2, 4)), ((6, 5, 4), (1, 1, 1))):
        check_map(device, shape, out, 3)


def raw_map(device, t_src, dims, t_out_base, out_strides, out_dims, null=None):
    from cfun_amd import _lib, ops
    lib = _lib.load()
    i64, i32 = C.c_int64 * 3, C.c_int32 * 3
    p = dict(src=ops.ptr_raw(t_src), src_strides=i64(*t_src.stride()), dims=i32(*dims), out=_lib.ptr(t_out_base),
             out_strides=i64(*out_strides), out_dims=i32(*out_dims))
    if null:
        p[null] = None
    return lib.cfun_map_resize(p["src"], p["src_strides"], p["dims"], p["out"], p["out_strides"], p["out_dims"], _lib.stream(t_src))


def check_map_strides(device):
    """Stride pairs the wrapper does not produce: a Fortran source into a Fortran output (both unit strides on H: the plain
    form), a sliced source, an output with padded rows and planes (odd pitches: the byte-store path of the tile; untouched
    padding), and an output axis of stride 1 with a unit-stride source axis elsewhere (the tile turned onto other axes)."""
    shape, out = (37, 150, 5), (BA + 5, 140, 4)
    src = _rng(5).integers(0, 256, shape).astype(np.uint8)
    want = torch.from_numpy(nr.map_resize(src, out))
    margin = 64

    def run(t_src, strides, span):
        base = torch.full((span + 2 * margin,), 201, dtype=torch.uint8, device=device)
        body = base[margin:margin + span]
        assert raw_map(device, t_src, shape, body, strides, out) == 0
        got = torch.as_strided(body.cpu(), out, strides)
        assert torch.equal(got, want), strides
        touched = torch.zeros(span, dtype=torch.bool)
        torch.as_strided(touched, out, strides).fill_(True)
        assert (body.cpu()[~touched] == 201).all() and (base.cpu()[:margin] == 201).all() and (base.cpu()[-margin:] == 201).all(), strides

    tc = torch.from_numpy(src).to(device)                                       # C order: D fastest
    tw = torch.from_numpy(np.ascontiguousarray(src.transpose(2, 0, 1))).to(device).permute(1, 2, 0)     # W fastest: the class map
    tf = fortran(src, device)
    h, w, d = out
    for t_src in (tc, tw, tf):
        run(t_src, (1, h, h * w), h * w * d)                                    # Fortran output
        run(t_src, (w * d, d, 1), h * w * d)                                    # C output
        assert (h + 2) % 4 and not (h + 3) % 4
        run(t_src, (1, h + 2, (h + 2) * (w + 1)), (h + 2) * (w + 1) * d)        # padded, odd pitches: byte stores
        run(t_src, (1, h + 3, (h + 3) * w + 4), ((h + 3) * w + 4) * d)          # padded, pitches that are multiples of 4, H' is not
        run(t_src, (w + 2, 1, (w + 2) * h), (w + 2) * h * d)                    # W' fastest, padded
    big = _rng(6).integers(0, 256, (41, 160, 9)).astype(np.uint8)
    sl = (slice(2, 39), slice(5, 155), slice(1, 6))
    tv = torch.from_numpy(np.ascontiguousarray(big.transpose(2, 0, 1))).to(device).permute(1, 2, 0)[sl]
    assert tuple(tv.shape) == shape and tv.stride()[1] == 1 and tv.storage_offset() > 0
    want = torch.from_numpy(nr.map_resize(np.ascontiguousarray(big[sl]), out))
    run(tv, (1, h, h * w), h * w * d)                                           # a sliced, offset class map: the tile


def check_map_refusals(device):
    shape, out = (9, 12, 5), (10, 8, 6)
    src = torch.from_numpy(_rng(7).integers(0, 256, shape).astype(np.uint8)).to(device)
    h, w, d = out
    base = torch.full((h * w * d + 128,), 201, dtype=torch.uint8, device=device)
    body = base[64:64 + h * w * d]
    ok = (1, h, h * w)
    assert raw_map(device, src, shape, body, ok, out) == 0
    assert (base.cpu()[:64] == 201).all() and (base.cpu()[-64:] == 201).all()
    base.fill_(201)
    bad = [dict(dims=(0, 12, 5)), dict(dims=(9, -3, 5)), dict(out=(10, 0, 6)), dict(out=(10, 8, -1)),
           dict(strides=(0, h, h * w)), dict(strides=(1, 0, h * w)), dict(strides=(1, h, -h * w)),      # zero / negative
           dict(strides=(1, h - 1, h * w)), dict(strides=(1, h, h * w - 1)), dict(strides=(1, 1, h * w)),   # overlapping
           dict(strides=(w * d, d - 1, 1)), dict(strides=(2, 1, 2 * h))] + \
          [dict(null=k) for k in ("src", "src_strides", "dims", "out", "out_strides", "out_dims")]
    for kw in bad:
        rc = raw_map(device, src, kw.get("dims", shape), body, kw.get("strides", ok), kw.get("out", out), kw.get("null"))
        assert rc == EINVAL, (kw, rc)
        assert (base.cpu() == 201).all(), kw
    # an axis of extent 1 addresses nothing: its stride may be anything positive
    one = torch.full((h * w,), 201, dtype=torch.uint8, device=device)
    assert raw_map(device, src, shape, one, (1, h, 1), (h, w, 1)) == 0
    assert torch.equal(one.cpu().reshape(w, h).t(), torch.from_numpy(nr.map_resize(src.cpu().numpy(), (h, w, 1)))[..., 0])


# -------------------------------------------------------------------------------------------------------------- the wrappers
def check_spacing_and_shape_by_hand():
    from cfun_amd import config, native
    lits_affine = np.array([[-0.703125, 0.0, 0.0, 172.9], [0.0, -0.703125, 0.0, 179.3], [0.0, 0.0, 5.0, -368.0], [0.0, 0.0, 0.0, 1.0]])
    assert native.diag_spacing(lits_affine).tolist() == [0.703125, 0.703125, 5.0]         # negative entries, as LiTS affines have
    rot = np.array([[0.0, -1.25, 0.0, 30.0], [0.8, 0.0, 0.0, -12.0], [0.0, 0.0, 2.5, 7.0], [0.0, 0.0, 0.0, 1.0]])
    with pytest.raises(ValueError, match="zero entry"):
        native.diag_spacing(rot)                                                          # (column norms would say 0.8, 1.25, 2.5)
    mean = config.LiTSConfig.MEAN_SPACING
    assert tuple(mean) == (0.79272507, 0.79272507, 1.50625819)
    # 512 * 0.7 / 0.79272507 = 452.11 -> 452;  129 * 2.5 / 1.50625819 = 214.11 -> 214
    rs = native.resampled_shape((512, 512, 129), (0.7, 0.7, 2.5), mean)
    assert rs.dtype == np.int32 and rs.tolist() == [452, 452, 214]
    # 512 * 0.703125 / 0.79272507 = 454.13 -> 454;  75 * 5 / 1.50625819 = 248.96 -> 249
    assert native.resampled_shape((512, 512, 75), native.diag_spacing(lits_affine), mean).tolist() == [454, 454, 249]
    assert native.resampled_shape((5, 7, 3), (1.0, 1.0, 1.0), (2.0, 2.0, 2.0)).tolist() == [2, 4, 2]      # 2.5, 3.5, 1.5: half to even
    assert native.resampled_shape((10, 10, 10), mean, mean).tolist() == [10, 10, 10]


def lits_config():
    import module_cases as mc
    cfg = mc.tiny_lits_config("together", max_dim=64, min_dim=32)
    cfg.PAD_IMAGE_SHAPE = [80, 80, 40]
    return cfg


def check_mold_inputs_native(device):
    """Window and meta equal utils.mold_inputs_lits' on the materialised resampled volume; the molded tensor equals the restated
    one bit for bit; the upload keeps dtype and order; an oversized volume raises."""
    from cfun_amd import native, utils
    cfg = lits_config()
    frame = cfg.PAD_IMAGE_SHAPE
    out = tuple(int(v) for v in cfg.IMAGE_SHAPE[:3])
    spacing = (1.0, 0.9, 2.6)
    for dt, order in ((np.int16, "F"), (np.float32, "C"), (np.float64, "F"), (np.int32, "F"), (np.uint16, "C")):
        base = hu((36, 44, 12), 100).astype(np.int32) + (1024 if dt == np.uint16 else 0)
        src = np.asarray(base.astype(dt), order=order)
        up = native._upload(src, torch.device(device))
        assert up.dtype == {np.int16: torch.int16, np.float32: torch.float32}.get(dt, torch.float64)
        assert up.stride() == ((1, 36, 36 * 44) if order == "F" else (44 * 12, 12, 1))
        molded, metas, windows, rs = native.mold_inputs_native(cfg, src, spacing, device=device)
        assert rs.tolist() == [45, 50, 21] == native.resampled_shape(src.shape, spacing, cfg.MEAN_SPACING).tolist()
        want = nr.mold_native(src, rs, frame, out)
        assert tuple(molded.shape) == (1, 1, out[2], out[0], out[1]) and molded.dtype == torch.float32
        assert torch.equal(molded[0, 0].cpu().view(torch.int32), torch.from_numpy(want).view(torch.int32)), dt
        stored = nr.resample(src, rs, (src.min(), src.max())).astype(np.float32)          # what preprocessing.py would have saved
        _, r_metas, r_windows = utils.mold_inputs_lits(cfg, [stored], device=device)
        assert np.array_equal(metas, r_metas) and np.array_equal(windows, r_windows)
    with pytest.raises(ValueError, match="does not fit PAD_IMAGE_SHAPE"):
        native.mold_inputs_native(cfg, src, (3.0, 0.9, 2.6), device=device)
    with pytest.raises(ValueError, match="volume expected"):
        native.mold_inputs_native(cfg, src[..., None], spacing, device=device)


NATIVE_AFFINE = np.array([[-1.0, 0.0, 0.0, 30.0], [0.0, 0.9, 0.0, -12.0], [0.0, 0.0, 2.6, 7.0], [0.0, 0.0, 0.0, 1.0]])


def native_case(seed, shape=(36, 44, 12)):
    """A synthetic scan on its own grid: int16 HU in NIfTI (Fortran) order."""
    return np.asfortranarray(_rng(seed).normal(0.0, 200.0, shape).astype(np.int16))


def check_detect_native(device):
    """detect_native's maps equal the shared detect helper fed the RESTATED molded tensor; mask_native is the order-0 resize of
    the resampled-grid map to the image's own shape."""
    import eval_cases as ec
    from oracle import cfun_oracle as orc
    from cfun_amd import evaluate, native
    cfg = lits_config()
    net = ec._net(device, cfg, 2)
    image = native_case(9)
    res = native.detect_native(net, image, NATIVE_AFFINE)
    rs = native.resampled_shape(image.shape, native.diag_spacing(NATIVE_AFFINE), cfg.MEAN_SPACING)
    assert res["resampled_shape"] == tuple(rs.tolist()) == (45, 50, 21)
    assert not res["empty"] and res["mask_device"].any(), "test setup: no detection / an all-zero map"
    out = tuple(int(v) for v in cfg.IMAGE_SHAPE[:3])
    molded = torch.from_numpy(nr.mold_native(image, rs, cfg.PAD_IMAGE_SHAPE, out)).to(device)[None, None]
    _, _, windows, _ = native.mold_inputs_native(cfg, image, native.diag_spacing(NATIVE_AFFINE), device=device)
    ref = evaluate.detect_molded(net, molded, tuple(float(v) for v in windows[0]), rs.tolist())
    assert tuple(res["mask_device"].shape) == (21, 45, 50) and res["mask_device"].dtype == torch.uint8
    assert torch.equal(res["mask_device"], ref["mask_device"])
    for k in ("rois", "class_ids", "scores"):
        assert np.array_equal(np.asarray(res[k]), np.asarray(ref[k])), k
    native_map = res["mask_native"]
    assert native_map.dtype == torch.uint8 and tuple(native_map.shape) == image.shape and native_map.stride() == (1, 36, 36 * 44)
    want = orc.skimage_resize(res["mask_device"].permute(1, 2, 0).cpu().numpy(), image.shape, 0)
    assert np.array_equal(native_map.cpu().numpy(), want)
    # a postprocess runs on the resampled grid, before the way back
    from cfun_amd import components
    post = native.detect_native(net, image, NATIVE_AFFINE, postprocess=components.Postprocess())
    assert torch.equal(post["mask_device_raw"], res["mask_device"]) and "component_stats" in post
    assert np.array_equal(post["mask_native"].cpu().numpy(), orc.skimage_resize(post["mask_device"].permute(1, 2, 0).cpu().numpy(), image.shape, 0))


def check_predict_for_submit(device, tmp_path):
    """Two synthetic cases written with nifti.save (anisotropic spacing, one with negative diagonal entries): the files read back
    with the native shape, uint8, the image's affine, the bytes of mask_native and the reference's names."""
    import eval_cases as ec
    from cfun_amd import native, nifti
    cfg = lits_config()
    net = ec._net(device, cfg, 2)
    src_dir, out_dir = os.path.join(str(tmp_path), "imagesTs"), os.path.join(str(tmp_path), "submissions")
    os.makedirs(src_dir)
    aff2 = np.diag([0.85, 1.1, 2.2, 1.0])
    aff2[:3, 3] = (-100.0, 55.0, 3.0)
    specs = [("test-volume-3.nii", native_case(9), NATIVE_AFFINE), ("test-volume-12.nii.gz", native_case(10, (40, 38, 14)), aff2)]
    paths = []
    for name, arr, aff in specs:
        paths.append(os.path.join(src_dir, name))
        nifti.save(nifti.Nifti1Image(arr, aff), paths[-1])
    saved, results = native.predict_for_submit(net, paths, out_dir)
    assert [os.path.basename(p) for p in saved] == ["test-segmentation-3.nii", "test-segmentation-12.nii"]
    assert sorted(os.listdir(out_dir)) == ["test-segmentation-12.nii", "test-segmentation-3.nii"]
    nonzero = 0
    for path, res, (_, arr, aff) in zip(saved, results, specs):
        back = nifti.load(path)
        data = back.get_data()
        assert data.shape == arr.shape and data.dtype == np.uint8
        np.testing.assert_allclose(back.affine, aff, rtol=0, atol=1e-6)
        assert np.array_equal(data, res["mask_native"].cpu().numpy())
        nonzero += int(data.any())
    assert nonzero >= 1, "test setup: every case gave an all-zero map"
    # tuples, a limit, positions as numbers; a case without detections writes zeros
    cfg.DETECTION_MIN_CONFIDENCE = 1.5
    saved, results = native.predict_for_submit(net, [(specs[0][1], specs[0][2]), (specs[1][1], specs[1][2], "liver_41")],
                                               os.path.join(out_dir, "b"), limit=2)
    assert [os.path.basename(p) for p in saved] == ["test-segmentation-0.nii", "test-segmentation-41.nii"]
    assert all(r["empty"] for r in results)
    back = nifti.load(saved[1]).get_data()
    assert back.shape == (40, 38, 14) and back.dtype == np.uint8 and not back.any()


# ---------------------------------------------------------------------------------------------------------- the bench shape
def check_bench_shape(device):
    """GPU only: 512x512x129 int16 Fortran at spacing (0.70, 0.70, 2.5) -> 452x452x214 -> 256x320x320, compared on the first
    slab, the last slab and three seeded z slabs of the restatement; the byte pass 214x452x452 -> 512x512x129 whole."""
    from cfun_amd import config, native
    cfg = config.LiTSConfig("together")
    shape = (512, 512, 129)
    rng = _rng(110)
    src = np.asfortranarray(rng.integers(-1024, 1500, shape, dtype=np.int16))
    rs = native.resampled_shape(shape, (0.70, 0.70, 2.5), cfg.MEAN_SPACING)
    assert rs.tolist() == [452, 452, 214]
    molded, _, _, _ = native.mold_inputs_native(cfg, src, (0.70, 0.70, 2.5), device=device)
    assert tuple(molded.shape) == (1, 1, 256, 320, 320)
    # the first and the last slab are the frame's zeros (214 of 536 planes are the volume's); the seeded three are drawn from
    # the output planes the volume reaches, so that they compare blends
    rz = nr.frame_index(256, 536) - nr.offsets(cfg.PAD_IMAGE_SHAPE, rs)[2]
    reached = np.flatnonzero((rz >= 0) & (rz < 214))
    assert 90 < reached.size < 110
    planes = sorted({0, 255} | set(int(v) for v in rng.choice(reached, 3, replace=False)))
    want = nr.mold_native(src, rs, cfg.PAD_IMAGE_SHAPE, (320, 320, 256), planes=planes)
    got = molded[0, 0][planes].cpu()
    assert torch.equal(got.view(torch.int32), torch.from_numpy(want).view(torch.int32))
    assert all((want[i] != 0).any() for i in (1, 2, 3)) and not want[0].any() and not want[-1].any()
    cmap = torch.from_numpy(rng.integers(0, 3, (214, 452, 452), dtype=np.uint8)).to(device)
    back = native.map_resize(cmap, shape)
    assert back.stride() == (1, 512, 512 * 512)
    assert np.array_equal(back.cpu().numpy(), nr.map_resize(cmap.cpu().numpy().transpose(1, 2, 0), shape))


# ------------------------------------------------------------------------------------------------------------ accounting
def header_symbols():
    """The same parse as test_abi.header_symbols, on include/cfun_native.h."""
    txt = open(os.path.join(ROOT, "include", "cfun_native.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(cfun_[a-z0-9_]+)\s*\(", txt)))


def check_coverage(tier):
    from cfun_amd import _lib
    assert header_symbols() == sorted(_lib.NATIVE_EXPORTS) == ["cfun_map_resize", "cfun_mold_native"]
    for other in (_lib.EXPORTS, _lib.SAMPLE_EXPORTS, _lib.LITS_SAMPLE_EXPORTS, _lib.TILE_EXPORTS, _lib.EVAL_EXPORTS, _lib.CC_EXPORTS,
                  _lib.SURFACE_EXPORTS, _lib.LESION_EXPORTS, _lib.FILL_EXPORTS, _lib.MORPH_EXPORTS):
        assert not set(_lib.NATIVE_EXPORTS) & set(other)
    missed = sorted(set(_lib.NATIVE_EXPORTS) - guard.SEEN[tier])
    assert not missed, "native-grid entries that never ran under guard: %s" % missed
