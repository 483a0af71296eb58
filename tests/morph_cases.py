"""Cases of the ball morphology (cfun_amd/morphology.py, cfun_amd/csrc/morph.hip) shared by test_morph_emu.py and
test_morph_gpu.py: the device against tests/morph_ref.py (scipy with the float32-built ball), everything an integer and compared
with torch.equal, nothing excluded -- the map and both columns of the statistics."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import cc_ref as cr
import eval_cases as ec
import fill_cases as fc
import guard
import morph_ref as mr
import test_morph_ref as hand
from conftest import ROOT


def kernel_constants():
    """(kNT, kMaxDim, kSlabBytes, kMaxLines) as cfun_amd/csrc/morph.hip declares them."""
    txt = open(os.path.join(ROOT, "cfun_amd", "csrc", "morph.hip")).read()
    vals = []
    for name in ("kNT", "kMaxDim", "kSlabBytes", "kMaxLines"):
        m = re.search(r"constexpr int %s = (\d+);" % name, txt)
        assert m, "morph.hip no longer declares %s" % name
        vals.append(int(m.group(1)))
    return tuple(vals)


# The shapes are what they are because of morph.hip's slabs.  The x sweep takes kSlabBytes // W whole rows per workgroup; the y
# and z sweeps take whole lines, pow2_floor(min(kMaxLines, slab cells // L)) columns wide, one byte a cell (two when a reach is
# above 254).  A changed constant fails here, before any case runs.
NT, MAX_DIM, SLAB, LINES = kernel_constants()
assert (NT, MAX_DIM, SLAB, LINES) == (256, 4096, 32768, 128)
SHAPES = [
    (1, 1, 1),                                 # one voxel
    (1, 1, LINES + 3),                         # extent 1 along z and y; a second, ragged slab of columns
    (1, 7, 1), (6, 1, 1),                      # extent 1 along the other pairs of axes
    (9, 12, 17),                               # the shape the definition was checked on: odd W, several rows per slab
    (3, 5, 2 * LINES + 3),                     # three slabs of columns, the last 3 wide
    (2, 5, MAX_DIM),                           # a row fills an eighth of the x slab exactly: 8 rows, then a ragged slab of 2
    (1, SLAB // LINES, LINES + 2),             # a y slab filled exactly (256 x 128 cells), then one 2 columns wide
    (SLAB // LINES + 1, 2, 3),                 # z lines of 257: the slab narrows to 64 columns
]
assert SHAPES == [(1, 1, 1), (1, 1, 131), (1, 7, 1), (6, 1, 1), (9, 12, 17), (3, 5, 259), (2, 5, 4096), (1, 256, 130), (257, 2, 3)]
BIG = (64, 72, 130)                                        # GPU tier only, as cc_cases.BIG: 599 040 voxels
LITS = hand.LITS
# (spacing, radius): "<=" against "<" where r^2 is a sum of spacing squares exactly (1, sqrt 2 as the double's square rounds to
# 2, 2, 3); 1.5 as a safe value between two; the LiTS ball of 119 offsets; r < sz, where the z sweep is not launched; the two
# anisotropies; a ball larger than whole dimensions of the small shapes
BALLS = [((1.0, 1.0, 1.0), 1.0), ((1.0, 1.0, 1.0), 1.5), ((1.0, 1.0, 1.0), math.sqrt(2)), ((1.0, 1.0, 1.0), 2.0),
         ((1.0, 1.0, 1.0), 3.0), (LITS, 3.0), (LITS, 1.0), ((0.5, 0.5, 1.5), 1.6), ((5.0, 1.0, 1.0), 3.0), ((1.0, 1.0, 1.0), 13.0)]
assert [int(mr.ball(s, r).sum()) for s, r in BALLS[:9]] == [7, 19, 19, 33, 123, 119, 5, 47, 29]
assert mr.ball(LITS, 1.0).shape[0] == 1 and mr.ball((5.0, 1.0, 1.0), 3.0).shape[0] == 1           # no reach along z
SLAB_BALLS = (0, 4, 5, 6, 8)                                # r = 1 and 3 in voxels, LiTS at 3 mm and at 1 mm, no reach along z
MODES = ("class", "foreground")
WAYS = [(by, outside) for by in MODES for outside in (0, 1)]


@functools.lru_cache(maxsize=None)
def _reference(key, k, op, radius, spacing, by, classes, outside, fill_value):
    """morph_ref.morph of a registered map, computed once and shared by the plain and the guarded copy of a case; read-only."""
    out, stats = mr.morph(_MAPS[key], k, op, radius, spacing, by, classes, outside, fill_value)
    out.setflags(write=False)
    stats.setflags(write=False)
    return out, stats


_MAPS = {}


def reference(pred, k, op, radius, spacing, by, classes=None, outside=None, fill_value=1):
    key = (pred.shape, pred.tobytes())
    _MAPS.setdefault(key, pred.copy())
    return _reference(key, k, op, float(radius), tuple(float(v) for v in spacing), by, classes, outside, fill_value)


def check_case(device, pred, k, op, radius, spacing=(1.0, 1.0, 1.0), by="class", classes=None, outside=None, fill_value=1):
    """One map through morph against morph_ref; returns (map, stats) of the device as numpy arrays."""
    from cfun_amd import morphology
    pred = np.ascontiguousarray(pred)
    t = torch.from_numpy(pred.copy()).to(device)
    want, want_stats = reference(pred, k, op, radius, spacing, by, classes, outside, fill_value)
    tag = "%s k %d %s r %r spacing %s %s classes %s outside %s value %d" % (pred.shape, k, op, radius, spacing, by, classes, outside,
                                                                           fill_value)
    out, stats = morphology.morph(t, k, op, radius, spacing, by, classes, outside, fill_value)
    assert out.dtype == torch.uint8 and tuple(out.shape) == pred.shape and stats.dtype == torch.int64 and tuple(stats.shape) == (k, 2)
    assert out.device == t.device and stats.device == t.device and out.data_ptr() != t.data_ptr()
    assert torch.equal(stats.cpu(), torch.from_numpy(want_stats.copy())), "stats: %s\n%s\n%s" % (tag, stats.cpu(), want_stats)
    assert torch.equal(out.cpu(), torch.from_numpy(want.copy())), "map: " + tag
    assert torch.equal(t.cpu(), torch.from_numpy(pred)), "the input was written to: " + tag
    got = out.cpu().numpy()
    if op in ("dilate", "close"):
        assert np.array_equal(got[pred != 0], pred[pred != 0]), "a non-zero byte was rewritten: " + tag
    else:
        assert np.array_equal(got[got != 0], pred[got != 0]), "a byte was set: " + tag
    return got, stats.cpu().numpy()


def check_all_ways(device, pred, k, radius, spacing=(1.0, 1.0, 1.0), fill_value=1):
    for op in mr.OPS:
        for by, outside in WAYS:
            check_case(device, pred, k, op, radius, spacing, by, None, outside, fill_value)


def clipped_ball_size(spacing, radius, shape):
    """The offsets of the ball that fit the shape at all: |d| < the extent along every axis."""
    b = mr.ball(spacing, radius)
    c = [s // 2 for s in b.shape]
    lo = [max(0, c[i] - (shape[i] - 1)) for i in range(3)]
    return int(b[lo[0]:b.shape[0] - lo[0], lo[1]:b.shape[1] - lo[1], lo[2]:b.shape[2] - lo[2]].sum())


def bernoulli(shape, op, n, k, seed):
    """A map whose density follows from the ball's size n so that the op's result is neither empty nor full.  Dilate: seeds with
    p = 1 - 0.5^(1/n), so half of the zero voxels have none in reach.  Erode: the complement at that density.  Open and close
    act where a whole ball fits: the complement (open) or the object (close) at p = 1 - n^(-1/n), so a given ball position is
    free of it with probability 1/n and a voxel has about one such position in reach.  k == 3: a tenth of the object is class 2."""
    rng = np.random.default_rng(seed)
    p = 1.0 - 0.5 ** (1.0 / n) if op in ("erode", "dilate") else 1.0 - float(n) ** (-1.0 / n)
    sparse = rng.random(shape) < p
    obj = sparse if op in ("dilate", "close") else ~sparse
    cls = np.ones(shape, np.uint8) if k == 2 else np.where(rng.random(shape) < 0.9, 1, 2)
    return np.where(obj, cls, 0).astype(np.uint8)


def _seed(shape, i):
    return 500 + shape[0] * 31 + shape[1] * 7 + shape[2] + 1000 * i


def check_bernoulli_shape(device, shape):
    """Every ball, all four ops, both modes, both values of outside.  What a draw tests is a property of the data, asserted on the
    REFERENCE: where the volume is large enough for the density rule to mean anything (1000 voxels, and the ball clipped to the
    shape still more than the origin), between 10 % and 90 % of the voxels the op could change do change -- read as the density
    rule reads the map: the foreground as one object, and the outside of the volume as object (the borders would otherwise erode
    most of a volume only a few balls wide).  With the classes apart an erosion clears nearly everything, since a tenth of a
    class-1 voxel's neighbours is class 2; those readings are run all the same."""
    for i, (spacing, radius) in enumerate(BALLS):
        n = clipped_ball_size(spacing, radius, shape)
        voxels = shape[0] * shape[1] * shape[2]
        if radius > 4.0 and voxels > 300:
            continue                                       # the 27^3 ball is for the smallest shapes: larger than all they have
        if voxels >= 1000 and shape != (9, 12, 17) and i not in SLAB_BALLS:
            continue                                       # the float edges do not depend on the shape; the slab edges need few balls
        for op in mr.OPS:
            pred = bernoulli(shape, op, max(n, 2), 3, _seed(shape, i))
            if voxels >= 1000 and n > 1 and radius <= 4.0:
                frac = mr.changed_fraction(pred, 3, op, radius, spacing, "foreground", None, 1)
                assert 0.1 <= frac <= 0.9, "test setup: %s %s r %r on %s changes %.3f of its candidates" % (op, spacing, radius, shape, frac)
            for by, outside in WAYS:
                check_case(device, pred, 3, op, radius, spacing, by, None, outside, 5)


def blobs(shape, seed):
    """Boxes of class 1 and 2 with one-voxel spurs and one-voxel gaps, thrown across the whole volume (and so across every slab
    seam): what an opening shaves and a closing bridges."""
    rng = np.random.default_rng(seed)
    v = np.zeros(shape, np.uint8)
    for j in range(12):
        lo = [int(rng.integers(0, max(1, s - 2))) for s in shape]
        hi = [min(s, l + int(rng.integers(3, 9))) for s, l in zip(shape, lo)]
        v[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1 + j % 2
        z, y = (lo[0] + hi[0]) // 2, (lo[1] + hi[1]) // 2
        v[z, y, hi[2]:hi[2] + 4] = 1 + j % 2                          # a spur along x
        g = (lo[2] + hi[2]) // 2
        v[lo[0]:hi[0], lo[1]:hi[1], g] = 0                             # a gap plane
    return v


def check_blobs(device):
    for shape, seed in (((9, 12, 17), 1), ((3, 5, 2 * LINES + 3), 2), ((12, 20, LINES + 9), 3)):
        v = blobs(shape, seed)
        for spacing, radius in (((1.0, 1.0, 1.0), 1.0), ((1.0, 1.0, 1.0), 2.0), (LITS, 3.0), (LITS, 1.0)):
            check_all_ways(device, v, 3, radius, spacing)
        opened, s_open = check_case(device, v, 3, "open", 1.0)
        closed, s_close = check_case(device, v, 3, "close", 1.0)
        assert s_open[:, 0].sum() > 0 and s_close[:, 1].sum() > 0, "test setup: nothing shaved or nothing bridged"


def check_hand_answers(device):
    """The answers of test_morph_ref.py, on the device."""
    for r, n in ((1, 7), (1.5, 19), (1.8, 27), (2, 33)):
        got, stats = check_case(device, hand.one_voxel(), 2, "dilate", r)
        assert int(got.sum()) == n and stats.tolist() == [[0, 0], [0, n - 1]]
    got, stats = check_case(device, hand.one_voxel(), 2, "dilate", 2, (3, 1, 1))
    assert int(got.sum()) == 13 and int(got[5].sum()) == 13
    got, stats = check_case(device, hand.cube(), 2, "erode", 1)
    assert int(got.sum()) == 27 and stats.tolist() == [[0, 0], [98, 0]]
    corner = hand.cube(0, 5)
    assert int(check_case(device, corner, 2, "erode", 1, outside=0)[0].sum()) == 27
    assert int(check_case(device, corner, 2, "erode", 1, outside=1)[0].sum()) == 64
    got, stats = check_case(device, hand.spur_cube(), 2, "open", 1)
    assert int(got.sum()) == 82 and stats.tolist() == [[0, 0], [46, 0]] and got[5, 5, 8] == 1 and got[5, 5, 9] == 0
    holed = hand.cube()
    holed[5, 5, 5] = 0
    got, stats = check_case(device, holed, 2, "close", 1)
    assert np.array_equal(got, hand.cube()) and stats.tolist() == [[0, 0], [0, 1]]
    got, stats = check_case(device, hand.two_blocks(), 2, "close", 1)
    assert int(got.sum()) == 159 and stats.tolist() == [[0, 0], [0, 9]]
    for outside in (0, 1, None):
        got, stats = check_case(device, corner, 2, "close", 1, outside=outside)
        assert np.array_equal(got, corner) and not stats.any()
    for v in (hand.one_voxel(), hand.cube(), corner, hand.spur_cube(), holed, hand.two_blocks()):
        check_all_ways(device, v, 2, 1.0)


def check_priority(device):
    v = hand.nested()
    got, stats = check_case(device, v, 3, "dilate", 1)
    assert stats.tolist() == [[0, 0], [0, 6 * 81 + 44], [0, 54]] and got[4, 6, 6] == 2 and got[4, 4, 4] == 1
    got, stats = check_case(device, v, 3, "close", 1)
    assert stats.tolist() == [[0, 0], [0, 44], [0, 0]]
    for m in (v, hand.mixed()):
        for radius in (1.0, 1.5):
            check_all_ways(device, m, 3, radius)
            check_all_ways(device, m, 15, radius)
            check_all_ways(device, m, 2, radius)                       # the same map with class 2 in no group: bytes >= K
    big = np.zeros((5, 13, LINES + 8), np.uint8)                       # and across a seam of the column slabs
    big[:, :, LINES - 6:LINES + 7] = v[4:9]
    check_all_ways(device, big, 3, 1.0)
    check_all_ways(device, big, 3, 3.0, LITS)


def check_selected_classes(device):
    v = hand.nested()
    got, stats = check_case(device, v, 3, "erode", 1, classes=(2,))
    assert np.array_equal(got == 1, v == 1) and int((got == 2).sum()) == 1 and stats.tolist() == [[0, 0], [0, 0], [26, 0]]
    m = hand.mixed()
    for op in mr.OPS:
        for classes in (1, (2,), (1, 2), ()):
            got, stats = check_case(device, m, 3, op, 1.0, classes=classes)
            sel = (classes,) if isinstance(classes, int) else classes
            for c in (1, 2):
                if c not in sel:
                    assert np.array_equal(got == c, m == c) and not stats[c].any()
        got, stats = check_case(device, m, 3, op, 1.0, by="foreground", classes=(2,))          # not looked at
    wide = np.random.default_rng(3).integers(0, 15, (4, 6, 40)).astype(np.uint8)
    for op in mr.OPS:
        check_case(device, wide, 15, op, 1.0, classes=(14, 3, 7))
        check_case(device, wide, 15, op, 1.5)
        check_case(device, wide, 8, op, 1.0)                           # bytes 8 .. 14: complement, copied through
        check_case(device, wide, 1, op, 1.0)                           # no class at all: a copy
        check_case(device, wide, 1, op, 1.0, by="foreground", fill_value=200)


def check_fill_value(device):
    v = hand.nested()
    for value in (1, 7, 255):
        for op in ("dilate", "close"):
            got, stats = check_case(device, hand.two_blocks(), 2, op, 1.0, by="foreground", fill_value=value)
            assert stats[0, 1] > 0 and int(((got == value) & (hand.two_blocks() == 0)).sum()) == stats[0, 1]
            check_case(device, v, 3, op, 1.0, by="class", fill_value=value)                    # by="class" does not look at it
        check_case(device, v, 3, "erode", 1.0, by="foreground", fill_value=value)


def check_identity_and_wide_cells(device):
    """A radius below every spacing: the ball is the origin, the map is copied.  And reaches above 254, where the cells of the
    intermediate are two bytes: along x, and along z, with spacings that keep the ball one voxel thick elsewhere."""
    v = hand.mixed()
    for op in mr.OPS:
        for by in MODES:
            for spacing, r in (((1, 1, 1), 0.99), ((1.5, 0.8, 0.8), 0.79), ((1, 1, 1), 0.0)):
                got, stats = check_case(device, v, 3, op, r, spacing, by)
                assert np.array_equal(got, v) and not stats.any()
    rng = np.random.default_rng(8)
    for shape, spacing in (((2, 2, 300), (1000.0, 1000.0, 1.0)), ((300, 2, 2), (1.0, 1000.0, 1000.0))):
        assert mr.reach(1.0, mr.squares(spacing, 270.0)[1]) == 270 > 254
        for op in mr.OPS:
            sparse = rng.random(shape) < 0.004
            pred = np.where(sparse if op in ("dilate", "close") else ~sparse, 1, 0).astype(np.uint8)
            for by, outside in WAYS:
                got, stats = check_case(device, pred, 2, op, 270.0, spacing, by, None, outside)
            assert op == "close" or stats.any(), "test setup: nothing changes"


def check_repeatable(device, shape=(9, 12, 17)):
    from cfun_amd import morphology
    t = torch.from_numpy(bernoulli(shape, "erode", 33, 3, 77)).to(device)
    u = torch.from_numpy(bernoulli(shape, "dilate", 33, 3, 78)).to(device)
    for op in mr.OPS:
        for by, outside in WAYS:
            for m in (t, u):
                (o1, s1), (o2, s2) = morphology.morph(m, 3, op, 2.0, by=by, outside=outside), morphology.morph(m, 3, op, 2.0, by=by, outside=outside)
                assert torch.equal(o1, o2) and torch.equal(s1, s2)


def check_big(device):
    """GPU tier only: one case per op at 64 x 72 x 130, so that workgroups really do run at the same time."""
    n = int(mr.ball(LITS, 3.0).sum())
    for i, op in enumerate(mr.OPS):
        pred = bernoulli(BIG, op, n, 3, 40 + i)
        frac = mr.changed_fraction(pred, 3, op, 3.0, LITS, "foreground", None, 1)
        assert 0.1 <= frac <= 0.9, "test setup: %s changes %.3f of its candidates" % (op, frac)
        check_case(device, pred, 3, op, 3.0, LITS, "foreground", None, 1, 9)
        check_case(device, pred, 3, op, 3.0, LITS)
    check_repeatable(device, BIG)


# --------------------------------------------------------------------------------------------------------------- entries
def check_zero_sized_and_c_entry(device):
    """Zero-sized volumes; every refusal of the C entry with canaries either side of out and stats; a workspace one byte short."""
    from cfun_amd import _lib, morphology
    lib = _lib.load()
    for dims in ((0, 5, 7), (5, 0, 7), (5, 7, 0)):
        pred = torch.zeros(dims, dtype=torch.uint8, device=device)
        for op, by in (("erode", "class"), ("close", "foreground")):
            out, stats = morphology.morph(pred, 8, op, 2.0, by=by)
            assert tuple(out.shape) == dims and out.dtype == torch.uint8 and tuple(stats.shape) == (8, 2) and not stats.cpu().any()
        assert lib.cfun_morph_workspace_bytes(*dims, 8) == 0
    dims, k = (2, 3, 70), 8
    pred_np = np.ones(dims, np.uint8)
    pred_np[0, 1, 5] = 0
    pred = torch.from_numpy(pred_np).to(device)
    out_buf, out = fc._canary(dims, torch.uint8, device, 77)
    stats_buf, stats = fc._canary((15, 2), torch.int64, device, -7)
    need = lib.cfun_morph_workspace_bytes(*dims, k)
    assert need >= 3 * pred_np.size
    ws = _lib.workspace(need, pred)
    i32, f32 = C.c_int32 * 3, C.c_float * 3
    p, st = _lib.ptr, _lib.stream(pred)
    inf, nan = float("inf"), float("nan")

    def call(d=dims, kk=k, mode=0, op=0, classes=None, s2=(1.0, 1.0, 1.0), r2=1.0, outside=0, value=1, o=None, nbytes=None):
        bits = ((1 << kk) - 2 if 1 <= kk <= 15 else 2) if classes is None else classes
        return lib.cfun_morph_apply(p(pred), i32(*d), kk, mode, op, bits, f32(*s2), r2, outside, value, p(out if o is None else o),
                                    p(stats), p(ws), ws.numel() if nbytes is None else nbytes, st)

    bad_dims = ((2048, 1024, 1024), (1, 1 << 16, 1 << 15), (1, 1, (1 << 31) - 1), (1 << 30, 1 << 30, 1 << 30), (2, -3, 4), (-1, 0, 4),
                (1, 1, 4097), (4097, 1, 1), (1, 4097, 0))
    for d in bad_dims:
        assert call(d=d) == -1, d
        assert lib.cfun_morph_workspace_bytes(*d, k) == 0
    for kk in (0, 16, -1):
        assert call(kk=kk) == -1 and lib.cfun_morph_workspace_bytes(*dims, kk) == 0
    for mode in (2, -1):
        assert call(mode=mode) == -1
    for op in (4, -1):
        assert call(op=op) == -1
    for classes in (1, 3, 1 << k, (1 << k) | 2, 1 << 31):
        assert call(classes=classes) == -1, classes
        assert call(classes=classes, mode=1) == 0                      # the foreground does not look at it
    for s2 in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, inf), (nan, 1.0, 1.0), (1.0, 1.0, nan), (1.0, -inf, 1.0)):
        assert call(s2=s2) == -1, s2
    for r2 in (-1.0, -1e-30, inf, -inf, nan):
        assert call(r2=r2) == -1, r2
    for outside in (2, -1):
        for op in range(4):
            assert call(outside=outside, op=op) == -1
    for value in (0, 256, -1):
        for op in (1, 3):
            assert call(mode=1, op=op, value=value) == -1, value
    out.fill_(77), stats.fill_(-7)
    assert call(o=pred) == -1                               # out may not be pred
    assert call(nbytes=need - 1) == -2                      # (outside guard mode ws has a floor of 256 bytes)
    for buf in (out_buf, stats_buf):
        assert bool((buf.cpu() == (77 if buf.dtype == torch.uint8 else -7)).all()), "a refused call wrote to an output"
    assert torch.equal(pred.cpu(), torch.from_numpy(pred_np))
    # the largest volume the entry accepts: the size query answers it, nothing is allocated
    assert lib.cfun_morph_workspace_bytes(128, 4096, 4095, 8) >= 3 * 128 * 4096 * 4095
    # accepted calls: every row of stats is written, whatever fill_value is where it is not used, and the canaries stay
    for mode, op, value, rows, classes, r2 in ((0, 0, 0, k, None, 1.0), (1, 1, 255, k, None, 1.0), (0, 3, 256, 15, None, 2.0),
                                               (1, 0, 0, 1, None, 1.0), (0, 2, 1, k, 0, 1.0), (0, 1, 1, k, None, 0.5),
                                               (0, 1, -5, k, 2, 1.0), (1, 2, 999, 3, 0xffffffff, 4.0)):
        out.fill_(77), stats.fill_(-7)
        assert call(kk=rows, mode=mode, op=op, value=value, classes=classes, r2=r2) == 0
        sel = None if classes is None or mode == 1 else tuple(c for c in range(1, rows) if (classes >> c) & 1)
        want, want_stats = mr.morph(pred_np, rows, mr.OPS[op], math.sqrt(r2), (1, 1, 1), MODES[mode], sel, 0, value)
        assert torch.equal(out.cpu(), torch.from_numpy(want)), (mode, op, value, rows, classes, r2)
        got = stats_buf.cpu()[64:64 + 30].view(15, 2)
        assert torch.equal(got[:rows], torch.from_numpy(want_stats)) and bool((got[rows:] == -7).all())
        for buf, t in ((out_buf, out), (stats_buf, stats)):
            flat, c = buf.cpu(), (77 if buf.dtype == torch.uint8 else -7)
            assert bool((flat[:64] == c).all()) and bool((flat[64 + t.numel():] == c).all()), "a canary beside an output changed"
    # zero-sized volumes through the C entry: stats all zeros, out untouched
    for d in ((0, 3, 70), (2, 0, 70), (2, 3, 0)):
        out.fill_(77), stats.fill_(-7)
        assert call(d=d) == 0
        assert not stats.cpu()[:k].any() and bool((stats.cpu()[k:] == -7).all()) and bool((out_buf.cpu() == 77).all())


def check_wrapper_preconditions(device):
    from cfun_amd import _lib, morphology
    pred = torch.zeros((4, 5, 6), dtype=torch.uint8, device=device)
    morph = morphology.morph
    with pytest.raises(ValueError, match="uint8"):
        morph(pred.to(torch.int32), 8, "erode", 1.0)
    with pytest.raises(ValueError, match=r"\[D,H,W\]"):
        morph(pred[0], 8, "erode", 1.0)
    huge = torch.zeros(1, dtype=torch.uint8, device=device).expand(2048, 1024, 1024)          # a view: nothing is allocated
    with pytest.raises(ValueError, match=r"2\^31"):
        morph(huge, 8, "erode", 1.0)
    with pytest.raises(ValueError, match="4096"):
        morph(torch.zeros(1, dtype=torch.uint8, device=device).expand(1, 1, 4097), 8, "erode", 1.0)
    for k in (0, 16, -1):
        with pytest.raises(ValueError, match="num_classes"):
            morph(pred, k, "erode", 1.0)
    for op in ("shrink", 0, None):
        with pytest.raises(ValueError, match="op must be"):
            morph(pred, 8, op, 1.0)
    with pytest.raises(ValueError, match="by must be"):
        morph(pred, 8, "erode", 1.0, by="organ")
    for radius in (-1.0, float("inf"), float("nan"), 1e30, None, "big"):
        with pytest.raises(ValueError, match="radius"):
            morph(pred, 8, "erode", radius)
    for spacing in ((1.0, 1.0), (0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("inf")), (float("nan"), 1.0, 1.0), (1e30, 1.0, 1.0)):
        with pytest.raises(ValueError, match="spacing"):
            morph(pred, 8, "erode", 1.0, spacing)
    for classes in (0, 8, (1, 8), (0,), -1, 1.5, "liver", (2.5,)):
        with pytest.raises(ValueError, match="classes"):
            morph(pred, 8, "erode", 1.0, classes=classes)
    for outside in (2, -1, 0.5, "in"):
        with pytest.raises(ValueError, match="outside"):
            morph(pred, 8, "erode", 1.0, outside=outside)
    for value in (0, 256, -1, 1.5, None):
        with pytest.raises(ValueError, match="fill_value"):
            morph(pred, 8, "dilate", 1.0, by="foreground", fill_value=value)
    with pytest.raises(RuntimeError, match="contiguous"):
        morph(pred.permute(2, 1, 0).contiguous().permute(2, 1, 0), 8, "erode", 1.0)
    if not _lib.is_emulator():
        with pytest.raises(RuntimeError, match="CPU tensor"):
            morph(pred.cpu(), 8, "erode", 1.0)
    for fn, op in ((morphology.erode, "erode"), (morphology.dilate, "dilate"), (morphology.open_ball, "open"), (morphology.close_ball, "close")):
        v = torch.from_numpy(hand.mixed()).to(device)
        a, b = fn(v, 3, 1.5, (1.0, 1.0, 2.0), "class", (1,)), morph(v, 3, op, 1.5, (1.0, 1.0, 2.0), "class", (1,))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    out, stats = morph(pred, 8, "open", 2.0)               # the defaults: unit spacing, by class, every class
    assert not out.cpu().any() and tuple(stats.shape) == (8, 2)


def check_value_object(device):
    from cfun_amd import components, morphology
    MO, FH, PP = morphology.Morphology, components.FillHoles, components.Postprocess
    d = MO("open", 2)
    assert (d.op, d.radius, d.spacing, d.by, d.classes, d.outside, d.fill_value, d.before) == ("open", 2.0, (1.0, 1.0, 1.0), "class", None,
                                                                                             0, 1, None)
    assert MO("close", 1).outside == 1 and MO("erode", 1).outside == 0 and MO("close", 1, outside=0).outside == 0
    assert MO("erode", 1, classes=2).classes == (2,) and MO("erode", 1, classes=[2, 1, 2]).classes == (1, 2)
    a = MO("close", 1.5, LITS, "foreground", None, 1, 7, FH(clean=PP(6)))
    assert a == MO("close", 1.5, LITS, "foreground", None, None, 7, FH(clean=PP(6))) and hash(a) == hash(MO("close", 1.5, LITS, "foreground", None, 1, 7, FH(clean=PP(6))))
    assert a != d and a != MO("close", 1.5, LITS, "foreground", None, 1, 7) and d != PP() and d == MO("open", 2.0, outside=0)
    assert len({a, d, MO("open", 2), MO("open", 2, before=d), MO("open", 2, before=MO("open", 2))}) == 3
    assert repr(d) == "Morphology('open', 2.0, spacing=(1.0, 1.0, 1.0), by='class', classes=None, outside=0, fill_value=1, before=None)"
    assert eval(repr(a), {"Morphology": MO, "FillHoles": FH, "Postprocess": PP}) == a
    with pytest.raises(AttributeError):
        d.connectivity = 6                                 # slots
    for args, kw in ((("shrink", 1), {}), (("open", -1), {}), (("open", 1), dict(spacing=(1, 1))), (("open", 1), dict(by="organ")),
                     (("open", 1), dict(classes=0)), (("open", 1), dict(outside=2)), (("open", 1), dict(fill_value=0)),
                     (("open", 1), dict(before="largest")), (("open", 1), dict(spacing=(0, 1, 1)))):
        with pytest.raises(ValueError):
            MO(*args, **kw)
    # the call: before's columns are before's own; the op runs on before's map
    pred_np = fc.dense(fc.SEAM_SHAPE, 0.9, 3, 31)
    pred = torch.from_numpy(pred_np).to(device)
    for before in (PP(6, "class"), FH(clean=PP(6, "class")), MO("close", 1.0, before=PP(26, "foreground"))):
        m = MO("open", 1.5, (1.0, 1.0, 1.0), before=before)
        out, stats = m(pred, 3)
        mid, mid_stats = before(pred, 3)
        want, want_stats = morphology.morph(mid, 3, "open", 1.5)
        assert stats.dtype == torch.int64 and tuple(stats.shape) == (3, mid_stats.shape[1] + 2) and stats.device == pred.device
        assert torch.equal(out, want) and torch.equal(stats[:, :-2], mid_stats) and torch.equal(stats[:, -2:], want_stats)
        host, host_stats = mr.morph(mid.cpu().numpy(), 3, "open", 1.5)
        assert host_stats[:, 0].sum() > 0 and np.array_equal(out.cpu().numpy(), host) and np.array_equal(want_stats.cpu().numpy(), host_stats)
    out, stats = MO("dilate", 1.0, by="foreground", fill_value=5)(pred, 3)
    host, host_stats = mr.morph(pred_np, 3, "dilate", 1.0, by="foreground", fill_value=5)
    assert np.array_equal(out.cpu().numpy(), host) and np.array_equal(stats.cpu().numpy(), host_stats)


# ------------------------------------------------------------------------------------------------- detect_original / run_test
def _check_morphed(r, base, k, m):
    """What run_test scored and reports with a Morphology: morph(before(raw)), restated on the host."""
    from cfun_amd import morphology
    for i, res in enumerate(r["results"]):
        raw = res["mask_device_raw"]
        assert torch.equal(raw, base["results"][i]["mask_device"]) and res["empty"] == base["results"][i]["empty"]
        mid, mid_stats = m.before(raw, k) if m.before is not None else (raw, None)
        want, want_stats = morphology.morph(mid, k, m.op, m.radius, m.spacing, m.by, m.classes, m.outside, m.fill_value)
        got, stats = res["mask_device"], res["component_stats"]
        assert got.dtype == torch.uint8 and got.device == raw.device and stats.device == raw.device and stats.dtype == torch.int64
        assert torch.equal(got, want), "the scored map is not morph() of the raw map"
        if mid_stats is not None:
            assert torch.equal(stats[:, :-2], mid_stats), "the before columns are not the before object's own"
        assert tuple(stats.shape) == (k, 2 + (0 if mid_stats is None else mid_stats.shape[1])) and torch.equal(stats[:, -2:], want_stats)
        host, host_stats = mr.morph(mid.cpu().numpy(), k, m.op, m.radius, m.spacing, m.by, m.classes, m.outside, m.fill_value)
        assert np.array_equal(got.cpu().numpy(), host) and np.array_equal(want_stats.cpu().numpy(), host_stats)
    return [res["mask_device"] for res in r["results"]]


def check_run_test_heart(device, tmp_path):
    import module_cases as mc
    from cfun_amd import components, evaluate, morphology
    cfg = mc.tiny_config("beginning")
    k = int(cfg.NUM_CLASSES)
    net = ec._net(device, cfg, 1)
    img, lab = ec._case_arrays(2, k)
    cases = [(img, lab, ec.AFFINE, "first.nii")]
    plain, plain_reads = fc._run_counted(evaluate, net, cases)
    assert not plain["results"][0]["empty"], "test setup: no detection"
    m = morphology.Morphology("open", 1.0, before=components.FillHoles(clean=components.Postprocess(connectivity=6, by="class")))
    r, reads = fc._run_counted(evaluate, net, cases, postprocess=m)
    assert reads == plain_reads, "the morphology added a synchronisation: %d host reads against %d" % (reads, plain_reads)
    scored = _check_morphed(r, plain, k, m)
    import eval_ref as er
    counts = er.confusion(scored[0].cpu().numpy().transpose(1, 2, 0), lab, k)
    np.testing.assert_allclose(r["per_class_ious"][0], er.per_class_iou(counts), rtol=1e-15, atol=0)
    m2 = morphology.Morphology("close", 1.5, (1.0, 1.0, 2.0), by="foreground", fill_value=3)
    _check_morphed(evaluate.run_test(net, cases, postprocess=m2), plain, k, m2)
    cfg.DETECTION_MIN_CONFIDENCE = 1.5                     # no detection at all: zeros in, zeros out
    res = evaluate.detect_original(net, torch.from_numpy(img)[..., None], m)
    assert res["empty"] is True and not res["mask_device"].cpu().any() and not res["mask_device_raw"].cpu().any()
    assert tuple(res["component_stats"].shape) == (k, 7) and not res["component_stats"].cpu().any()


def check_run_test_lits(device, tmp_path):
    import module_cases as mc
    from cfun_amd import components, evaluate, morphology
    cfg = mc.tiny_lits_config("together", max_dim=64, min_dim=32)
    cfg.PAD_IMAGE_SHAPE = [80, 80, 40]
    k = int(cfg.NUM_CLASSES)
    net = ec._net(device, cfg, 2)
    rng = np.random.default_rng(9)
    image = rng.normal(0.0, 200.0, ec.SRC).astype(np.float32)
    label = np.zeros(ec.SRC, np.int32)
    label[5:30, 10:44, 2:15] = rng.integers(0, k, (25, 34, 13))
    cases = [(image, label, ec.AFFINE, "liver_7.nii.gz", (44, 52, 22))]
    plain, plain_reads = fc._run_counted(evaluate, net, cases)
    assert not plain["results"][0]["empty"], "test setup: no detection"
    # the LiTS recipe: the organ as one component, then the liver opened by 2 mm at the mean spacing
    m = morphology.Morphology("open", 2.0, LITS, classes=1, before=components.Postprocess(connectivity=26, by="foreground"))
    r, reads = fc._run_counted(evaluate, net, cases, postprocess=m)
    assert reads == plain_reads, "the morphology added a synchronisation: %d host reads against %d" % (reads, plain_reads)
    _check_morphed(r, plain, k, m)


# ------------------------------------------------------------------------------------------------------------ accounting
def morph_header_symbols():
    """The same parse as test_abi.header_symbols, on include/cfun_morph.h."""
    txt = open(os.path.join(ROOT, "include", "cfun_morph.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(cfun_[a-z0-9_]+)\s*\(", txt)))


MORPH_NO_LAUNCH = {"cfun_morph_workspace_bytes": "host-side query: launches nothing, touches no device memory"}


def check_coverage(tier):
    from cfun_amd import _lib
    assert morph_header_symbols() == sorted(_lib.MORPH_EXPORTS) == ["cfun_morph_apply", "cfun_morph_workspace_bytes"]
    for other in (_lib.EXPORTS, _lib.SAMPLE_EXPORTS, _lib.TILE_EXPORTS, _lib.EVAL_EXPORTS, _lib.CC_EXPORTS, _lib.SURFACE_EXPORTS,
                  _lib.LESION_EXPORTS, _lib.FILL_EXPORTS):
        assert not set(_lib.MORPH_EXPORTS) & set(other)
    missed = sorted(set(_lib.MORPH_EXPORTS) - set(MORPH_NO_LAUNCH) - guard.SEEN[tier])
    assert not missed, "morph entries that launch work but never ran under guard: %s" % missed
