"""Cases of the hole filling (cfun_amd/components.py fill_holes / FillHoles, cfun_amd/csrc/fill.hip) shared by test_fill_emu.py
and test_fill_gpu.py: the device against tests/fill_ref.py (scipy.ndimage.binary_fill_holes), everything an integer and compared
with torch.equal, nothing excluded -- the map and both columns of the statistics."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import cc_cases as cc
import cc_ref as cr
import eval_cases as ec
import eval_ref as er
import fill_ref as fr
import guard
import test_fill_ref as hand
from conftest import ROOT


def tile_constants(name):
    """(kTZ, kTY, kTX) as cfun_amd/csrc/<name> declares them."""
    txt = open(os.path.join(ROOT, "cfun_amd", "csrc", name)).read()
    m = re.search(r"constexpr int kTZ = (\d+), kTY = (\d+), kTX = (\d+);", txt)
    assert m, "%s no longer declares its tile as kTZ, kTY, kTX" % name
    return tuple(int(v) for v in m.groups())


# The shapes are cc_cases.SHAPES, and they are what they are because of cc.hip's tile, which fill.hip shares: one voxel; one voxel
# over the tile in x alone; one over in every axis; less than a tile in z, two tiles and a voxel in y and in x; two tiles and a
# voxel in z, ragged in y and x; a single row of four tiles.  A changed constant fails here, before any case runs.
TZ, TY, TX = tile_constants("cc.hip")
assert tile_constants("fill.hip") == (TZ, TY, TX), "fill.hip and cc.hip no longer share one tile"
SHAPES = [(1, 1, 1), (1, 1, TX + 1), (TZ + 1, TY + 1, TX + 1), (3, 2 * TY + 1, 2 * TX + 2), (2 * TZ + 1, TY + 2, TX + 3),
          (2, 1, 3 * TX + 8)]
assert SHAPES == cc.SHAPES == [(1, 1, 1), (1, 1, 65), (9, 9, 65), (3, 17, 130), (17, 10, 67), (2, 1, 200)]
SEAM_SHAPE = (2 * TZ + 1, TY + 2, TX + 3)                  # (17,10,67): a shell from (1,1,1) to (15,8,65) crosses z = 8, y = 8, x = 64
SEAM_HI = (2 * TZ - 1, TY, TX + 1)
assert SEAM_SHAPE == (17, 10, 67) and SEAM_HI == (15, 8, 65)
BIG = (8 * TZ, 9 * TY, 2 * TX + 2)                         # GPU tier only: 8 x 9 x 3 tiles, 599 040 voxels
assert BIG == cc.BIG == (64, 72, 130)
DEGENERATE = [(1, 1, 1), (1, 1, 65), (2, 1, 200)]          # no interior: under every neighbourhood every voxel is on a border
INTERIOR = [s for s in SHAPES if min(s) >= 3]
assert INTERIOR == [(9, 9, 65), (3, 17, 130), (17, 10, 67)] and [s for s in SHAPES if s not in INTERIOR] == DEGENERATE

# (connectivity, axis): the two 3-D neighbourhoods and 4 / 8 within the planes perpendicular to each axis
NEIGHBOURHOODS = [(6, None), (26, None), (4, 0), (8, 0), (4, 1), (8, 1), (4, 2), (8, 2)]
MODES = ("class", "foreground")


def dense(shape, p, k, seed):
    """Object with probability p.  k == 2: all class 1; k == 3: class 1 takes 90 % of the object and class 2 the rest."""
    assert k in (2, 3)
    rng = np.random.default_rng(seed)
    obj = rng.random(shape) < p
    cls = np.ones(shape, np.uint8) if k == 2 else np.where(rng.random(shape) < 0.9, 1, 2)
    return np.where(obj, cls, 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _reference(key, k, by, conn, axis, fill_value):
    """fill_ref.fill of a registered map, computed once and shared by the plain and the guarded copy of a case; read-only."""
    out, stats = fr.fill(_MAPS[key], k, by, conn, axis, fill_value)
    out.setflags(write=False)
    stats.setflags(write=False)
    return out, stats


_MAPS = {}


def reference(pred, k, by, conn, axis, fill_value=1):
    key = (pred.shape, pred.tobytes())
    _MAPS.setdefault(key, pred.copy())
    return _reference(key, k, by, conn, axis, fill_value)


def check_case(device, pred, k, by, conn, axis, fill_value=1):
    """One map through fill_holes against fill_ref; returns (filled, stats) of the device as numpy arrays."""
    from cfun_amd import components
    pred = np.ascontiguousarray(pred)
    t = torch.from_numpy(pred.copy()).to(device)
    want, want_stats = reference(pred, k, by, conn, axis, fill_value)
    tag = "%s k %d %s conn %s axis %s value %d" % (pred.shape, k, by, conn, axis, fill_value)
    out, stats = components.fill_holes(t, k, by, conn, axis, fill_value)
    assert out.dtype == torch.uint8 and tuple(out.shape) == pred.shape and stats.dtype == torch.int64 and tuple(stats.shape) == (k, 2)
    assert out.device == t.device and stats.device == t.device and out.data_ptr() != t.data_ptr()
    assert torch.equal(stats.cpu(), torch.from_numpy(want_stats.copy())), "stats: %s\n%s\n%s" % (tag, stats.cpu(), want_stats)
    assert torch.equal(out.cpu(), torch.from_numpy(want.copy())), "filled: " + tag
    assert torch.equal(t.cpu(), torch.from_numpy(pred)), "the input was written to: " + tag
    got = out.cpu().numpy()
    assert np.array_equal(got[pred != 0], pred[pred != 0]), "a non-zero byte was rewritten: " + tag
    return got, stats.cpu().numpy()


def check_all_ways(device, pred, k, fill_value=1):
    for conn, axis in NEIGHBOURHOODS:
        for by in MODES:
            check_case(device, pred, k, by, conn, axis, fill_value)


def _seed(shape):
    return 300 + shape[0] * 31 + shape[1] * 7 + shape[2]


def check_bernoulli_shape(device, shape):
    """Densities 0.75 and 0.95 with K = 2, 0.95 with K = 3, all eight neighbourhoods, both modes.  What a draw tests is a property
    of the data, asserted on the REFERENCE: at 0.95 every neighbourhood encloses something and leaves something open on the
    shapes that have an interior; at 0.75 the 26-neighbourhood leaks nearly everywhere at these sizes, so that density tests only
    the open side there (and both sides under the other seven).  The shapes without an interior fill nothing."""
    for p, k in ((0.75, 2), (0.95, 2), (0.95, 3)):
        pred = dense(shape, p, k, _seed(shape) + k)
        for conn, axis in NEIGHBOURHOODS:
            for by in MODES:
                want, want_stats = reference(pred, k, by, conn, axis)
                filled = int(want_stats[:, 1].sum())
                assert filled == int((want != pred).sum())
                if shape in DEGENERATE:
                    assert not want_stats.any(), "test setup: a shape without an interior encloses something"
                else:
                    n_open = int(fr.open_components(pred, k, by, conn, axis).sum())
                    assert n_open >= 1, "test setup: no open component: %s" % ((shape, p, k, conn, axis, by),)
                    if p == 0.95 or conn != 26:
                        assert filled >= 1, "test setup: nothing is filled: %s" % ((shape, p, k, conn, axis, by),)
                check_case(device, pred, k, by, conn, axis)
        if k == 3 and shape == SEAM_SHAPE:
            # class 1's complement holds the class-2 voxels: most of its enclosed components are made of those and change nothing
            _, s = reference(pred, 3, "class", 6, None)
            assert s[1, 0] > s[1, 1] > 0, "test setup: enclosed components do not exceed filled voxels: %s" % s.tolist()


def seam_shell():
    """A closed class-1 shell from (1,1,1) to SEAM_HI in SEAM_SHAPE: its interior crosses the seams at z = 8, y = 8 and x = 64."""
    v = np.zeros(SEAM_SHAPE, np.uint8)
    z, y, x = SEAM_HI
    v[1:z + 1, 1:y + 1, 1:x + 1] = 1
    v[2:z, 2:y, 2:x] = 0
    return v, (z - 2) * (y - 2) * (x - 2)


def check_cavity_across_seams(device):
    v, interior = seam_shell()
    z, y, x = SEAM_HI
    assert interior == 13 * 6 * 63
    check_all_ways(device, v, 2)
    for conn in (6, 26):
        got, stats = check_case(device, v, 2, "class", conn, None)
        assert stats.tolist() == [[0, 0], [1, interior]] and bool((got[2:z, 2:y, 2:x] == 1).all())
    got, stats = check_case(device, v, 2, "foreground", 4, 0, 9)
    assert stats.tolist() == [[z - 2, interior], [0, 0]] and bool((got[2:z, 2:y, 2:x] == 9).all())
    # one face voxel removed at the far corner: the open mark has to travel from there through every tile the interior touches
    pin = v.copy()
    pin[z, y - 1, x - 1] = 0
    check_all_ways(device, pin, 2)
    for conn in (6, 26):
        got, stats = check_case(device, pin, 2, "class", conn, None)
        assert not stats.any() and np.array_equal(got, pin)
    # one edge voxel removed (where the z and y walls meet): shut under 6, a leak under 26
    edge = v.copy()
    edge[z, y, x - 1] = 0
    check_all_ways(device, edge, 2)
    got, stats = check_case(device, edge, 2, "class", 6, None)
    assert stats.tolist() == [[0, 0], [1, interior]] and got[z, y, x - 1] == 0
    got, stats = check_case(device, edge, 2, "class", 26, None)
    assert not stats.any() and np.array_equal(got, edge)


def check_uniform_tiles(device):
    """Tiles with nothing of the object in them take a path of their own in the local pass (the tile is one box, or one rectangle
    per plane).  A closed shell around whole empty tiles -- the tile z 8 .. 15, y 8 .. 15, x 64 .. 127 lies strictly inside --
    and, outside it, empty tiles that are open; ragged on every axis, so that the last tiles are boxes smaller than a tile."""
    shape = (3 * TZ + 2, 3 * TY + 2, 3 * TX + 8)
    assert shape == (26, 26, 200)
    v = np.zeros(shape, np.uint8)
    v[1:17, 1:18, 1:131] = 1
    v[2:16, 2:17, 2:130] = 0
    interior = 14 * 15 * 128
    check_all_ways(device, v, 2)
    for conn in (6, 26):
        got, stats = check_case(device, v, 2, "class", conn, None)
        assert stats.tolist() == [[0, 0], [1, interior]] and bool((got[TZ:2 * TZ, TY:2 * TY, TX:2 * TX] == 1).all())
    got, stats = check_case(device, v, 2, "class", 4, 2)              # planes perpendicular to x: 128 rectangles
    assert stats.tolist() == [[0, 0], [128, interior]]
    check_all_ways(device, v, 3)                                      # class 2 is nowhere: every tile of its labelling is empty
    pin = v.copy()
    pin[16, 16, 129] = 0                                              # a face voxel at the far corner, two tiles from the empty one
    check_all_ways(device, pin, 2)
    got, stats = check_case(device, pin, 2, "class", 6, None)
    assert not stats.any() and np.array_equal(got, pin)


def channel(shape):
    """cc_cases.serpentine as the COMPLEMENT: class 1 everywhere, the one-voxel-wide path carved out of the interior (one voxel of
    frame all round).  Returns (closed map, open map, voxels of the channel): in the open map the channel reaches the border
    at its LAST voxel only, through one voxel of the frame."""
    d, h, w = shape
    inner = cc.serpentine((d - 2, h - 2, w - 2)) > 0
    closed = np.ones(shape, np.uint8)
    closed[1:-1, 1:-1, 1:-1][inner] = 0
    # the path's ends: channel voxels with at most one face neighbour in the channel; it starts at (0,0,0) of the interior
    pad = np.pad(inner, 1).astype(np.int32)
    nb = (pad[:-2, 1:-1, 1:-1] + pad[2:, 1:-1, 1:-1] + pad[1:-1, :-2, 1:-1] + pad[1:-1, 2:, 1:-1] + pad[1:-1, 1:-1, :-2] +
          pad[1:-1, 1:-1, 2:])
    ends = [tuple(int(c) for c in e) for e in np.argwhere(inner & (nb <= 1))]
    assert (0, 0, 0) in ends and 1 <= len(ends) <= 2, "test setup: the serpentine is not a simple path"
    lz, ly, lx = ends[-1]
    assert lx in (0, w - 3), "test setup: the path does not end at a wall"
    opened = closed.copy()
    opened[lz + 1, ly + 1, 0 if lx == 0 else w - 1] = 0
    return closed, opened, int(inner.sum())


def check_channel(device, shape):
    closed, opened, n = channel(shape)
    check_all_ways(device, closed, 2)
    check_all_ways(device, opened, 2)
    for conn in (6, 26):
        for by in MODES:
            row = 1 if by == "class" else 0
            got, stats = check_case(device, closed, 2, by, conn, None)
            assert bool((got == 1).all()) and stats[row].tolist() == [1, n]          # the whole channel, one component
            got, stats = check_case(device, opened, 2, by, conn, None)
            assert np.array_equal(got, opened) and not stats.any()                    # open at its far end: nothing


def check_priority(device):
    v = hand.nested()
    for conn in (6, 26):
        got, stats = check_case(device, v, 3, "class", conn, None)
        assert got[4, 4, 4] == 2 and stats.tolist() == [[0, 0], [1, 98], [1, 1]]
    check_all_ways(device, v, 3, fill_value=7)
    check_all_ways(device, v, 2)                          # the same map with class 2 in no group: bytes >= K
    big = np.zeros(SEAM_SHAPE, np.uint8)                  # and across the x seam
    big[4:13, 0:9, TX - 6:TX + 3] = v
    got, stats = check_case(device, big, 3, "class", 6, None)
    assert got[8, 4, TX - 2] == 2 and stats.tolist() == [[0, 0], [1, 98], [1, 1]]
    check_all_ways(device, big, 3)
    check_all_ways(device, big, 15)
    blob = np.zeros((7, 7, 7), np.uint8)                  # a class-2 blob wholly inside class 1, no background
    blob[1:6, 1:6, 1:6] = 1
    blob[2:5, 2:5, 2:5] = 2
    got, stats = check_case(device, blob, 3, "class", 6, None)
    assert np.array_equal(got, blob) and stats.tolist() == [[0, 0], [1, 0], [0, 0]]
    check_all_ways(device, blob, 3)


def check_values_beyond_k(device):
    pred = dense((9, 9, 65), 0.95, 3, 12)
    rng = np.random.default_rng(13)
    far = (rng.random(pred.shape) < 0.2) & (pred != 0)
    pred[far] = rng.integers(3, 6, int(far.sum()))        # ids 3 .. 5 with K = 3
    pred[4, 4, 30] = 255
    assert (pred >= 3).any()
    check_all_ways(device, pred, 3)
    check_all_ways(device, pred, 1)                       # no class at all: by="class" copies the map through
    got, stats = check_case(device, pred, 1, "class", 6, None)
    assert np.array_equal(got, pred) and not stats.any()
    w = hand.shell(5, 1, 3, 9)                            # a shell of an unknown byte: foreground, but no class's object
    got, stats = check_case(device, w, 3, "class", 6, None)
    assert np.array_equal(got, w) and not stats.any()
    got, stats = check_case(device, w, 3, "foreground", 6, None, 2)
    assert got[2, 2, 2] == 2 and stats.tolist() == [[1, 1], [0, 0], [0, 0]]


def check_fill_value(device):
    pred = dense(SEAM_SHAPE, 0.95, 3, 21)
    for value in (1, 7, 255):
        for conn, axis in ((6, None), (8, 0)):
            got, stats = check_case(device, pred, 3, "foreground", conn, axis, value)
            assert stats[0, 1] > 0 and int(((got == value) & (pred == 0)).sum()) == stats[0, 1]
            check_case(device, pred, 3, "class", conn, axis, value)          # by="class" does not look at it


def check_repeatable(device, shape=SEAM_SHAPE):
    from cfun_amd import components
    t = torch.from_numpy(dense(shape, 0.95, 3, 77)).to(device)
    for conn, axis in NEIGHBOURHOODS:
        for by in MODES:
            (o1, s1), (o2, s2) = components.fill_holes(t, 3, by, conn, axis), components.fill_holes(t, 3, by, conn, axis)
            assert torch.equal(o1, o2) and torch.equal(s1, s2)


def big_map():
    """Density 0.95, K = 3, with three closed class-1 shells (7^3, interior 5^3 of background) planted on tile corners."""
    pred = dense(BIG, 0.95, 3, 5)
    corners = [(TZ, TY, TX), (2 * TZ, 3 * TY, TX), (7 * TZ, 8 * TY, TX)]
    for z, y, x in corners:
        pred[z - 3:z + 4, y - 3:y + 4, x - 3:x + 4] = 1
        pred[z - 2:z + 3, y - 2:y + 3, x - 2:x + 3] = 0
        assert z + 4 <= BIG[0] and y + 4 <= BIG[1] and x + 4 <= BIG[2]
    return pred, corners


def check_big(device):
    """GPU tier only: several hundred tiles, so that workgroups really do run at the same time."""
    pred, corners = big_map()
    for conn, axis in NEIGHBOURHOODS:
        got, stats = check_case(device, pred, 3, "class", conn, axis)
        for z, y, x in corners:
            assert bool((got[z - 2:z + 3, y - 2:y + 3, x - 2:x + 3] == 1).all())
        assert stats[1, 0] > 3 and stats[1, 1] > 3 * 125
    for conn, axis in ((6, None), (26, None), (4, 0)):
        check_case(device, pred, 3, "foreground", conn, axis, 3)
    check_repeatable(device, BIG)


# --------------------------------------------------------------------------------------------------------------- entries
def _canary(shape, dtype, device, value):
    """A tensor with 64 canary elements either side of it in one allocation."""
    n = int(np.prod(shape))
    buf = torch.full((n + 128,), value, dtype=dtype, device=device)
    return buf, buf[64:64 + n].view(shape)


def check_zero_sized_and_c_entry(device):
    """Zero-sized volumes; every refusal of the C entry with canaries either side of out and stats; a workspace one byte short."""
    from cfun_amd import _lib, components
    lib = _lib.load()
    for dims in ((0, 5, 7), (5, 0, 7), (5, 7, 0)):
        pred = torch.zeros(dims, dtype=torch.uint8, device=device)
        for by, axis in (("class", None), ("foreground", 0)):
            out, stats = components.fill_holes(pred, 8, by, axis=axis)
            assert tuple(out.shape) == dims and out.dtype == torch.uint8 and tuple(stats.shape) == (8, 2) and not stats.cpu().any()
        assert lib.cfun_fill_workspace_bytes(*dims, 8) == 0
    dims, k = (2, 3, 70), 8
    pred_np = np.ones(dims, np.uint8)
    pred_np[0, 1, 5] = 0
    pred = torch.from_numpy(pred_np).to(device)
    out_buf, out = _canary(dims, torch.uint8, device, 77)
    stats_buf, stats = _canary((15, 2), torch.int64, device, -7)
    need = lib.cfun_fill_workspace_bytes(*dims, k)
    assert need >= 4 * pred_np.size
    ws = _lib.workspace(need, pred)
    i32 = C.c_int32 * 3
    p, st = _lib.ptr, _lib.stream(pred)

    def call(d=dims, kk=k, mode=0, conn=6, axis=-1, value=1, o=None, nbytes=None):
        return lib.cfun_fill_holes(p(pred), i32(*d), kk, mode, conn, axis, value, p(out if o is None else o), p(stats), p(ws),
                                   ws.numel() if nbytes is None else nbytes, st)

    bad_dims = ((2048, 1024, 1024), (1, 1 << 16, 1 << 15), (1, 1, (1 << 31) - 1), (1 << 30, 1 << 30, 1 << 30), (2, -3, 4), (-1, 0, 4))
    for d in bad_dims:
        assert call(d=d) == -1, d
        assert lib.cfun_fill_workspace_bytes(*d, k) == 0
    for kk in (0, 16, -1):
        assert call(kk=kk) == -1 and lib.cfun_fill_workspace_bytes(*dims, kk) == 0
    for mode in (2, -1):
        assert call(mode=mode) == -1
    for conn, axis in ((4, -1), (8, -1), (18, -1), (0, -1), (6, 0), (26, 1), (6, 2), (0, 0), (4, 3), (6, 3), (4, -2), (6, -2)):
        assert call(conn=conn, axis=axis) == -1, (conn, axis)
    for value in (0, 256, -1):
        assert call(mode=1, value=value) == -1, value
    assert call(o=pred) == -1                               # out may not be pred
    assert call(nbytes=need - 1) == -2                      # (outside guard mode ws has a floor of 256 bytes)
    for buf in (out_buf, stats_buf):
        assert bool((buf.cpu() == (77 if buf.dtype == torch.uint8 else -7)).all()), "a refused call wrote to an output"
    assert torch.equal(pred.cpu(), torch.from_numpy(pred_np))
    # the largest volume the entry accepts is one voxel short of 2^31 - 1: the size query answers it, nothing is allocated
    assert lib.cfun_fill_workspace_bytes(1, 1, (1 << 31) - 2, 8) > 4 * ((1 << 31) - 2)
    # accepted calls: every row of stats is written, whatever fill_value is in class mode, and the canaries stay
    for mode, value, rows in ((0, 0, k), (1, 255, k), (0, 1, 15), (1, 1, 1)):
        out.fill_(77), stats.fill_(-7)
        assert call(kk=rows, mode=mode, value=value) == 0
        want, want_stats = fr.fill(pred_np, rows, MODES[mode], 6, None, value)
        assert torch.equal(out.cpu(), torch.from_numpy(want))
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
    from cfun_amd import _lib, components
    pred = torch.zeros((4, 5, 6), dtype=torch.uint8, device=device)
    fill = components.fill_holes
    with pytest.raises(ValueError, match="uint8"):
        fill(pred.to(torch.int32), 8)
    with pytest.raises(ValueError, match=r"\[D,H,W\]"):
        fill(pred[0], 8)
    huge = torch.zeros(1, dtype=torch.uint8, device=device).expand(2048, 1024, 1024)          # a view: nothing is allocated
    with pytest.raises(ValueError, match=r"2\^31"):
        fill(huge, 8)
    for k in (0, 16, -1):
        with pytest.raises(ValueError, match="num_classes"):
            fill(pred, k)
    with pytest.raises(ValueError, match="by must be"):
        fill(pred, 8, "organ")
    for conn, axis in ((4, None), (8, None), (18, None), (6, 0), (26, 1), (6, 2), (0, 0)):
        with pytest.raises(ValueError, match="connectivity"):
            fill(pred, 8, "class", conn, axis)
    for axis in (3, -1, "z", 1.5):
        with pytest.raises(ValueError, match="axis"):
            fill(pred, 8, axis=axis)
    for value in (0, 256, -1, 1.5, None):
        with pytest.raises(ValueError, match="fill_value"):
            fill(pred, 8, "foreground", fill_value=value)
    with pytest.raises(RuntimeError, match="contiguous"):
        fill(pred.permute(2, 1, 0).contiguous().permute(2, 1, 0), 8)
    if not _lib.is_emulator():
        with pytest.raises(RuntimeError, match="CPU tensor"):
            fill(pred.cpu(), 8)
    out, stats = fill(pred, 8)                             # the defaults: by class, 6, no axis
    assert not out.cpu().any() and tuple(stats.shape) == (8, 2)


def check_value_object(device):
    from cfun_amd import components
    FH, PP = components.FillHoles, components.Postprocess
    d = FH()
    assert (d.by, d.connectivity, d.axis, d.fill_value, d.clean) == ("class", 6, None, 1, None)
    assert FH(axis=0).connectivity == 4 and FH(axis=2, connectivity=8).connectivity == 8
    a = FH("foreground", 8, 0, 7, PP(6, "foreground", False, 5))
    assert a == FH("foreground", 8, 0, 7, PP(6, "foreground", False, 5)) and hash(a) == hash(FH("foreground", 8, 0, 7, PP(6, "foreground", False, 5)))
    assert a != d and a != FH("foreground", 8, 0, 7) and a != FH("foreground", 8, 0, 7, PP()) and d != PP() and d == FH(connectivity=6)
    assert len({a, d, FH(), FH(axis=0), FH(axis=0, connectivity=4)}) == 3
    assert repr(d) == "FillHoles(by='class', connectivity=6, axis=None, fill_value=1, clean=None)"
    assert repr(a) == ("FillHoles(by='foreground', connectivity=8, axis=0, fill_value=7, clean=Postprocess(connectivity=6, "
                       "by='foreground', largest_only=False, min_voxels=5))")
    assert eval(repr(a), {"FillHoles": FH, "Postprocess": PP}) == a
    with pytest.raises(AttributeError):
        d.radius = 3                                       # slots
    for kw in (dict(by="organ"), dict(connectivity=4), dict(connectivity=26, axis=0), dict(axis=3), dict(fill_value=0),
               dict(fill_value=256), dict(clean="largest"), dict(clean=FH())):
        with pytest.raises(ValueError):
            FH(**kw)
    # the call: the clean columns are clean_components' own, zeros without one; the fill runs on the cleaned map
    pred_np = dense(SEAM_SHAPE, 0.95, 3, 31)
    pred_np[0, 0, 0:3] = 0
    pred_np[0, 0, 1] = 2                                   # a speck the cleaning removes
    pred = torch.from_numpy(pred_np).to(device)
    pp = PP(6, "class")
    out, stats = FH(clean=pp)(pred, 3)
    cleaned, clean_stats = components.clean_components(pred, 3, 6, "class")
    want, want_stats = components.fill_holes(cleaned, 3)
    assert stats.dtype == torch.int64 and tuple(stats.shape) == (3, 5) and stats.device == pred.device
    assert torch.equal(out, want) and torch.equal(stats[:, :3], clean_stats) and torch.equal(stats[:, 3:], want_stats)
    _, host_clean, host_clean_stats = cr.clean(pred_np, 3, 6, "class")
    host, host_stats = fr.fill(host_clean, 3)
    assert host_clean[0, 0, 1] == 0 and host_stats[:, 1].sum() > 0
    assert np.array_equal(out.cpu().numpy(), host)
    assert np.array_equal(stats.cpu().numpy(), np.concatenate([host_clean_stats, host_stats], axis=1))
    out, stats = FH("foreground", axis=0, fill_value=5)(pred, 3)
    host, host_stats = fr.fill(pred_np, 3, "foreground", 4, 0, 5)
    assert np.array_equal(out.cpu().numpy(), host) and tuple(stats.shape) == (3, 5)
    assert not stats[:, :3].cpu().any() and np.array_equal(stats[:, 3:].cpu().numpy(), host_stats)


# ------------------------------------------------------------------------------------------------- detect_original / run_test
class HostReads:
    """Counts the calls that make the host wait for the device: what run_test's "one synchronisation per case" is made of."""
    NAMES = ("cpu", "item", "tolist", "numpy", "__bool__", "__int__", "__float__", "__index__", "nonzero")

    def __init__(self):
        self.count = 0
        self._undo = []

    def __enter__(self):
        def counted(fn):
            def call(*a, **kw):
                self.count += 1
                return fn(*a, **kw)
            return call
        for obj, name in [(torch.Tensor, n) for n in self.NAMES] + [(torch.cuda, "synchronize")]:
            self._undo.append((obj, name, name in vars(obj), vars(obj).get(name)))
            setattr(obj, name, counted(getattr(obj, name)))
        return self

    def __exit__(self, *exc):
        for obj, name, had, old in reversed(self._undo):
            if had:
                setattr(obj, name, old)
            else:
                delattr(obj, name)
        return False


def _check_filled(r, base, labels, k, fh):
    """What run_test scored and reports with a FillHoles: fill_holes(clean_components(raw)), restated on the host."""
    from cfun_amd import components
    for i, res in enumerate(r["results"]):
        raw = res["mask_device_raw"]
        assert torch.equal(raw, base["results"][i]["mask_device"]) and res["empty"] == base["results"][i]["empty"]
        raw_np = raw.cpu().numpy()
        if fh.clean is not None:
            pp = fh.clean
            _, cleaned, clean_stats = cr.clean(raw_np, k, pp.connectivity, pp.by, pp.largest_only, pp.min_voxels)
            dev_clean, dev_clean_stats = components.clean_components(raw, k, pp.connectivity, pp.by, pp.largest_only, pp.min_voxels)
        else:
            cleaned, clean_stats, dev_clean = raw_np, np.zeros((k, 3), np.int64), raw
            dev_clean_stats = torch.zeros((k, 3), dtype=torch.int64, device=raw.device)
        want, fill_stats = fr.fill(cleaned, k, fh.by, fh.connectivity, fh.axis, fh.fill_value)
        got, stats = res["mask_device"], res["component_stats"]
        assert got.dtype == torch.uint8 and got.device == raw.device and stats.device == raw.device
        assert stats.dtype == torch.int64 and tuple(stats.shape) == (k, 5)
        assert torch.equal(stats[:, :3], dev_clean_stats), "the clean columns are not clean_components' own"
        assert torch.equal(got, components.fill_holes(dev_clean, k, fh.by, fh.connectivity, fh.axis, fh.fill_value)[0])
        assert np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(stats.cpu().numpy(), np.concatenate([clean_stats, fill_stats], axis=1))
        if labels[i] is None:
            continue
        counts = er.confusion(want.transpose(1, 2, 0), labels[i], k)
        np.testing.assert_allclose(r["per_class_ious"][i], er.per_class_iou(counts), rtol=1e-15, atol=0)
        np.testing.assert_allclose(r["dice"][i], er.dice(counts), rtol=1e-15, atol=0)
        np.testing.assert_allclose(r["mask_ious"][i], er.mask_iou(counts), rtol=1e-15, atol=0)
    return [res["mask_device"] for res in r["results"]]


def _run_counted(evaluate, net, cases, **kw):
    """run_test and the number of times it made the host wait for the device."""
    with HostReads() as reads:
        r = evaluate.run_test(net, cases, **kw)
    assert reads.count > 0
    return r, reads.count


def check_run_test_heart(device, tmp_path):
    import module_cases as mc
    from cfun_amd import components, evaluate, nifti
    cfg = mc.tiny_config("beginning")
    k = int(cfg.NUM_CLASSES)
    net = ec._net(device, cfg, 1)
    img, lab = ec._case_arrays(2, k)
    cases = [(img, lab, ec.AFFINE, "first.nii")]
    dirs = [os.path.join(str(tmp_path), n) for n in ("plain", "filled")]
    plain, plain_reads = _run_counted(evaluate, net, cases, save_dir=dirs[0], draw_bbox=True)
    assert not plain["results"][0]["empty"], "test setup: no detection"
    fh = components.FillHoles(clean=components.Postprocess(connectivity=6, by="class", largest_only=True, min_voxels=2))
    r, reads = _run_counted(evaluate, net, cases, save_dir=dirs[1], draw_bbox=True, postprocess=fh)
    assert reads == plain_reads, "the fill added a synchronisation: %d host reads against %d" % (reads, plain_reads)
    filled = _check_filled(r, plain, [lab], k, fh)
    # the saved file is the FILLED map with the box drawn, under the filled map's score
    path = os.path.join(dirs[1], str(r["per_class_ious"][0].mean()) + "_first.nii")
    assert r["saved"] == [path]
    want = ec._edges_numpy(filled[0].permute(1, 2, 0).cpu().numpy().astype(np.int32), r["results"][0]["rois"][0])
    assert np.array_equal(nifti.load(path).get_data(), want)
    # without a cleaning step, slice by slice; detect_original alone; and no detection at all: zeros in, zeros out
    fh2 = components.FillHoles("foreground", 8, 0, 3)
    _check_filled(evaluate.run_test(net, cases, postprocess=fh2), plain, [lab], k, fh2)
    res = evaluate.detect_original(net, torch.from_numpy(img)[..., None], components.FillHoles(axis=1))
    want, want_stats = fr.fill(res["mask_device_raw"].cpu().numpy(), k, "class", 4, 1)
    assert np.array_equal(res["mask_device"].cpu().numpy(), want) and np.array_equal(res["component_stats"].cpu().numpy()[:, 3:], want_stats)
    cfg.DETECTION_MIN_CONFIDENCE = 1.5
    res = evaluate.detect_original(net, torch.from_numpy(img)[..., None], fh)
    assert res["empty"] is True and not res["mask_device"].cpu().any() and not res["mask_device_raw"].cpu().any()
    assert tuple(res["component_stats"].shape) == (k, 5) and not res["component_stats"].cpu().any()


def check_run_test_lits(device, tmp_path):
    import module_cases as mc
    from cfun_amd import components, evaluate
    cfg = mc.tiny_lits_config("together", max_dim=64, min_dim=32)
    cfg.PAD_IMAGE_SHAPE = [80, 80, 40]
    k = int(cfg.NUM_CLASSES)
    net = ec._net(device, cfg, 2)
    rng = np.random.default_rng(9)
    image = rng.normal(0.0, 200.0, ec.SRC).astype(np.float32)
    label = np.zeros(ec.SRC, np.int32)
    label[5:30, 10:44, 2:15] = rng.integers(0, k, (25, 34, 13))
    cases = [(image, label, ec.AFFINE, "liver_7.nii.gz", (44, 52, 22))]
    dirs = [os.path.join(str(tmp_path), n) for n in ("plain", "filled")]
    plain, plain_reads = _run_counted(evaluate, net, cases, save_dir=dirs[0], draw_bbox=True)
    assert not plain["results"][0]["empty"], "test setup: no detection"
    # "liver u tumour" as one organ, then the axial slices' holes by class: the LiTS recipe
    fh = components.FillHoles(by="class", axis=0, clean=components.Postprocess(connectivity=26, by="foreground", largest_only=True))
    r, reads = _run_counted(evaluate, net, cases, save_dir=dirs[1], draw_bbox=True, postprocess=fh)
    assert reads == plain_reads, "the fill added a synchronisation: %d host reads against %d" % (reads, plain_reads)
    _check_filled(r, plain, [label], k, fh)
    assert len(r["saved"]) == 1 and os.path.basename(r["saved"][0]) == str(r["per_class_ious"][0].mean()) + "_liver_7.nii.gz"
    # the detector-only stage: zeros in, zeros out, no mask scores
    cfg.STAGE = "beginning"
    assert net.detector_phase_only
    r = evaluate.run_test(net, cases[:1], postprocess=fh)
    res = r["results"][0]
    assert r["per_class_ious"].shape == (0, k - 1) and not res["mask_device"].cpu().any() and not res["mask_device_raw"].cpu().any()
    assert tuple(res["component_stats"].shape) == (k, 5) and not res["component_stats"].cpu().any()


# ------------------------------------------------------------------------------------------------------------ accounting
def fill_header_symbols():
    """The same parse as test_abi.header_symbols, on include/cfun_fill.h."""
    txt = open(os.path.join(ROOT, "include", "cfun_fill.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(cfun_[a-z0-9_]+)\s*\(", txt)))


FILL_NO_LAUNCH = {"cfun_fill_workspace_bytes": "host-side query: launches nothing, touches no device memory"}


def check_coverage(tier):
    from cfun_amd import _lib
    assert fill_header_symbols() == sorted(_lib.FILL_EXPORTS) == ["cfun_fill_holes", "cfun_fill_workspace_bytes"]
    for other in (_lib.EXPORTS, _lib.SAMPLE_EXPORTS, _lib.TILE_EXPORTS, _lib.EVAL_EXPORTS, _lib.CC_EXPORTS, _lib.SURFACE_EXPORTS,
                  _lib.LESION_EXPORTS):
        assert not set(_lib.FILL_EXPORTS) & set(other)
    missed = sorted(set(_lib.FILL_EXPORTS) - set(FILL_NO_LAUNCH) - guard.SEEN[tier])
    assert not missed, "fill entries that launch work but never ran under guard: %s" % missed
