"""Cases of the warp path (cfun_amd.sample.warp_and_box / Warp / draw_warp / affine_map and ``augment=`` on make_sample,
make_sample_heart and make_sample_lits; k_warp_gather<0>, k_warp_gather<1> and k_warp_finish in cfun_amd/csrc/sample_warp.hip)
shared by test_sample_warp_emu.py and test_sample_warp_gpu.py: the device against tests/sample_warp_ref.py.  Both sides run the
header's double operations in the header's order, so image, labels, both boxes and the flag must be equal bit for bit."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch

import guard
import sample_ref as sr
import sample_warp_ref as wr
from conftest import ROOT

EINVAL, EWORKSPACE = -1, -2


def tile_constants():
    """The brick constants as cfun_amd/csrc/sample_warp.hip states them; the shapes below are derived from these values."""
    txt = open(os.path.join(ROOT, "cfun_amd", "csrc", "sample_warp.hip")).read()
    m = re.search(r"constexpr int kWX = (\d+), kWY = (\d+), kWZ = (\d+), kMaxGrid = (\d+);", txt)
    assert m, "sample_warp.hip no longer states its tile constants in one line"
    return tuple(int(v) for v in m.groups())


WX, WY, WZ, SRC_MAX_GRID = tile_constants()
assert (WX, WY, WZ) == (32, 8, 4), "the warp brick changed: re-derive the sweeps below from the new constants"
# either side of the brick and of the 4-wide store path: 1, 3 (scalar stores), 4 (one quad), tile - 1, tile (16-byte stores along
# x), tile + 1 (two bricks, scalar), tile + 4 (two bricks, 16-byte stores, a ragged second brick)
EDGE_W = [1, 3, 4, WX - 1, WX, WX + 1, WX + 4]
EDGE_H = [1, 3, 4, WY - 1, WY, WY + 1, WY + 4]
EDGE_D = sorted({1, WZ - 1, WZ, WZ + 1, 2 * WZ + 1})
# (D, H, W)
W_CASES = [(5, 6, w) for w in EDGE_W]
H_CASES = [(5, h, 8) for h in EDGE_H]
D_CASES = [(d, 6, 9) for d in EDGE_D]
# a brick that spans one, two and four control cells per axis: cells of (D - 1) / (g - 1) voxels on SPAN_SHAPE
SPAN_SHAPE = (2 * WZ + 1, WY + 5, WX + 17)
SPANS = {1: (2, 2, 2), 2: (5, 4, 3), 4: (9, 7, 7)}
# a grid coarser than, equal to and finer than the brick: cells of twice, once and a quarter of the brick's extent
CELL_SHAPE = (2 * WZ + 1, 2 * WY + 1, 2 * WX + 1)
CELL_GRIDS = {"coarser": (2, 2, 2), "equal": (3, 3, 3), "finer": (9, 9, 9)}
ANGLES = [0, 7, -13, 20, -20, 45, 90, 180]


def max_grid():
    from cfun_amd import _lib
    return int(_lib.load().cfun_sample_warp_max_grid())


def _rng(seed):
    return np.random.default_rng(seed)


def volume(shape, seed, kind="blob"):
    """image float32 [D,H,W] and labels uint8 [D,H,W]: a blob of random classes 0..2 in the middle, or every voxel set."""
    rng = _rng(seed)
    img = rng.normal(100.0, 350.0, shape).astype(np.float32)
    lab = np.zeros(shape, np.uint8)
    if kind == "blob":
        lo = [n // 4 for n in shape]
        hi = [max(l + 1, n - n // 5) for l, n in zip(lo, shape)]
        lab[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = rng.integers(0, 3, [b - a for a, b in zip(lo, hi)])
    elif kind == "full":
        lab[:] = rng.integers(1, 100, shape)
    return img, lab


def field(g, seed, sigma=1.5):
    return _rng(seed).normal(0.0, sigma, (3,) + tuple(g)).astype(np.float32)


def _bits(t):
    return t.cpu().view(torch.int32)


def compare(got, want, what=""):
    img, lab, raw, box, empty = got
    r_img, r_lab, r_raw, r_box, r_empty = want
    assert img.dtype == torch.float32 and tuple(img.shape) == r_img.shape
    diff = _bits(img) != torch.from_numpy(r_img).view(torch.int32)
    assert not diff.any(), "image bits, %s: %d of %d differ" % (what, int(diff.sum()), diff.numel())
    assert lab.dtype == torch.uint8 and raw.dtype == box.dtype == empty.dtype == torch.int32
    assert torch.equal(lab.cpu(), torch.from_numpy(r_lab)), "labels, " + what
    assert raw.cpu().tolist() == r_raw.tolist() and box.cpu().tolist() == r_box.tolist(), (what, raw, r_raw, box, r_box)
    assert empty.cpu().tolist() == [r_empty], what


def check_case(device, img, lab, grid=None, amap=None, flips=(False, False, False), orders=(0, 1)):
    from cfun_amd import sample
    ti, tl = torch.from_numpy(img).to(device), torch.from_numpy(lab).to(device)
    res = {}
    for order in orders:
        what = "%s grid %s map %s flips %s order %d" % (img.shape, None if grid is None else grid.shape[1:], amap, flips, order)
        got = sample.warp_and_box(ti, tl, sample.Warp(grid, amap, flips, order))
        compare(got, wr.warp(img, lab, grid, amap, flips, order), what)
        res[order] = got
    if len(res) == 2:                                                          # the labels do not depend on the image's order
        assert all(torch.equal(p, q) for p, q in zip(res[0][1:], res[1][1:]))
    return res


def check_sweep(device, shape):
    from cfun_amd import sample
    img, lab = volume(shape, sum(shape))
    amap = sample.affine_map(13, shape[1], shape[2])
    check_case(device, img, lab, field((3, 3, 3), 7), amap, (False, True, False))
    check_case(device, img, lab, None, None)                                    # identity: the source comes back
    got = sample.warp_and_box(torch.from_numpy(img).to(device), torch.from_numpy(lab).to(device), sample.Warp())
    assert torch.equal(_bits(got[0]), torch.from_numpy(img).view(torch.int32)) and torch.equal(got[1].cpu(), torch.from_numpy(lab))


def check_cells_per_brick(device):
    """The first brick spans one, two and four control cells on every axis (counted on the restatement's step 1)."""
    from cfun_amd import sample
    img, lab = volume(SPAN_SHAPE, 11, "full")
    for want, g in SPANS.items():
        for n, ga, tile in zip(SPAN_SHAPE, g, (WZ, WY, WX)):
            cells = wr.control(n, ga)[0][:tile]
            assert len(set(cells.tolist())) == want, (want, n, ga, tile)
        check_case(device, img, lab, field(g, 12 + want), sample.affine_map(-7, SPAN_SHAPE[1], SPAN_SHAPE[2], scale=(1.1, 0.9)))


def check_grid_extents(device):
    """Grid extents 2, 3 and the query's value, on a volume of several bricks and on one smaller than the grid itself (the whole
    grid then sits under one brick: the LDS block at its largest); mixed extents."""
    top = max_grid()
    assert top >= 9 and top == SRC_MAX_GRID
    for shape in ((6, 10, 36), (3, 5, 7)):
        img, lab = volume(shape, 13, "full")
        for g in ((2, 2, 2), (3, 3, 3), (top, top, top), (2, top, 3)):
            check_case(device, img, lab, field(g, 14, 0.7))


def check_grid_against_brick(device):
    """Cells of twice, once and a quarter of the brick's extent per axis."""
    img, lab = volume(CELL_SHAPE, 15)
    for name, g in CELL_GRIDS.items():
        cell = [(n - 1) / (k - 1) for n, k in zip(CELL_SHAPE, g)]
        ratio = [c / t for c, t in zip(cell, (WZ, WY, WX))]
        assert ratio == {"coarser": [2.0] * 3, "equal": [1.0] * 3, "finer": [0.25] * 3}[name]
        check_case(device, img, lab, field(g, 16, 1.0), None, (True, False, False))


def check_flips(device):
    from cfun_amd import sample
    shape = (6, 9, 13)
    img, lab = volume(shape, 17)
    grid, amap = field((3, 4, 3), 18, 1.0), sample.affine_map(13, shape[1], shape[2])
    seen = set()
    for flips in itertools.product((False, True), repeat=3):
        got = check_case(device, img, lab, grid, amap, flips)
        seen.add(got[1][0].cpu().numpy().tobytes())
        plain = check_case(device, img, lab, None, None, flips, orders=(0,))[0]
        want = img
        for a in range(3):
            want = np.flip(want, a) if flips[a] else want
        assert torch.equal(_bits(plain[0]), torch.from_numpy(np.ascontiguousarray(want)).view(torch.int32))
    assert len(seen) == 8


def check_angles_and_scales(device):
    """Eight angles, each zoomed in and out (scale above and below 1 on both in-plane axes)."""
    from cfun_amd import sample
    shape = (5, 18, 21)
    img, lab = volume(shape, 19, "full")
    grid = field((2, 3, 3), 20, 1.0)
    for k, angle in enumerate(ANGLES):
        for scale in ((1.25, 1.1), (0.8, 0.9)):
            check_case(device, img, lab, grid if k % 2 else None, sample.affine_map(angle, shape[1], shape[2], scale=scale))


def check_translations(device):
    """A translation that pushes the object partly out of the volume, and one that pushes it wholly out: the empty flag, zero
    boxes, an all-zero image."""
    from cfun_amd import sample
    shape = (6, 16, 36)
    img, lab = volume(shape, 21)
    part = check_case(device, img, lab, None, sample.affine_map(7, 16, 36, translate=(3, 20)))[1]
    assert int(part[4].cpu()) == 0 and part[2].cpu().tolist()[5] == 36 and 0 < int((part[1] != 0).sum()) < int((lab != 0).sum())
    gone = check_case(device, img, lab, field((2, 2, 2), 22, 0.5), sample.affine_map(0, 16, 36, translate=(0, 80)))[1]
    assert int(gone[4].cpu()) == 1 and not gone[2].cpu().any() and not gone[3].cpu().any() and not gone[0].cpu().any()


def check_boxes(device):
    """An object on each face, a one-plane object (the zero box, not empty), an empty source."""
    shape = (6, 10, 36)
    img = volume(shape, 23)[0]
    for axis in range(3):
        for side in (0, shape[axis] - 1):
            lab = np.zeros(shape, np.uint8)
            idx = [slice(2, 5), slice(3, 7), slice(10, 30)]
            idx[axis] = slice(side, side + 1) if axis else slice(min(side, shape[0] - 2), min(side, shape[0] - 2) + 2)
            lab[tuple(idx)] = 3
            got = check_case(device, img, lab, orders=(1,))[1]
            raw = got[2].cpu().tolist()
            assert raw[axis] == 0 if side == 0 else raw[3 + axis] == shape[axis], (axis, side, raw)
    lab = np.zeros(shape, np.uint8)
    lab[3, 2:8, 5:30] = 1
    got = check_case(device, img, lab, orders=(0,))[0]
    assert not got[2].cpu().any() and not got[3].cpu().any() and int(got[4].cpu()) == 0
    got = check_case(device, img, np.zeros(shape, np.uint8), field((3, 3, 3), 24))[1]
    assert not got[2].cpu().any() and not got[3].cpu().any() and int(got[4].cpu()) == 1


def check_non_finite(device):
    """A NaN source voxel spreads through zero weights under order 1 and stays one voxel under order 0; a NaN control value
    gives zeros."""
    img, lab = volume((4, 5, 6), 25, "full")
    img[2, 2, 3] = np.nan
    got = check_case(device, img, lab)
    assert int(torch.isnan(got[1][0]).sum()) == 8 and int(torch.isnan(got[0][0]).sum()) == 1
    grid = np.zeros((3, 2, 2, 2), np.float32)
    grid[1, 1, 0, 1] = np.nan
    got = check_case(device, img, lab, grid)
    assert not got[1][0].cpu().any() and not got[1][1].cpu().any() and int(got[1][4].cpu()) == 1
    grid = field((3, 3, 3), 26)
    grid[2, 0, 0, 0] = np.inf
    check_case(device, volume((9, 12, 40), 27)[0], volume((9, 12, 40), 27)[1], grid)


def check_repeatable(device):
    from cfun_amd import sample
    shape = (9, 20, 68)
    img, lab = volume(shape, 28)
    w = sample.Warp(field((4, 4, 5), 29, 2.0), sample.affine_map(-13, 20, 68), (False, False, True), 1)
    ti, tl = torch.from_numpy(img).to(device), torch.from_numpy(lab).to(device)
    a, b = sample.warp_and_box(ti, tl, w), sample.warp_and_box(ti, tl, w)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and all(torch.equal(p, q) for p, q in zip(a[1:], b[1:]))


def check_gpu_shape(device):
    """GPU only: 64 x 72 x 130 with a 6^3 grid at 13 degrees, both orders."""
    from cfun_amd import sample
    shape = (64, 72, 130)
    img, lab = volume(shape, 30)
    got = check_case(device, img, lab, field((6, 6, 6), 31, 2.0), sample.affine_map(13, 72, 130))
    assert int(got[1][4].cpu()) == 0


def check_equals_frame_rotate_resize(device):
    """A zero grid, no flips, order 0 and map = rotation_map(angle, H, W) against cfun_sample_lits given the same volume as an
    [H,W,D] view with frame = source = output and normalise off: image, labels and both boxes bit for bit, at four angles."""
    from cfun_amd import sample
    shape = (7, 22, 36)
    img, lab = volume(shape, 32)
    ti, tl = torch.from_numpy(img).to(device), torch.from_numpy(lab).to(device)
    hwd = (shape[1], shape[2], shape[0])
    for angle in (7, -13, 20, 90):
        amap = sample.rotation_map(angle, shape[1], shape[2])
        a = sample.warp_and_box(ti, tl, sample.Warp(np.zeros((3, 2, 3, 2), np.float32), amap, (False, False, False), 0))
        b = sample.frame_rotate_resize(ti.permute(1, 2, 0), tl.permute(1, 2, 0), hwd, hwd, angle=angle, normalise=False)
        assert torch.equal(_bits(a[0]), _bits(b[0])), angle
        assert all(torch.equal(p, q) for p, q in zip(a[1:], b[1:])), angle
        assert int((a[1] != tl).sum()) > 0


# --------------------------------------------------------------------------------------------------------- the C entry itself
OUTPUTS = (("image", torch.float32, -7.0), ("labels", torch.uint8, 201), ("raw_box", torch.int32, -77), ("box", torch.int32, -78),
           ("empty", torch.int32, -79), ("workspace", torch.uint8, 203))


def raw_call(device, img, lab, grid=None, amap=None, flips=0, order=1, short=0, null=(), dims=None, gdims=None, shift=0,
             alias=None, margin=64):
    """cfun_sample_warp called directly, every output AND the workspace inside a larger buffer with ``margin`` canary elements
    either side, the workspace size passed ``short`` bytes below what cfun_sample_warp_workspace_bytes reports.  ``shift``: the
    image and label outputs start that many ELEMENTS later (a misaligned pointer); ``alias``: (output, input) names -- the
    output pointer is replaced by the input's."""
    from cfun_amd import _lib
    lib = _lib.load()
    ti, tl = torch.from_numpy(img).to(device), torch.from_numpy(lab).to(device)
    tg = torch.from_numpy(grid).to(device) if grid is not None else None
    i32 = C.c_int32 * 3
    dims = tuple(img.shape) if dims is None else dims
    if gdims is None and grid is not None:
        gdims = tuple(grid.shape[1:])
    need = lib.cfun_sample_warp_workspace_bytes(i32(*dims))
    n = img.size
    counts = dict(image=n + shift, labels=n + shift, raw_box=6, box=6, empty=1, workspace=max(int(need), 8))
    bufs, views = {}, {}
    for name, dt, canary in OUTPUTS:
        bufs[name] = torch.full((counts[name] + 2 * margin,), canary, dtype=dt, device=device)
        views[name] = bufs[name][margin:margin + counts[name]]
    views["image"], views["labels"] = views["image"][shift:], views["labels"][shift:]
    before = {k: v.cpu().clone() for k, v in bufs.items()}
    p = dict(image=_lib.ptr(ti), labels=_lib.ptr(tl), dims=i32(*dims), grid=_lib.ptr(tg), gdims=i32(*gdims) if gdims is not None else None,
             out_image=_lib.ptr(views["image"]), out_labels=_lib.ptr(views["labels"]), raw_box=_lib.ptr(views["raw_box"]),
             box=_lib.ptr(views["box"]), empty=_lib.ptr(views["empty"]), workspace=_lib.ptr(views["workspace"]))
    if alias is not None:
        p[alias[0]] = p[alias[1]] + alias[2]
    for k in null:
        p[k] = None
    cmap = (C.c_double * 6)(*amap) if amap is not None else None
    rc = lib.cfun_sample_warp(p["image"], p["labels"], p["dims"], p["grid"], p["gdims"], cmap, flips, order, p["out_image"],
                              p["out_labels"], p["raw_box"], p["box"], p["empty"], p["workspace"], max(int(need) - short, 0),
                              _lib.stream(ti))
    return rc, views, bufs, before, need, (ti, tl, tg)


def _canaries_intact(bufs, before, margin=64):
    for k, b in bufs.items():
        now = b.cpu()
        assert torch.equal(now[:margin], before[k][:margin]) and torch.equal(now[-margin:], before[k][-margin:]), "canary of " + k


def _untouched(bufs, before, what):
    for k, b in bufs.items():
        assert torch.equal(b.cpu(), before[k]), (what, k)


def _shaped(v, shape):
    return [v[k].reshape(shape) if k in ("image", "labels") else v[k] for k in ("image", "labels", "raw_box", "box", "empty")]


def check_misaligned_outputs(device):
    """W % 4 == 0 but the output pointers start one element late: the scalar store path, the same answer, canaries intact."""
    from cfun_amd import sample
    shape = (5, 9, 36)
    img, lab = volume(shape, 33)
    grid, amap = field((3, 3, 3), 34), sample.affine_map(13, 9, 36)
    for shift in (0, 1, 2):
        for order in (0, 1):
            rc, views, bufs, before, _, _ = raw_call(device, img, lab, grid, amap, 2, order, shift=shift)
            assert rc == 0
            _canaries_intact(bufs, before)
            if shift:
                assert views["image"].data_ptr() % 16 != 0
            compare(_shaped(views, shape), wr.warp(img, lab, grid, amap, (False, True, False), order), "shift %d" % shift)


def check_refusals(device):
    """Every refusal of the header: the return code, and nothing written -- outputs, workspace and the canaries either side."""
    from cfun_amd import _lib, sample
    lib = _lib.load()
    top = max_grid()
    shape = (5, 9, 36)
    img, lab = volume(shape, 35)
    grid, amap = field((3, 3, 3), 36), sample.affine_map(13, 9, 36)
    rc, views, bufs, before, need, _ = raw_call(device, img, lab, grid, amap, 5, 1)
    bricks = ((shape[2] - 1) // WX + 1) * ((shape[1] - 1) // WY + 1) * ((shape[0] - 1) // WZ + 1)
    assert rc == 0 and need == bricks * 6 * 4
    _canaries_intact(bufs, before)
    compare(_shaped(views, shape), wr.warp(img, lab, grid, amap, (True, False, True), 1))
    # grid and map may be NULL (gdims then as well)
    rc, views, bufs, before, _, _ = raw_call(device, img, lab, None, None, 0, 0)
    assert rc == 0
    compare(_shaped(views, shape), wr.warp(img, lab, None, None, (False, False, False), 0))
    big = field((top + 1, 3, 3), 37)
    nan_map = list(amap)
    nan_map[2] = float("nan")
    inf_map = list(amap)
    inf_map[4] = float("inf")
    bad = [dict(dims=(0, 9, 36)), dict(dims=(5, -1, 36)), dict(dims=(5, 9, 0)),
           dict(dims=(1 << 11, 1 << 10, 1 << 10)),                               # 2^31 voxels
           dict(dims=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)),
           dict(gdims=(1, 3, 3)), dict(gdims=(3, 3, 0)), dict(gdims=(3, -2, 3)),
           dict(grid=big), dict(gdims=(3, top + 1, 3)), dict(gdims=(3, 3, top + 1)),      # one past the query's value
           dict(amap=nan_map), dict(amap=inf_map),
           dict(order=2), dict(order=-1), dict(flips=8), dict(flips=-1),
           dict(alias=("out_image", "image", 0)), dict(alias=("out_image", "image", 4 * (img.size - 1))),
           dict(alias=("out_labels", "labels", 0)), dict(alias=("out_labels", "image", 8)), dict(alias=("out_image", "grid", 0)),
           dict(alias=("out_image", "labels", 0))] + \
          [dict(null=(k,)) for k in ("image", "labels", "dims", "gdims", "out_image", "out_labels", "raw_box", "box", "empty")]
    for kw in bad:
        args = dict(grid=grid, amap=amap, flips=5, order=1)
        args.update(kw)
        rc, _, bufs, before, _, held = raw_call(device, img, lab, **args)
        assert rc == EINVAL, (kw, rc)
        _untouched(bufs, before, kw)
        assert torch.equal(held[0].cpu().view(torch.int32), torch.from_numpy(img).view(torch.int32)), kw
        assert torch.equal(held[1].cpu(), torch.from_numpy(lab)), kw
    for kw in (dict(short=1), dict(null=("workspace",))):
        rc, _, bufs, before, _, _ = raw_call(device, img, lab, grid, amap, 5, 1, **kw)
        assert rc == EWORKSPACE, (kw, rc)
        _untouched(bufs, before, kw)
    i32 = C.c_int32 * 3
    assert lib.cfun_sample_warp_workspace_bytes(i32(5, 0, 4)) == 0 and lib.cfun_sample_warp_workspace_bytes(None) == 0
    assert lib.cfun_sample_warp_workspace_bytes(i32(1 << 11, 1 << 10, 1 << 10)) == 0
    assert lib.cfun_sample_warp_workspace_bytes(i32(2 ** 31 - 1, 1, 1)) == ((2 ** 31 - 2) // WZ + 1) * 24


def check_wrapper_preconditions(device):
    from cfun_amd import sample
    img, lab = volume((5, 9, 12), 38)
    ti, tl = torch.from_numpy(img).to(device), torch.from_numpy(lab).to(device)
    top = max_grid()
    with pytest.raises(ValueError, match="one shape"):
        sample.warp_and_box(ti, tl[:, :, :4], sample.Warp())
    with pytest.raises(ValueError, match="uint8 labels"):
        sample.warp_and_box(ti, tl.to(torch.int32), sample.Warp())
    with pytest.raises(ValueError, match="control grid"):
        sample.warp_and_box(ti, tl, sample.Warp(np.zeros((3, top + 1, 2, 2), np.float32)))
    with pytest.raises(ValueError, match="control grid"):
        sample.warp_and_box(ti, tl, sample.Warp(np.zeros((2, 2, 2, 2), np.float32)))
    with pytest.raises(ValueError, match="image_order"):
        sample.warp_and_box(ti, tl, sample.Warp(image_order=3))
    # a tensor grid on the device and a float64 image go through the wrapper's conversions
    g = field((3, 3, 3), 39)
    got = sample.warp_and_box(ti.double(), tl, sample.Warp(torch.from_numpy(g).to(device).double(), None, (False, False, True), 1))
    compare(got, wr.warp(img, lab, g, None, (False, False, True), 1))


# ------------------------------------------------------------------------------------------------------------ the draw (host)
def check_draw_warp():
    from cfun_amd import sample
    shape = (16, 32, 32)
    gen = torch.Generator().manual_seed(5)
    state = gen.get_state()
    a = sample.draw_warp(shape, gen, grid=(4, 5, 5), sigma=(1.0, 2.0, 2.0), angle=(-20, 20), scale_range=(0.9, 1.1), flip_p=(0.5, 0.5, 0.5))
    gen.set_state(state)
    b = sample.draw_warp(shape, gen, grid=(4, 5, 5), sigma=(1.0, 2.0, 2.0), angle=(-20, 20), scale_range=(0.9, 1.1), flip_p=(0.5, 0.5, 0.5))
    assert torch.equal(a.grid, b.grid) and a.map == b.map and a.flips == b.flips and a.factor == b.factor and a.image_order == b.image_order
    c = sample.draw_warp(shape, gen, grid=(4, 5, 5), sigma=(1.0, 2.0, 2.0), angle=(-20, 20))
    assert not torch.equal(a.grid, c.grid)                                      # the generator moved on
    assert a.grid.dtype == torch.float32 and tuple(a.grid.shape) == (3, 4, 5, 5) and len(a.map) == 6
    assert sample.draw_warp(shape, torch.Generator().manual_seed(1)).map is None
    assert sample.draw_warp(shape, torch.Generator().manual_seed(1), angle=13).map == sample.affine_map(13, 32, 32)
    # the half-cell bound, for sigma from a tenth of a cell to ten cells
    for g in ((5, 5, 5), (2, 9, 3), (4, 4, 12)):
        cell = [(n - 1) / (k - 1) for n, k in zip(shape, g)]
        for mult in (0.1, 0.5, 1.0, 3.0, 10.0):
            w = sample.draw_warp(shape, torch.Generator().manual_seed(int(mult * 10)), grid=g, sigma=[mult * c for c in cell])
            v = w.grid.numpy().astype(np.float64)
            for c in range(3):
                assert np.abs(np.diff(v[c], axis=c)).max() <= 0.5 * cell[c], (g, mult, c)
            assert 0.0 < w.factor <= 1.0
            assert w.factor < 1.0 or mult < 3.0, (g, mult, w.factor)            # (a difference of 3 cells' sigma exceeds half a cell)
            raw = sample.draw_warp(shape, torch.Generator().manual_seed(int(mult * 10)), grid=g, sigma=[mult * c * 1e-3 for c in cell])
            assert raw.factor == 1.0
            assert np.allclose(v, raw.grid.numpy().astype(np.float64) * 1e3 * w.factor, rtol=1e-5, atol=1e-9)
    w = sample.draw_warp((1, 32, 32), torch.Generator().manual_seed(2), sigma=50.0)     # an axis of extent 1 sets no bound
    assert 0.0 < w.factor < 1.0
    # extremes of flip_p
    for k in range(20):
        gen = torch.Generator().manual_seed(k)
        assert sample.draw_warp(shape, gen, flip_p=(0, 0, 0)).flips == (False, False, False)
        assert sample.draw_warp(shape, gen, flip_p=(1, 1, 1)).flips == (True, True, True)
        assert sample.draw_warp(shape, gen, flip_p=(1, 0, 1)).flips == (True, False, True)
    with pytest.raises(ValueError):
        sample.draw_warp(shape, grid=(1, 5, 5))


# ------------------------------------------------------------------------------------------------------------ the routes
def _count_calls(fn):
    """Run ``fn`` with cfun_amd.sample.warp_and_box counted: (result, calls)."""
    from cfun_amd import sample
    orig, calls = sample.warp_and_box, []

    def counted(*a, **kw):
        calls.append(1)
        return orig(*a, **kw)
    sample.warp_and_box = counted
    try:
        return fn(), len(calls)
    finally:
        sample.warp_and_box = orig


def check_route(device, route, seed=2):
    """``make_sample`` / ``make_sample_heart`` / ``make_sample_lits`` with ``augment=draw_warp(...)`` on the tiny configurations:
    every tensor of the dict equals the restated sample's -- the route's own un-normalised output (held to ITS restatement by its
    own tests) pushed through tests/sample_warp_ref.py, utils.mold_image on the heart routes, sample_ref's RPN targets on the NEW
    box -- the dict feeds train_epoch with finite losses equal to those of the restated sample; with ``augment=None`` the route
    returns what a second plain call returns and never reaches warp_and_box."""
    import copy
    import module_cases as mc
    from cfun_amd import sample, step, train, utils
    lits = route == "lits"
    cfg = mc.tiny_lits_config("beginning") if lits else mc.tiny_config("beginning")
    cfg.BATCH_SIZE = 1
    if lits:
        cfg.PAD_IMAGE_SHAPE = [44, 41, 24]
    torch.manual_seed(seed)
    net = step.CFUNHotPath(cfg).to(device)
    if not lits:
        b = cfg.UNET_MASK_BRANCH_CHANNEL
        gen = torch.Generator().manual_seed(1)
        masks = [torch.empty(cfg.TRAIN_ROIS_PER_IMAGE, c).bernoulli_(0.4, generator=gen) / 0.4 for c in (b, 2 * b, 4 * b, 8 * b, 16 * b)]
        net.mask.modified_u_net.dropout_masks = masks
    ref_net = copy.deepcopy(net)
    if not lits:
        ref_net.mask.modified_u_net.dropout_masks = masks
    rng = _rng(seed)
    dev = torch.device(device)
    anchors = net.anchors.to(device)
    keys = torch.from_numpy(rng.integers(0, 1 << 32, anchors.shape[0], dtype=np.uint64).astype(np.int64)).to(device)
    mx, mn = int(cfg.IMAGE_MAX_DIM), int(cfg.IMAGE_MIN_DIM)
    if lits:
        src = (36, 30, 17)
        image = rng.normal(0.0, 250.0, src).astype(np.float32)
        mask = np.zeros(src, np.int8)
        mask[6:30, 5:26, 2:15] = rng.integers(1, cfg.NUM_CLASSES, (24, 21, 13))
        angle, make = -13, sample.make_sample_lits
        h, w, d = [int(v) for v in cfg.IMAGE_SHAPE[:3]]
        before = sample.frame_rotate_resize(torch.from_numpy(image).to(dev), torch.from_numpy(mask).to(dev), cfg.PAD_IMAGE_SHAPE,
                                            (h, w, d), angle=angle, normalise=True)
    elif route == "heart":
        src = (40, 36, 20)
        image = np.asfortranarray(rng.integers(-1000, 1500, src).astype(np.int16))
        mask = np.zeros(src, np.int16, order="F")
        mask[8:32, 7:30, 3:17] = rng.integers(1, cfg.NUM_CLASSES, (24, 23, 14))
        angle, make = 13.0, sample.make_sample_heart
        before = sample.resize_rotate_box(torch.from_numpy(image).to(dev), torch.from_numpy(mask).to(dev), (mx, mx, mn), angle, zscore=False)
    else:
        src = (40, 36, 20)
        image = rng.normal(0.0, 1.0, src).astype(np.float32)
        mask = np.zeros(src, np.int32)
        mask[8:32, 7:30, 3:17] = rng.integers(1, cfg.NUM_CLASSES, (24, 23, 14))
        angle, make = 13.0, sample.make_sample
        r_image = utils.resize_image(torch.from_numpy(image)[..., None].to(dev), min_dim=mn, max_dim=mx, mode="self", device=dev)[0]
        r_mask = utils.resize_mask(torch.from_numpy(mask).to(dev), None, None, max_dim=mx, min_dim=mn, mode="self", device=dev)
        before = sample.rotate_and_box(r_image, r_mask, angle)
    shape = tuple(before[0].shape)
    warp = sample.draw_warp(shape, torch.Generator().manual_seed(7), grid=(3, 4, 4), sigma=(0.5, 1.0, 1.0), angle=(-10, 10),
                            scale_range=(0.95, 1.05), flip_p=(0, 0, 1))
    assert warp.flips == (False, False, True) and warp.map is not None

    s, calls = _count_calls(lambda: make(image, mask, angle, cfg, anchors, keys=keys, augment=warp))
    assert calls == 1
    (p1, c1), (p2, c2) = [_count_calls(lambda: make(image, mask, angle, cfg, anchors, keys=keys, augment=aug)) for aug in (None, None)]
    assert c1 == 0 and c2 == 0 and sorted(p1) == sorted(p2) == sorted(s)
    for k in p1:
        if torch.is_tensor(p1[k]):
            same = torch.equal(_bits(p1[k]), _bits(p2[k])) if p1[k].dtype == torch.float32 else torch.equal(p1[k], p2[k])
            assert same, k
    assert not torch.equal(p1["gt_labels"], s["gt_labels"])

    r_img, r_lab, r_raw, r_box, r_empty = wr.warp(before[0].cpu().numpy(), before[1].cpu().numpy(), warp.grid.numpy(), warp.map,
                                                  warp.flips, warp.image_order)
    assert r_empty == 0
    match, bbox, counts = sr.build_rpn_targets(anchors.cpu().numpy(), r_box[None].astype(np.float64), cfg.RPN_TRAIN_ANCHORS_PER_IMAGE,
                                               cfg.RPN_BBOX_STD_DEV, keys.cpu().numpy())
    assert (match == 1).any()
    t_img = torch.from_numpy(r_img).to(dev)
    nfg = cfg.NUM_CLASSES - 1
    rs = dict(image=(t_img if lits else utils.mold_image(t_img))[None, None], gt_class_ids=torch.arange(1, nfg + 1, device=dev),
              gt_boxes=torch.from_numpy(np.tile(r_box.astype(np.float32), (nfg, 1))).to(dev), gt_labels=torch.from_numpy(r_lab).to(dev),
              rpn_match=torch.from_numpy(match.reshape(1, -1, 1)).to(dev), rpn_bbox_t=torch.from_numpy(bbox.astype(np.float32)[None]).to(dev))
    for k in ("image", "gt_class_ids", "gt_boxes", "gt_labels", "rpn_match", "rpn_bbox_t"):
        assert s[k].dtype == rs[k].dtype and torch.equal(s[k], rs[k]), k
    assert s["raw_box"].cpu().tolist() == r_raw.tolist() and s["rpn_counts"].cpu().tolist() == counts.tolist()
    assert int(s["empty"].cpu()) == 0

    def one_step(n, smp):
        opt = train.make_optimizer(n, cfg, bucket_bytes=1 << 16)
        torch.manual_seed(11)                              # detection_target_layer's randperm draws
        return train.train_epoch(n, [smp], opt, 1, cfg)

    got, want = one_step(net, s), one_step(ref_net, rs)
    assert all(np.isfinite(v) for v in got), got
    assert got == want, (got, want)
    assert got[1] > 0 and got[2] > 0                       # the RPN losses saw the targets


# ------------------------------------------------------------------------------------------------------------ accounting
def header_symbols():
    """The same parse as test_abi.header_symbols, on include/cfun_sample_warp.h."""
    txt = open(os.path.join(ROOT, "include", "cfun_sample_warp.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(cfun_[a-z0-9_]+)\s*\(", txt)))


NO_LAUNCH = {"cfun_sample_warp_workspace_bytes": "host-side query: launches nothing, touches no device memory",
             "cfun_sample_warp_max_grid": "host-side query: a constant"}


def check_coverage(tier):
    from cfun_amd import _lib
    assert header_symbols() == sorted(_lib.WARP_SAMPLE_EXPORTS) == ["cfun_sample_warp", "cfun_sample_warp_max_grid",
                                                                    "cfun_sample_warp_workspace_bytes"]
    for other in (_lib.EXPORTS, _lib.SAMPLE_EXPORTS, _lib.LITS_SAMPLE_EXPORTS, _lib.NATIVE_EXPORTS, _lib.HEART_SAMPLE_EXPORTS,
                  _lib.TILE_EXPORTS, _lib.EVAL_EXPORTS, _lib.CC_EXPORTS, _lib.SURFACE_EXPORTS, _lib.LESION_EXPORTS, _lib.FILL_EXPORTS,
                  _lib.MORPH_EXPORTS):
        assert not set(_lib.WARP_SAMPLE_EXPORTS) & set(other)
    missed = sorted(set(_lib.WARP_SAMPLE_EXPORTS) - set(NO_LAUNCH) - guard.SEEN[tier])
    assert not missed, "warp entries that launch work but never ran under guard: %s" % missed
