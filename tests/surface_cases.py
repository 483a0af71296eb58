"""Cases of the surface-distance path (cfun_amd/evaluate.py: surface_field, surface_distances, SurfaceScores;
cfun_amd/csrc/surface.hip) shared by test_surface_emu.py and test_surface_gpu.py: the device against tests/surface_ref.py.
The surface bytes, the float32 field, the counts, the maxima, the two order statistics and frac are compared for equality,
nothing excluded; the four fp64 sums within terms * 2^-52 * sum|terms| of the restatement's."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import eval_cases as ec
import guard
import surface_ref as sr
from conftest import ROOT

# [D,H,W]: one voxel; a line one voxel over a wave; one over the 8 x 8 x 64 tile of the neighbouring tiers in every axis; ragged in
# every axis; a single row
SHAPES = [(1, 1, 1), (1, 1, 65), (9, 9, 65), (3, 17, 130), (17, 10, 67), (2, 1, 200)]
BIG = (64, 72, 130)                     # GPU tier only: 599 040 voxels, several hundred workgroups per sweep
SPACINGS = [(1.0, 1.0, 1.0), (1.25, 0.78125, 0.78125), (2.5, 0.7, 0.7), (0.3, 1.7, 3.1)]      # unit, dyadic, two anisotropic
U = 2.0 ** -52


def kernel_constants():
    src = open(os.path.join(ROOT, "cfun_amd", "csrc", "surface.hip")).read()
    return {k: int(v) for k, v in re.findall(r"constexpr int (k\w+) = (\d+);", src)}


def slab_shapes():
    """One shape per sweep at the line length where the slab stops holding kMaxLines lines (the x sweep then takes 63 rows per
    workgroup, the y and z sweeps 32 columns instead of 64), and one per sweep with a line so long that the slab holds three
    rows / two columns.  Derived from the constants of surface.hip; the lines are the long axis, the volume stays small."""
    c = kernel_constants()
    assert c["kSlabFloats"] >= c["kMaxDim"] and c["kMaxLines"] == 64 and c["kNT"] == 256
    edge = c["kSlabFloats"] // c["kMaxLines"] + 1          # 161
    long = c["kSlabFloats"] // 4 + 1                        # 2561: 3 lines fit
    assert c["kSlabFloats"] // edge == c["kMaxLines"] - 1 and c["kSlabFloats"] // long == 3
    assert c["kSlabFloats"] // (edge + 1) == c["kMaxLines"] - 1 and c["kSlabFloats"] // (long + 1) == 3      # x: rows of W + 1 floats
    return [(2, 35, edge), (2, edge, 67), (edge, 2, 67), (1, 4, long), (1, long, 3), (long, 1, 3)]


def bernoulli(shape, p, k, seed, beyond=0):
    """Foreground with probability p, classes 1 .. k-1 (+ ``beyond`` ids past k-1) uniformly."""
    rng = np.random.default_rng(seed)
    fg = rng.random(shape) < p
    return np.where(fg, rng.integers(1, k + beyond, shape), 0).astype(np.uint8)


def ellipsoids(shape, k, shift):
    """An ellipsoid in bands, an organ-like case: class 1 + (band of the normalised radius), the centre moved by ``shift``."""
    d, h, w = shape
    z, y, x = np.indices(shape).astype(np.float64)
    r = np.sqrt(((z - d / 2.0 - shift[0]) / (0.45 * d)) ** 2 + ((y - h / 2.0 - shift[1]) / (0.4 * h)) ** 2 +
                ((x - w / 2.0 - shift[2]) / (0.35 * w)) ** 2)
    return np.where(r < 1.0, 1 + np.minimum((r * (k - 1)).astype(np.int64), k - 2), 0).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- reference
_FIELDS = {}


def ref_field(m, cls, spacing):
    """surface_ref's surface and field, computed once per (map, class, spacing) and shared (the guarded copies ask again)."""
    key = (m.shape, hash(m.tobytes()), int(cls), tuple(spacing))
    if key not in _FIELDS:
        s = sr.surface(m, cls)
        f = sr.field(s, spacing)
        s.setflags(write=False)
        f.setflags(write=False)
        _FIELDS[key] = (s, f)
    return _FIELDS[key]


def ref_stats(pred, label, k, spacing, q):
    zero = dict.fromkeys(sr.FIELDS, 0.0)
    zero["n_pred"] = zero["n_label"] = 0
    rows = [zero]
    for c in range(1, k):
        fields = (ref_field(pred, c, spacing)[1], ref_field(label, c, spacing)[1])
        rows.append(sr.class_stats(pred, label, c, spacing, q, fields=fields))
    return rows


# ------------------------------------------------------------------------------------------------------------------- checks
def check_field(device, m, cls, spacing):
    from cfun_amd import evaluate
    t = torch.from_numpy(np.ascontiguousarray(m)).to(device)
    s, f = evaluate.surface_field(t, cls, spacing)
    assert s.dtype == torch.uint8 and f.dtype == torch.float32 and tuple(s.shape) == tuple(f.shape) == m.shape
    assert s.device == t.device and f.device == t.device
    ws, wf = ref_field(m, cls, spacing)
    tag = "%s cls %d spacing %s" % (m.shape, cls, spacing)
    assert torch.equal(s.cpu(), torch.from_numpy(ws.astype(np.uint8))), "surface: " + tag
    assert torch.equal(f.cpu(), torch.from_numpy(np.array(wf))), "field: " + tag      # +inf == +inf; no NaN on either side
    assert torch.equal(t.cpu(), torch.from_numpy(m)), "the input was written to: " + tag
    return s, f


def records_of(stats):
    """The device records as a list of dicts (surface_ref.FIELDS)."""
    r = stats.cpu().numpy()
    assert r.dtype == np.int64 and r.shape[1] == len(sr.FIELDS)
    v = r[:, 2:].copy().view(np.float64)
    return [dict(zip(sr.FIELDS, [int(r[c, 0]), int(r[c, 1])] + [float(x) for x in v[c]])) for c in range(r.shape[0])]


def check_stats(device, pred, label, k, spacing, q=95.0, label_tensor=None):
    """surface_distances and SurfaceScores against the restatement; returns the device tensor."""
    from cfun_amd import evaluate
    p = torch.from_numpy(np.ascontiguousarray(pred)).to(device)
    lab = label_tensor if label_tensor is not None else torch.from_numpy(np.ascontiguousarray(label)).to(device)
    stats = evaluate.surface_distances(p, lab, k, spacing, q)
    assert stats.dtype == torch.int64 and tuple(stats.shape) == (k, 11) and stats.device == p.device
    got, want = records_of(stats), ref_stats(pred, label, k, spacing, q)
    tag = "%s k %d spacing %s q %s" % (pred.shape, k, spacing, q)
    assert got[0] == dict(zip(sr.FIELDS, [0, 0] + [0.0] * 9)), "row 0: " + tag
    sc = evaluate.SurfaceScores(stats)
    for c in range(1, k):
        g, w = got[c], want[c]
        for name in ("n_pred", "n_label", "max_sq_pl", "max_sq_lp", "q_lo_sq", "q_hi_sq", "frac"):
            assert g[name] == w[name], "%s of class %d: %r != %r, %s" % (name, c, g[name], w[name], tag)
        # a sum of n non-negative terms, each term and each addition rounded once: n * 2^-52 * sum covers both sides
        for name, n in (("sum_pl", w["n_pred"]), ("sum_lp", w["n_label"]), ("sumsq_pl", w["n_pred"]), ("sumsq_lp", w["n_label"])):
            assert abs(g[name] - w[name]) <= n * U * abs(w[name]), "%s of class %d: %r != %r, %s" % (name, c, g[name], w[name], tag)
        ws = sr.scores(w)
        empty = w["n_pred"] == 0 or w["n_label"] == 0
        # hausdorff and hd_percentile are functions of values that are equal; the others are quotients (and a root) of sums
        # with a relative error of n * 2^-52 at most each, plus a rounding per operation
        rel = (w["n_pred"] + w["n_label"] + 8) * U
        for name in ws:
            have = float(getattr(sc, name)[c - 1])
            if empty:
                assert np.isnan(have) and np.isnan(ws[name]), "%s of class %d: %r, %s" % (name, c, have, tag)
            elif name in ("hausdorff", "hd_percentile"):
                assert have == ws[name], "%s of class %d: %r != %r, %s" % (name, c, have, ws[name], tag)
            else:
                assert abs(have - ws[name]) <= rel * abs(ws[name]), "%s of class %d: %r != %r, %s" % (name, c, have, ws[name], tag)
        assert int(sc.n_pred[c - 1]) == w["n_pred"] and int(sc.n_label[c - 1]) == w["n_label"]
    assert torch.equal(p.cpu(), torch.from_numpy(pred)), "the prediction was written to: " + tag
    return stats


def _seed(shape):
    return 100 + shape[0] * 31 + shape[1] * 7 + shape[2]


def check_bernoulli_field(device, shape):
    seed = _seed(shape)
    for i, p in enumerate((0.02, 0.3, 0.7)):
        for k in (3, 8):
            m = bernoulli(shape, p, k, seed + k)
            for spacing in SPACINGS:
                for cls in (1, k - 1):
                    check_field(device, m, cls, spacing)


def check_bernoulli_stats(device, shape):
    seed = _seed(shape)
    for i, p in enumerate((0.02, 0.3, 0.7)):
        for j, k in enumerate((3, 8)):
            pred, label = bernoulli(shape, p, k, seed + k), bernoulli(shape, p, k, seed + 50 + k)
            for s, spacing in enumerate(SPACINGS):
                if k == 3 or s == (i + j) % len(SPACINGS):          # K = 8: one spacing per map, all four over the maps
                    check_stats(device, pred, label, k, spacing, q=(95.0, 50.0, 100.0, 0.0)[s])


def check_slab_shape(device, shape):
    """The shapes of slab_shapes(): a sparse and a dense map, the field of one class and the statistics."""
    for p, spacing in ((0.02, SPACINGS[2]), (0.3, SPACINGS[3])):
        pred, label = bernoulli(shape, p, 3, _seed(shape)), bernoulli(shape, p, 3, _seed(shape) + 1)
        check_field(device, pred, 1, spacing)
        check_stats(device, pred, label, 3, spacing)


def check_ellipsoids(device, shape=(17, 20, 67)):
    pred, label = ellipsoids(shape, 4, (0.0, 0.0, 0.0)), ellipsoids(shape, 4, (1.5, -2.0, 3.0))
    assert all((pred == c).any() and (label == c).any() for c in (1, 2, 3)), "test setup: a band is missing"
    for spacing in SPACINGS:
        check_field(device, pred, 2, spacing)
        check_stats(device, pred, label, 4, spacing)
    check_stats(device, pred, pred, 4, SPACINGS[2])                 # a map against itself: every distance is zero
    from cfun_amd import evaluate
    sc = evaluate.SurfaceScores(evaluate.surface_distances(torch.from_numpy(pred).to(device), torch.from_numpy(pred).to(device), 4,
                                                           SPACINGS[2]))
    assert not sc.hausdorff.any() and not sc.assd.any() and not sc.rmsd.any() and not sc.hd_percentile.any()


def check_full_and_empty(device, shape):
    full, zero = np.full(shape, 2, np.uint8), np.zeros(shape, np.uint8)
    for spacing in (SPACINGS[0], SPACINGS[2]):
        s, f = check_field(device, full, 2, spacing)
        d, h, w = shape
        inner = max(d - 2, 0) * max(h - 2, 0) * max(w - 2, 0)
        assert int(s.sum()) == d * h * w - inner                   # the faces of the volume are surface
        s, f = check_field(device, zero, 2, spacing)
        assert not s.cpu().any() and bool(torch.isinf(f.cpu()).all())
        s, f = check_field(device, full, 1, spacing)                # a class that is not there
        assert not s.cpu().any() and bool(torch.isinf(f.cpu()).all())
        for pred, label in ((full, full), (full, zero), (zero, full), (zero, zero)):
            stats = check_stats(device, pred, label, 3, spacing)
            got = records_of(stats)
            assert not any(got[1].values()) and (got[2]["n_pred"] > 0) == bool(pred.any())
            if not (pred.any() and label.any()):
                assert all(got[2][name] == 0.0 for name in sr.FIELDS[2:])


def check_absent_and_beyond(device):
    shape = (9, 9, 65)
    pred, label = bernoulli(shape, 0.3, 4, 5), bernoulli(shape, 0.3, 4, 6)
    pred[pred == 2] = 0                                             # class 2 in the label only, class 3 in the prediction only
    label[label == 3] = 0
    stats = check_stats(device, pred, label, 4, SPACINGS[2])
    got = records_of(stats)
    assert got[2]["n_pred"] == 0 and got[2]["n_label"] > 0 and got[3]["n_pred"] > 0 and got[3]["n_label"] == 0
    assert all(got[c][name] == 0.0 for c in (2, 3) for name in sr.FIELDS[2:])
    assert got[1]["n_pred"] > 0 and got[1]["sum_pl"] > 0.0
    # bytes >= K belong to no class, and border a class like any other byte
    pred, label = bernoulli(shape, 0.45, 3, 11, beyond=3), bernoulli(shape, 0.45, 3, 12, beyond=3)
    pred[0, 0, 0] = 255
    assert (pred >= 3).any() and (label >= 3).any()
    check_stats(device, pred, label, 3, SPACINGS[1])
    check_stats(device, pred, label, 15, SPACINGS[3])
    check_field(device, pred, 255, SPACINGS[0])
    check_field(device, pred, 5, SPACINGS[2])


def check_label_dtypes(device):
    """The wrapper's dense uint8 label: any dtype, any strides, ids outside [0, K) in no class."""
    shape = (9, 10, 33)
    pred, label = bernoulli(shape, 0.4, 4, 21), bernoulli(shape, 0.4, 4, 22, beyond=2).astype(np.int64)
    label[0, 0, :5] = (-1, -300, 256 + 1, 1 << 40, 4)               # none of them is class 1 (uint8 wrap-around would make 257 one)
    as_map = np.where((label >= 0) & (label < 4), label, 4).astype(np.uint8)
    for dtype in (torch.int64, torch.int32, torch.float32, torch.float64):
        lab = torch.from_numpy(label).to(device)
        if dtype == torch.int32:
            lab = lab.clamp(-(1 << 31), (1 << 31) - 1)
        check_stats(device, pred, as_map, 4, SPACINGS[2], label_tensor=lab.to(dtype))
    hwd = torch.from_numpy(np.ascontiguousarray(label.transpose(1, 2, 0))).to(device)          # the loader's [H,W,D]
    check_stats(device, pred, as_map, 4, SPACINGS[2], label_tensor=hwd.permute(2, 0, 1))
    check_stats(device, pred, as_map, 4, SPACINGS[2], label_tensor=torch.from_numpy(as_map).to(device))


def check_repeatable(device, shape):
    from cfun_amd import evaluate
    p, lab = [torch.from_numpy(bernoulli(shape, 0.3, 8, 77 + i)).to(device) for i in range(2)]
    a, b = [evaluate.surface_distances(p, lab, 8, SPACINGS[3], 95.0) for _ in range(2)]
    assert torch.equal(a, b), "two runs differ (the sums included)"
    (s1, f1), (s2, f2) = [evaluate.surface_field(p, 3, SPACINGS[3]) for _ in range(2)]
    assert torch.equal(s1, s2) and torch.equal(f1, f2)


def check_big(device):
    """GPU tier only: workgroups that really do run at the same time."""
    pred, label = bernoulli(BIG, 0.3, 3, 5), bernoulli(BIG, 0.3, 3, 6)
    check_field(device, pred, 1, SPACINGS[2])
    check_stats(device, pred, label, 3, SPACINGS[2])
    e1, e2 = ellipsoids(BIG, 3, (0.0, 0.0, 0.0)), ellipsoids(BIG, 3, (2.0, -3.0, 5.0))
    check_stats(device, e1, e2, 3, SPACINGS[3])
    check_repeatable(device, BIG)


def check_zero_sized_and_c_entry(device):
    from cfun_amd import _lib, evaluate
    for dims in ((0, 5, 7), (5, 0, 7), (5, 7, 0)):
        pred = torch.zeros(dims, dtype=torch.uint8, device=device)
        s, f = evaluate.surface_field(pred, 1, SPACINGS[0])
        assert tuple(s.shape) == dims and tuple(f.shape) == dims
        stats = evaluate.surface_distances(pred, pred, 8, SPACINGS[0])
        assert tuple(stats.shape) == (8, 11) and not stats.cpu().any()
        assert np.isnan(evaluate.SurfaceScores(stats).hausdorff).all()
    lib = _lib.load()
    assert lib.cfun_surface_workspace_bytes(0, 5, 7, 8) == 0 and lib.cfun_surface_workspace_bytes(5, 7, 0, 8) == 0
    # rejected by the C entries with nothing launched: the outputs keep their sentinel
    pred = torch.ones((2, 3, 4), dtype=torch.uint8, device=device)
    surf = torch.full((2, 3, 4), 77, dtype=torch.uint8, device=device)
    field = torch.full((2, 3, 4), -7.0, dtype=torch.float32, device=device)
    stats = torch.full((15, 11), -7, dtype=torch.int64, device=device)
    need = lib.cfun_surface_workspace_bytes(2, 3, 4, 8)
    assert need >= 10 * 24
    ws = _lib.workspace(need, pred)
    i32, f32 = C.c_int32 * 3, C.c_float * 3
    p, st = _lib.ptr, _lib.stream(pred)
    one = f32(1.0, 1.0, 1.0)

    def field_rc(dims=(2, 3, 4), cls=1, s2=one):
        return lib.cfun_surface_field(p(pred), i32(*dims), cls, s2, p(surf), p(field), p(ws), ws.numel(), st)

    def stats_rc(dims=(2, 3, 4), k=8, s2=one, qf=0.95, nbytes=None):
        return lib.cfun_surface_stats(p(pred), p(pred), i32(*dims), k, s2, qf, p(stats), p(ws), ws.numel() if nbytes is None else nbytes,
                                      st)

    for dims in ((2048, 1024, 1024), (4096, 4096, 128), (4097, 1, 1), (1, 4097, 1), (1, 1, 4097), (1, 1, (1 << 31) - 1), (2, -3, 4),
                 (-1, 3, 4), (2, 3, -4)):
        assert field_rc(dims=dims) == -1 and stats_rc(dims=dims) == -1, dims
        assert lib.cfun_surface_workspace_bytes(*dims, 8) == 0
    for cls in (0, 256, -1):
        assert field_rc(cls=cls) == -1, cls
    for k in (0, 16, -1):
        assert stats_rc(k=k) == -1 and lib.cfun_surface_workspace_bytes(2, 3, 4, k) == 0, k
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        for axis in range(3):
            s2 = f32(*[bad if i == axis else 1.0 for i in range(3)])
            assert field_rc(s2=s2) == -1 and stats_rc(s2=s2) == -1, (bad, axis)
    for qf in (-0.1, 1.0000001, float("nan"), float("inf")):
        assert stats_rc(qf=qf) == -1, qf
    assert stats_rc(nbytes=need - 1) == -2 and stats_rc(nbytes=0) == -2
    assert bool((surf.cpu() == 77).all()) and bool((field.cpu() == -7.0).all()) and bool((stats.cpu() == -7).all())
    # the edges that are accepted: K = 1 and K = 15, the percentile's two ends, the workspace exactly as reported
    assert stats_rc(k=1) == 0 and stats_rc(qf=1.0, nbytes=need) == 0
    assert bool((stats.cpu()[8:] == -7).all()) and not stats.cpu()[0].any()
    assert lib.cfun_surface_workspace_bytes(2, 3, 4, 15) <= need and stats_rc(k=15, qf=0.0) == 0
    assert int(stats.cpu()[1, 0]) == 24 and not stats.cpu()[2:, :2].any()
    assert field_rc(cls=255) == 0 and not surf.cpu().any()
    # the largest volume the entries accept: the size query answers it, nothing is allocated
    assert lib.cfun_surface_workspace_bytes(4096, 4096, 127, 8) > 10 * 4096 * 4096 * 127


def check_wrapper_preconditions(device):
    from cfun_amd import _lib, evaluate
    pred = torch.zeros((4, 5, 6), dtype=torch.uint8, device=device)
    sp = SPACINGS[0]
    def against_zeros(t, spacing=sp):
        return evaluate.surface_distances(t, torch.zeros(1, dtype=torch.uint8, device=device).expand(tuple(t.shape)), 8, spacing)

    for fn in (lambda t, spacing=sp: evaluate.surface_field(t, 1, spacing), against_zeros):
        with pytest.raises(ValueError, match="uint8"):
            fn(pred.to(torch.int32))
        with pytest.raises(ValueError, match=r"\[D,H,W\]"):
            fn(pred[0])
        with pytest.raises(ValueError, match=r"2\^31"):
            fn(torch.zeros(1, dtype=torch.uint8, device=device).expand(2048, 1024, 1024))      # a view: nothing is allocated
        with pytest.raises(ValueError, match="4096"):
            fn(torch.zeros(1, dtype=torch.uint8, device=device).expand(1, 1, 4097))
        with pytest.raises(RuntimeError, match="contiguous"):
            fn(pred.permute(2, 1, 0).contiguous().permute(2, 1, 0))
        for bad in ((1.0, 1.0), (1.0, 0.0, 1.0), (1.0, -2.0, 1.0), (float("nan"), 1.0, 1.0), (1.0, 1.0, float("inf")), (1e30, 1.0, 1.0)):
            with pytest.raises(ValueError, match="spacing"):
                fn(pred, bad)
    for cls in (0, 256, -1):
        with pytest.raises(ValueError, match="cls"):
            evaluate.surface_field(pred, cls, sp)
    for k in (0, 16, -1):
        with pytest.raises(ValueError, match="num_classes"):
            evaluate.surface_distances(pred, pred, k, sp)
    with pytest.raises(ValueError, match="differ in shape"):
        evaluate.surface_distances(pred, pred[:3], 8, sp)
    for q in (-1.0, 100.5, float("nan")):
        with pytest.raises(ValueError, match="percentile"):
            evaluate.surface_distances(pred, pred, 8, sp, q)
    with pytest.raises(ValueError, match="records"):
        evaluate.SurfaceScores(np.zeros((8, 10), np.int64))
    if not _lib.is_emulator():
        with pytest.raises(RuntimeError, match="CPU tensor"):
            evaluate.surface_field(pred.cpu(), 1, sp)
        with pytest.raises(ValueError, match="different devices"):
            evaluate.surface_distances(pred, pred.cpu(), 8, sp)
    assert evaluate.affine_spacing(ec.AFFINE) == (2.5, 0.8, 1.25)


# ----------------------------------------------------------------------------------------------------------------- run_test
TODAY = {"per_class_ious", "mean", "std", "total_mean", "mask_ious", "dice", "detect_time", "results", "saved"}


def _check_surface_keys(r, labels, k, q, spacing):
    """The new keys equal surface_ref applied to the returned map and the label."""
    n = len(labels)
    assert set(r) == TODAY | {"hausdorff", "hd95", "assd"}
    for key in ("hausdorff", "hd95", "assd"):
        assert r[key].shape == (n, k - 1) and r[key].dtype == np.float64
    for i, res in enumerate(r["results"]):
        pred = res["mask_device"].cpu().numpy()
        label = np.ascontiguousarray(np.asarray(labels[i]).transpose(2, 0, 1))
        as_map = np.where((label >= 0) & (label < k), label, k).astype(np.uint8)
        want = ref_stats(pred, as_map, k, spacing, q)
        sc = res["surface_scores"]
        for c in range(1, k):
            ws = sr.scores(want[c])
            rel = (want[c]["n_pred"] + want[c]["n_label"] + 8) * U
            for key, name in (("hausdorff", "hausdorff"), ("hd95", "hd_percentile"), ("assd", "assd")):
                have = r[key][i, c - 1]
                assert have == getattr(sc, name)[c - 1] or (np.isnan(have) and np.isnan(getattr(sc, name)[c - 1]))
                if np.isnan(ws[name]):
                    assert np.isnan(have), (key, c)
                elif name == "assd":
                    assert abs(have - ws[name]) <= rel * abs(ws[name]), (key, c, have, ws[name])
                else:
                    assert have == ws[name], (key, c, have, ws[name])
    return r


def check_run_test_heart(device, tmp_path):
    import module_cases as mc
    from cfun_amd import components, evaluate
    cfg = mc.tiny_config("beginning")
    k = int(cfg.NUM_CLASSES)
    net = ec._net(device, cfg, 1)
    img, lab = ec._case_arrays(2, k)
    cases = [(img, lab, ec.AFFINE, "first.nii")]
    spacing = (2.5, 0.8, 1.25)                                       # ec.AFFINE's column norms, as (sz, sy, sx)
    assert inspect.signature(evaluate.run_test).parameters["surface"].default is None
    plain = evaluate.run_test(net, cases, surface=None)
    assert set(plain) == TODAY and not plain["results"][0]["empty"], "test setup: no detection"
    assert set(plain["results"][0]) == {"rois", "class_ids", "scores", "mask_device", "empty"}
    r = _check_surface_keys(evaluate.run_test(net, cases, surface=True), [lab], k, 95.0, spacing)
    for key in ("per_class_ious", "mask_ious", "dice"):
        np.testing.assert_array_equal(r[key], plain[key])
    assert torch.equal(r["results"][0]["mask_device"], plain["results"][0]["mask_device"])
    assert np.isfinite(r["hausdorff"]).any(), "test setup: no class is present on both sides"
    _check_surface_keys(evaluate.run_test(net, cases, surface=50), [lab], k, 50.0, spacing)
    # with a post-processing step the CLEANED map is what is measured
    pp = components.Postprocess(connectivity=6, by="class", largest_only=True, min_voxels=2)
    r = _check_surface_keys(evaluate.run_test(net, cases, postprocess=pp, surface=True), [lab], k, 95.0, spacing)
    assert not torch.equal(r["results"][0]["mask_device"], plain["results"][0]["mask_device"]), "test setup: the cleaning removed nothing"
    with pytest.raises(ValueError, match="surface"):
        evaluate.run_test(net, cases, surface=101)


def check_run_test_lits(device, tmp_path):
    import module_cases as mc
    from cfun_amd import evaluate
    cfg = mc.tiny_lits_config("together", max_dim=64, min_dim=32)
    cfg.PAD_IMAGE_SHAPE = [80, 80, 40]
    k = int(cfg.NUM_CLASSES)
    net = ec._net(device, cfg, 2)
    rng = np.random.default_rng(9)
    image = rng.normal(0.0, 200.0, ec.SRC).astype(np.float32)
    label = np.zeros(ec.SRC, np.int32)
    label[5:30, 10:44, 2:15] = rng.integers(0, k, (25, 34, 13))
    cases = [(image, label, ec.AFFINE, "liver_7.nii.gz", (44, 52, 22))]
    plain = evaluate.run_test(net, cases, surface=None)
    assert set(plain) == TODAY and set(plain["results"][0]) == {"rois", "class_ids", "scores", "mask_device", "empty"}
    assert not plain["results"][0]["empty"], "test setup: no detection"
    r = _check_surface_keys(evaluate.run_test(net, cases, surface=True), [label], k, 95.0, (2.5, 0.8, 1.25))
    np.testing.assert_array_equal(r["per_class_ious"], plain["per_class_ious"])
    # the detector-only stage: no mask scores, no surface scores
    cfg.STAGE = "beginning"
    assert net.detector_phase_only
    r = evaluate.run_test(net, cases, surface=True)
    assert r["per_class_ious"].shape == (0, k - 1) and "surface_scores" not in r["results"][0]
    for key in ("hausdorff", "hd95", "assd"):
        assert r[key].shape == (0, k - 1)


# ------------------------------------------------------------------------------------------------------------ accounting
def surface_header_symbols():
    """The same parse as test_abi.header_symbols, on include/cfun_surface.h."""
    txt = open(os.path.join(ROOT, "include", "cfun_surface.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(cfun_[a-z0-9_]+)\s*\(", txt)))


SURFACE_NO_LAUNCH = {"cfun_surface_workspace_bytes": "host-side query: launches nothing, touches no device memory"}


def check_coverage(tier):
    from cfun_amd import _lib
    assert surface_header_symbols() == sorted(_lib.SURFACE_EXPORTS)
    for other in (_lib.EXPORTS, _lib.SAMPLE_EXPORTS, _lib.TILE_EXPORTS, _lib.EVAL_EXPORTS, _lib.CC_EXPORTS):
        assert not set(_lib.SURFACE_EXPORTS) & set(other)
    missed = sorted(set(_lib.SURFACE_EXPORTS) - set(SURFACE_NO_LAUNCH) - guard.SEEN[tier])
    assert not missed, "surface entries that launch work but never ran under guard: %s" % missed
