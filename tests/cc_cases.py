"""Cases of the connected-component path (cfun_amd/components.py, cfun_amd/csrc/cc.hip) shared by test_cc_emu.py and
test_cc_gpu.py: the device against tests/cc_ref.py (scipy.ndimage.label), everything an integer and compared with torch.equal,
nothing excluded -- labels, cleaned map and statistics."""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest
import torch

import cc_ref as cr
import eval_cases as ec
import eval_ref as er
import guard
from conftest import ROOT

# [D,H,W] against the kernel's 8z x 8y x 64x tile: one voxel; one voxel over the tile in x alone; one over in every axis; less
# than a tile in z, two tiles and a voxel in y and in x; two tiles and a voxel in z, ragged in y and x; a single row of four tiles
SHAPES = [(1, 1, 1), (1, 1, 65), (9, 9, 65), (3, 17, 130), (17, 10, 67), (2, 1, 200)]
BIG = (64, 72, 130)                     # GPU tier only: 8 x 9 x 3 tiles, 599 040 voxels
TIE_SHAPE = (9, 17, 70)
CONNS = (6, 26)
MODES = ("class", "foreground")


def bernoulli(shape, p, k, seed, beyond=0):
    """Foreground with probability p, classes 1 .. k-1 (+ ``beyond`` ids past k-1) uniformly."""
    rng = np.random.default_rng(seed)
    fg = rng.random(shape) < p
    return np.where(fg, rng.integers(1, k + beyond, shape), 0).astype(np.uint8)


def serpentine(shape, value=1):
    """A one-voxel-wide path through every second row of every second plane, joined at alternating ends: ONE component under
    either connectivity, of the longest chain the volume allows, crossing every tile seam once per row."""
    d, h, w = shape
    v = np.zeros(shape, np.uint8)
    ys_fwd = list(range(0, h, 2))
    x_dir, fwd = 1, True
    zs = list(range(0, d, 2))
    for zi, z in enumerate(zs):
        ys = ys_fwd if fwd else ys_fwd[::-1]
        for yi, y in enumerate(ys):
            v[z, y, :] = value
            x_end = w - 1 if x_dir > 0 else 0
            x_dir = -x_dir
            if yi + 1 < len(ys):
                v[z, (y + ys[yi + 1]) // 2, x_end] = value
        if zi + 1 < len(zs):
            v[z + 1, ys[-1], x_end] = value
        fwd = not fwd
    return v


def diagonals(shape, value=2):
    """Space diagonals in all four directions of x and y, so that a component crosses tile corners and edges through every kind of
    backward neighbour (dx and dy of either sign with dz = -1)."""
    d, h, w = shape
    v = np.zeros(shape, np.uint8)
    n = min(d, h, w)
    for i in range(n):
        v[i, i, i] = value
        v[i, h - 1 - i, w - 1 - i] = value
        v[i, i, w - 1 - i] = value
        v[i, h - 1 - i, i] = value
    for i in range(min(d, h, max(w - 56, 0))):          # through the corner where the z, y and x seams at 8, 8, 64 meet
        v[i, i, 56 + i] = value
    return v


def checkerboard(shape, value=1):
    z, y, x = np.indices(shape)
    return (((z + y + x) % 2 == 0) * value).astype(np.uint8)


def blob_and_specks(shape):
    """A box of class 1 and specks of exactly 3 voxels (1 x 1 x 3) of the same class, two voxels clear of everything else."""
    d, h, w = shape
    v = np.zeros(shape, np.uint8)
    v[2:d - 5, 1:h - 2, 5:w - 7] = 1
    specks = [(0, 0, 0), (d - 1, h - 1, w - 3), (d - 2, 0, 62), (0, h - 1, 63), (d - 1, 0, 20), (d - 3, h - 1, 0)]
    for z, y, x in specks:
        v[z, y, x:x + 3] = 1
    return v, 3, len(specks)


def check_case(device, pred, k, conn, by, largest_only=True, min_voxels=0, ref=None):
    """One map through label_components and clean_components against cc_ref; returns (labels, cleaned, stats) of the device."""
    from cfun_amd import components
    t = torch.from_numpy(np.ascontiguousarray(pred)).to(device)
    want_lab, want_out, want_stats = ref if ref is not None else cr.clean(pred, k, conn, by, largest_only, min_voxels)
    tag = "%s k %d conn %d %s largest %s min %d" % (pred.shape, k, conn, by, largest_only, min_voxels)
    lab = components.label_components(t, conn, by)
    assert lab.dtype == torch.int32 and tuple(lab.shape) == pred.shape and lab.device == t.device
    assert torch.equal(lab.cpu(), torch.from_numpy(want_lab)), "labels: " + tag
    out, stats = components.clean_components(t, k, conn, by, largest_only, min_voxels)
    assert out.dtype == torch.uint8 and tuple(out.shape) == pred.shape and stats.dtype == torch.int64 and tuple(stats.shape) == (k, 3)
    assert out.device == t.device and stats.device == t.device
    assert torch.equal(stats.cpu(), torch.from_numpy(want_stats)), "stats: %s\n%s\n%s" % (tag, stats.cpu(), want_stats)
    assert torch.equal(out.cpu(), torch.from_numpy(want_out)), "cleaned: " + tag
    assert torch.equal(t.cpu(), torch.from_numpy(pred)), "the input was written to: " + tag
    return lab, out, stats


def check_all_ways(device, pred, k, **kw):
    for conn in CONNS:
        for by in MODES:
            check_case(device, pred, k, conn, by, **kw)


def check_bernoulli_shape(device, shape):
    seed = 100 + shape[0] * 31 + shape[1] * 7 + shape[2]
    for p in (0.2, 0.45, 0.7):
        for k in (3, 8):
            check_all_ways(device, bernoulli(shape, p, k, seed + k), k)
    check_all_ways(device, bernoulli(shape, 0.45, 3, seed), 3, largest_only=False, min_voxels=3)


def check_random_tie(device):
    """A random draw in which several components tie for largest: the tie rule on data nobody arranged.  That the draw HAS the tie
    is a property of the data, asserted on the reference."""
    pred = bernoulli(TIE_SHAPE, 0.45, 8, 0)
    lab, _, stats = cr.clean(pred, 8, 6, "class")
    tied = [int((np.bincount(lab[pred == c]) == stats[c, 1]).sum()) for c in range(1, 8)]
    assert max(tied) >= 3 and sum(t >= 2 for t in tied) >= 2, "test setup: this draw has no tie for largest: %s" % tied
    check_all_ways(device, pred, 8)
    check_all_ways(device, pred, 3)                     # the same map with classes 3 .. 7 in no group


def check_hand_tie(device):
    v = np.zeros((9, 9, 130), np.uint8)
    v[8, 1, 62:66] = 1                                   # 4 voxels across the x seam, the LARGER first index
    v[0, 8, 126:130] = 1                                 # 4 voxels at the far end of a row, the smaller first index
    v[4, 4, 0:3] = 1
    for conn in CONNS:
        for by in MODES:
            _, out, stats = check_case(device, v, 2, conn, by)
            assert out.cpu().numpy().sum() == 4 and bool(out[0, 8, 126:130].all())
            assert stats.cpu().tolist() == ([[0, 0, 0], [3, 4, 7]] if by == "class" else [[3, 4, 7], [0, 0, 0]])


def check_serpentine(device, shape):
    v = serpentine(shape)
    for conn in CONNS:
        for by in MODES:
            lab, out, stats = check_case(device, v, 2, conn, by)
            assert torch.equal(lab.cpu(), torch.from_numpy(v.astype(np.int32)))          # one component rooted at voxel 0
            assert int(stats.cpu()[1 if by == "class" else 0, 0]) == 1


def check_full_and_empty(device, shape):
    full = np.full(shape, 2, np.uint8)
    n = int(np.prod(shape))
    for conn in CONNS:
        for by in MODES:
            lab, out, stats = check_case(device, full, 3, conn, by, min_voxels=n)
            assert bool((lab == 1).all()) and bool((out == 2).all())
            assert stats.cpu().tolist()[2 if by == "class" else 0] == [1, n, 0]
            _, out, stats = check_case(device, full, 3, conn, by, min_voxels=n + 1)
            assert not out.cpu().any() and stats.cpu().tolist()[2 if by == "class" else 0] == [1, n, n]
            lab, out, stats = check_case(device, np.zeros(shape, np.uint8), 3, conn, by)
            assert not lab.cpu().any() and not out.cpu().any() and not stats.cpu().any()


def check_diagonal_checkerboard(device):
    check_all_ways(device, diagonals((17, 17, 67)), 3)
    check_all_ways(device, diagonals((17, 17, 67)), 3, largest_only=False, min_voxels=2)
    check_all_ways(device, checkerboard((9, 9, 65)), 2)
    cb = checkerboard((9, 9, 65)) * bernoulli((9, 9, 65), 1.0, 3, 3)          # every voxel its own class-mode component under 6
    check_all_ways(device, cb, 3)
    both = np.where(checkerboard((9, 9, 65)) > 0, 1, 2).astype(np.uint8)      # no background: 4096 labels in one tile under 6
    check_all_ways(device, both, 3)


def check_blob_and_specks(device):
    v, speck, nspecks = blob_and_specks((17, 10, 67))
    blob = int(v.sum()) - speck * nspecks
    for min_voxels in (speck - 1, speck, speck + 1):
        for largest_only in (False, True):
            check_all_ways(device, v, 2, largest_only=largest_only, min_voxels=min_voxels)
    _, out, stats = check_case(device, v, 2, 26, "class", largest_only=False, min_voxels=speck)
    assert int(out.sum()) == blob + speck * nspecks and stats.cpu().tolist()[1] == [nspecks + 1, blob, 0]
    _, out, stats = check_case(device, v, 2, 26, "class", largest_only=False, min_voxels=speck + 1)
    assert int(out.sum()) == blob and stats.cpu().tolist()[1] == [nspecks + 1, blob, speck * nspecks]


def check_values_beyond_k(device):
    pred = bernoulli((9, 9, 65), 0.45, 3, 11, beyond=3)                       # ids 1 .. 5 with K = 3
    assert (pred >= 3).any()
    check_all_ways(device, pred, 3)
    _, out, _ = check_case(device, pred, 3, 26, "class")
    assert np.array_equal(out.cpu().numpy()[pred >= 3], pred[pred >= 3])      # copied through
    pred[0, 0, 0] = 255
    check_all_ways(device, pred, 3, largest_only=False, min_voxels=2)
    check_all_ways(device, pred, 15)


def check_repeatable(device, shape):
    from cfun_amd import components
    t = torch.from_numpy(bernoulli(shape, 0.45, 8, 77)).to(device)
    for conn in CONNS:
        a, b = components.label_components(t, conn, "class"), components.label_components(t, conn, "class")
        assert torch.equal(a, b)
        (o1, s1), (o2, s2) = components.clean_components(t, 8, conn), components.clean_components(t, 8, conn)
        assert torch.equal(o1, o2) and torch.equal(s1, s2)


def check_big(device):
    """GPU tier only: several hundred tiles, so that workgroups really do run at the same time."""
    check_all_ways(device, bernoulli(BIG, 0.45, 8, 5), 8)
    check_serpentine(device, BIG)
    check_full_and_empty(device, BIG)
    check_repeatable(device, BIG)


def check_zero_sized_and_c_entry(device):
    from cfun_amd import _lib, components
    for dims in ((0, 5, 7), (5, 0, 7), (5, 7, 0)):
        pred = torch.zeros(dims, dtype=torch.uint8, device=device)
        lab = components.label_components(pred)
        assert tuple(lab.shape) == dims and lab.dtype == torch.int32
        out, stats = components.clean_components(pred, 8)
        assert tuple(out.shape) == dims and tuple(stats.shape) == (8, 3) and not stats.cpu().any()
    lib = _lib.load()
    assert lib.cfun_cc_workspace_bytes(0, 5, 7, 8) == 0 and lib.cfun_cc_workspace_bytes(5, 7, 0, 8) == 0
    # rejected by the C entries with nothing launched: the outputs keep their sentinel
    pred = torch.ones((2, 3, 4), dtype=torch.uint8, device=device)
    labels = torch.full((2, 3, 4), -7, dtype=torch.int32, device=device)
    out = torch.full((2, 3, 4), 77, dtype=torch.uint8, device=device)
    stats = torch.full((15, 3), -7, dtype=torch.int64, device=device)
    ws = _lib.workspace(lib.cfun_cc_workspace_bytes(2, 3, 4, 8), pred)
    i32 = C.c_int32 * 3
    p, st = _lib.ptr, _lib.stream(pred)
    big = ((2048, 1024, 1024), (1, 1 << 16, 1 << 15), (1, 1, (1 << 31) - 1), (1 << 30, 1 << 30, 1 << 30), (2, -3, 4))
    for dims in big:
        assert lib.cfun_cc_label(p(pred), i32(*dims), 26, 0, p(labels), p(ws), ws.numel(), st) == -1, dims
        assert lib.cfun_cc_filter(p(pred), p(labels), i32(*dims), 8, 0, 1, 0, p(out), p(stats), p(ws), ws.numel(), st) == -1, dims
        assert lib.cfun_cc_workspace_bytes(*dims, 8) == 0
    for conn, mode in ((18, 0), (0, 0), (26, 2), (6, -1)):
        assert lib.cfun_cc_label(p(pred), i32(2, 3, 4), conn, mode, p(labels), p(ws), ws.numel(), st) == -1, (conn, mode)
    for k, mode, mv in ((0, 0, 0), (16, 0, 0), (8, 2, 0), (8, 0, -1)):
        assert lib.cfun_cc_filter(p(pred), p(labels), i32(2, 3, 4), k, mode, 1, mv, p(out), p(stats), p(ws), ws.numel(), st) == -1
    assert lib.cfun_cc_workspace_bytes(2, 3, 4, 0) == 0 and lib.cfun_cc_workspace_bytes(2, 3, 4, 16) == 0
    assert lib.cfun_cc_filter(p(pred), p(labels), i32(2, 3, 4), 8, 0, 1, 0, p(out), p(stats), p(ws), ws.numel() - 1, st) == -2
    assert bool((labels.cpu() == -7).all()) and bool((out.cpu() == 77).all()) and bool((stats.cpu() == -7).all())
    # the largest volume the entries accept is one voxel short of 2^31 - 1: the size query answers it, nothing is allocated
    assert lib.cfun_cc_workspace_bytes(1, 1, (1 << 31) - 2, 8) > 4 * ((1 << 31) - 2)


def check_wrapper_preconditions(device):
    from cfun_amd import _lib, components
    pred = torch.zeros((4, 5, 6), dtype=torch.uint8, device=device)
    for fn in (components.label_components, lambda t, *a, **kw: components.clean_components(t, 8, *a, **kw)):
        with pytest.raises(ValueError, match="uint8"):
            fn(pred.to(torch.int32))
        with pytest.raises(ValueError, match=r"\[D,H,W\]"):
            fn(pred[0])
        with pytest.raises(ValueError, match="connectivity"):
            fn(pred, 18)
        with pytest.raises(ValueError, match="by must be"):
            fn(pred, 26, "organ")
        huge = torch.zeros(1, dtype=torch.uint8, device=device).expand(2048, 1024, 1024)      # a view: nothing is allocated
        with pytest.raises(ValueError, match=r"2\^31"):
            fn(huge)
        with pytest.raises(RuntimeError, match="contiguous"):
            fn(pred.permute(2, 1, 0).contiguous().permute(2, 1, 0))
    for k in (0, 16, -1):
        with pytest.raises(ValueError, match="num_classes"):
            components.clean_components(pred, k)
    with pytest.raises(ValueError, match="min_voxels"):
        components.clean_components(pred, 8, min_voxels=-1)
    for kw in (dict(connectivity=18), dict(by="organ"), dict(min_voxels=-1)):
        with pytest.raises(ValueError):
            components.Postprocess(**kw)
    pp = components.Postprocess(6, "foreground", False, 5)
    assert pp == components.Postprocess(6, "foreground", False, 5) and pp != components.Postprocess()
    assert (pp.connectivity, pp.by, pp.largest_only, pp.min_voxels) == (6, "foreground", False, 5)
    d = components.Postprocess()
    assert (d.connectivity, d.by, d.largest_only, d.min_voxels) == (26, "class", True, 0)
    if not _lib.is_emulator():
        with pytest.raises(RuntimeError, match="CPU tensor"):
            components.label_components(pred.cpu())


# ------------------------------------------------------------------------------------------------- detect_original / run_test
def _file_bytes(path):
    """Byte for byte; of a .gz the bytes it holds (the gzip header carries the time of writing)."""
    raw = open(path, "rb").read()
    return gzip.decompress(raw) if path.endswith(".gz") else raw


def _same_results(a, b):
    for key in ("per_class_ious", "mean", "std", "mask_ious", "dice"):
        np.testing.assert_array_equal(a[key], b[key])
    assert len(a["results"]) == len(b["results"])
    for ra, rb in zip(a["results"], b["results"]):
        assert set(ra) == set(rb) == {"rois", "class_ids", "scores", "mask_device", "empty"}
        assert ra["empty"] == rb["empty"] and torch.equal(ra["mask_device"], rb["mask_device"])
        for key in ("rois", "class_ids", "scores"):
            np.testing.assert_array_equal(ra[key], rb[key])
    assert [os.path.basename(p) for p in a["saved"]] == [os.path.basename(p) for p in b["saved"]]
    for pa, pb in zip(a["saved"], b["saved"]):
        assert _file_bytes(pa) == _file_bytes(pb)


def _check_postprocessed(r, base, labels, k, pp):
    for i, res in enumerate(r["results"]):
        raw = res["mask_device_raw"]
        assert torch.equal(raw, base["results"][i]["mask_device"]) and res["empty"] == base["results"][i]["empty"]
        _, want, want_stats = cr.clean(raw.cpu().numpy(), k, pp.connectivity, pp.by, pp.largest_only, pp.min_voxels)
        assert res["mask_device"].dtype == torch.uint8 and res["mask_device"].device == raw.device
        assert np.array_equal(res["mask_device"].cpu().numpy(), want)
        assert res["component_stats"].device == raw.device
        assert np.array_equal(res["component_stats"].cpu().numpy(), want_stats)
        if labels[i] is None:
            continue
        counts = er.confusion(want.transpose(1, 2, 0), labels[i], k)
        np.testing.assert_allclose(r["per_class_ious"][i], er.per_class_iou(counts), rtol=1e-15, atol=0)
        np.testing.assert_allclose(r["dice"][i], er.dice(counts), rtol=1e-15, atol=0)
        np.testing.assert_allclose(r["mask_ious"][i], er.mask_iou(counts), rtol=1e-15, atol=0)
    return [res["mask_device"] for res in r["results"]]


def check_run_test_heart(device, tmp_path):
    import module_cases as mc
    from cfun_amd import components, evaluate, nifti
    cfg = mc.tiny_config("beginning")
    k = int(cfg.NUM_CLASSES)
    net = ec._net(device, cfg, 1)
    img, lab = ec._case_arrays(2, k)
    cases = [(img, lab, ec.AFFINE, "first.nii")]
    dirs = [os.path.join(str(tmp_path), n) for n in ("plain", "none", "pp")]
    plain = evaluate.run_test(net, cases, save_dir=dirs[0], draw_bbox=True)
    none = evaluate.run_test(net, cases, save_dir=dirs[1], draw_bbox=True, postprocess=None)
    assert not plain["results"][0]["empty"], "test setup: no detection"
    _same_results(plain, none)
    pp = components.Postprocess(connectivity=6, by="class", largest_only=True, min_voxels=2)
    r = evaluate.run_test(net, cases, save_dir=dirs[2], draw_bbox=True, postprocess=pp)
    cleaned = _check_postprocessed(r, plain, [lab], k, pp)
    assert not torch.equal(cleaned[0], plain["results"][0]["mask_device"]), "test setup: the cleaning removed nothing"
    # the saved file is the CLEANED map with the box drawn, under the cleaned map's score
    path = os.path.join(dirs[2], str(r["per_class_ious"][0].mean()) + "_first.nii")
    assert r["saved"] == [path]
    want = ec._edges_numpy(cleaned[0].permute(1, 2, 0).cpu().numpy().astype(np.int32), r["results"][0]["rois"][0])
    assert np.array_equal(nifti.load(path).get_data(), want)
    # detect_original alone; and no detection at all: zeros in, zeros out
    res = evaluate.detect_original(net, torch.from_numpy(img)[..., None], components.Postprocess(26, "foreground"))
    _, want, want_stats = cr.clean(res["mask_device_raw"].cpu().numpy(), k, 26, "foreground")
    assert np.array_equal(res["mask_device"].cpu().numpy(), want) and np.array_equal(res["component_stats"].cpu().numpy(), want_stats)
    cfg.DETECTION_MIN_CONFIDENCE = 1.5
    res = evaluate.detect_original(net, torch.from_numpy(img)[..., None], pp)
    assert res["empty"] is True and not res["mask_device"].cpu().any() and not res["mask_device_raw"].cpu().any()
    assert tuple(res["component_stats"].shape) == (k, 3) and not res["component_stats"].cpu().any()


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
    dirs = [os.path.join(str(tmp_path), n) for n in ("plain", "none", "pp")]
    plain = evaluate.run_test(net, cases, save_dir=dirs[0], draw_bbox=True)
    none = evaluate.run_test(net, cases, save_dir=dirs[1], draw_bbox=True, postprocess=None)
    assert not plain["results"][0]["empty"], "test setup: no detection"
    _same_results(plain, none)
    pp = components.Postprocess(connectivity=26, by="foreground", largest_only=True)          # "liver u tumour" as one organ
    r = evaluate.run_test(net, cases, save_dir=dirs[2], draw_bbox=True, postprocess=pp)
    _check_postprocessed(r, plain, [label], k, pp)
    assert len(r["saved"]) == 1 and os.path.basename(r["saved"][0]) == str(r["per_class_ious"][0].mean()) + "_liver_7.nii.gz"
    # the detector-only stage: zeros in, zeros out, no mask scores
    cfg.STAGE = "beginning"
    assert net.detector_phase_only
    r = evaluate.run_test(net, cases[:1], postprocess=pp)
    res = r["results"][0]
    assert r["per_class_ious"].shape == (0, k - 1) and not res["mask_device"].cpu().any() and not res["mask_device_raw"].cpu().any()
    assert tuple(res["component_stats"].shape) == (k, 3) and not res["component_stats"].cpu().any()


# ------------------------------------------------------------------------------------------------------------ accounting
def cc_header_symbols():
    """The same parse as test_abi.header_symbols, on include/cfun_cc.h."""
    txt = open(os.path.join(ROOT, "include", "cfun_cc.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(cfun_[a-z0-9_]+)\s*\(", txt)))


CC_NO_LAUNCH = {"cfun_cc_workspace_bytes": "host-side query: launches nothing, touches no device memory"}


def check_coverage(tier):
    from cfun_amd import _lib
    assert cc_header_symbols() == sorted(_lib.CC_EXPORTS)
    for other in (_lib.EXPORTS, _lib.SAMPLE_EXPORTS, _lib.TILE_EXPORTS, _lib.EVAL_EXPORTS):
        assert not set(_lib.CC_EXPORTS) & set(other)
    missed = sorted(set(_lib.CC_EXPORTS) - set(CC_NO_LAUNCH) - guard.SEEN[tier])
    assert not missed, "component entries that launch work but never ran under guard: %s" % missed
