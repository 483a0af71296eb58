"""Cases of the lesion-scoring path (cfun_amd/lesions.py, cfun_amd/csrc/lesion.hip) shared by test_lesion_emu.py and
test_lesion_gpu.py: the device against tests/lesion_ref.py (scipy.ndimage.label, find_objects, a numpy contingency count),
everything an integer and compared with torch.equal, nothing excluded -- ranks, count, table, overlap.  The sizes at which the
kernels change path are read from lesion.hip itself."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import cc_cases as cc
import eval_cases as ec
import guard
import lesion_ref as lr
from conftest import ROOT


def _const(name):
    src = open(os.path.join(ROOT, "cfun_amd", "csrc", "lesion.hip")).read()
    m = re.search(r"constexpr int (?:\w+ = [^,;]+, )*%s = (\d+)\s*[,;]" % name, src)
    assert m, "lesion.hip no longer defines %s as a plain number" % name
    return int(m.group(1))


CHUNK = _const("kChunk")              # voxels per chunk of the root scan
SCAN_NT = _const("kScanNT")           # chunks the scan workgroup takes per round
PAIR_SLOTS = _const("kPairSlots")     # slots of the overlap kernel's LDS table
STEP = _const("kNT") * _const("kU")   # voxels an overlap workgroup takes per step
MIN_STEPS = _const("kMinSteps")       # steps it takes before a second workgroup is launched
MANY_CHUNKS = (65, 130, 131)          # 1 106 950 voxels: one round of the scan workgroup and a ragged second
CONNS = (6, 26)
MODES = ("class", "foreground")


def check_constants():
    """The shapes below straddle these values; a changed constant has to be met by new shapes, not by silence."""
    assert CHUNK == 4096 and SCAN_NT == 256 and PAIR_SLOTS == 2048 and STEP == 1024 and MIN_STEPS == 16
    n = MANY_CHUNKS[0] * MANY_CHUNKS[1] * MANY_CHUNKS[2]
    assert SCAN_NT < -(-n // CHUNK) < 2 * SCAN_NT


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def check_rank(device, pred, conn, by, cap=1023):
    """One map through rank_components against lesion_ref; returns the device's (ranks, table, count)."""
    from cfun_amd import lesions
    t = _dev(pred, device)
    want_ranks, n = lr.rank(pred, conn, by)
    want_count, want_table = lr.table(pred, want_ranks, n, cap)
    tag = "%s conn %d %s cap %d (%d components)" % (pred.shape, conn, by, cap, n)
    ranks, table, count = lesions.rank_components(t, conn, by, cap)
    assert ranks.dtype == torch.int32 and tuple(ranks.shape) == pred.shape and ranks.device == t.device
    assert count.dtype == torch.int64 and tuple(count.shape) == (2,) and count.device == t.device
    assert table.dtype == torch.int64 and tuple(table.shape) == (cap + 2, lr.FIELDS) and table.device == t.device
    assert torch.equal(count.cpu(), torch.from_numpy(want_count)), "count: %s: %s" % (tag, count.cpu().tolist())
    assert torch.equal(ranks.cpu(), torch.from_numpy(want_ranks)), "ranks: " + tag
    got = table.cpu()
    if not torch.equal(got, torch.from_numpy(want_table)):
        bad = (got != torch.from_numpy(want_table)).any(dim=1).nonzero().flatten().tolist()
        raise AssertionError("table: %s: rows %s\n%s\n%s" % (tag, bad[:6], got[bad[:6]], want_table[bad[:6]]))
    assert torch.equal(t.cpu(), torch.from_numpy(pred)), "the input was written to: " + tag
    return ranks, table, count


def check_rank_all_ways(device, pred, cap=1023):
    for conn in CONNS:
        for by in MODES:
            check_rank(device, pred, conn, by, cap)


def check_rank_chunk_edges(device):
    """V = chunk - 1, chunk, chunk + 1, and two chunks with a ragged third; a root on the first and on the last voxel of a chunk."""
    for v in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 37):
        check_rank_all_ways(device, cc.bernoulli((1, 1, v), 0.3, 3, v), cap=4095)
    edge = np.zeros((2, 1, CHUNK), np.uint8)              # linear index = z * CHUNK + x: the rows are the chunks
    for i in (0, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 77, CHUNK + 78):
        edge.reshape(-1)[i] = 1 + i % 3
    for conn in CONNS:
        ranks, table, count = check_rank(device, edge, conn, "class")
        assert count.cpu().tolist() == [6, 0]
        assert table[1:7, 0].cpu().tolist() == [0, 77, CHUNK - 1, CHUNK, CHUNK + 78, 2 * CHUNK - 1]


def check_rank_many_chunks(device):
    """More chunks than the scan workgroup has threads: its loop takes a second round, with a carry."""
    pred = cc.bernoulli(MANY_CHUNKS, 0.004, 3, 21)
    _, _, count = check_rank(device, pred, 26, "foreground", cap=4095)
    assert int(count.cpu()[0]) > 2 * SCAN_NT              # (so that roots lie in the chunks of the second round too)
    assert pred.reshape(-1)[SCAN_NT * CHUNK:].any()


def check_rank_shapes(device):
    """Widths that are no multiple of 4 or 64; Bernoulli maps at three densities, both connectivities, both modes."""
    for shape in ((17, 10, 67), (5, 7, 9)):
        seed = shape[0] * 31 + shape[2]
        for p in (0.05, 0.3, 0.6):
            check_rank_all_ways(device, cc.bernoulli(shape, p, 4, seed + int(p * 100)), cap=4095)
    check_rank_all_ways(device, cc.blob_and_specks((17, 10, 67))[0])


def check_rank_checkerboard_full_empty(device):
    cb = cc.checkerboard((9, 9, 65))
    n = int(cb.sum())
    _, _, count = check_rank(device, cb, 6, "class", cap=4095)          # every other voxel a component
    assert count.cpu().tolist() == [n, 0]
    _, table, count = check_rank(device, cb, 6, "foreground", cap=100)
    assert count.cpu().tolist() == [n, n - 100] and table.cpu()[101].tolist() == [-1, n - 100, 0, 0, 0, 9, 9, 65, -1]
    check_rank(device, cb, 26, "class")                                 # one component
    for shape in ((9, 9, 65), (5, 7, 9)):
        nvox = int(np.prod(shape))
        ranks, table, count = check_rank(device, np.full(shape, 2, np.uint8), 26, "class")
        assert bool((ranks == 1).all()) and count.cpu().tolist() == [1, 0]
        assert table.cpu()[:2].tolist() == [[-1, 0, 0, 0, 0, *shape, 0], [0, nvox, 0, 0, 0, *shape, 2]]
        ranks, table, count = check_rank(device, np.zeros(shape, np.uint8), 6, "foreground")
        assert not ranks.cpu().any() and not count.cpu().any()
        assert table.cpu()[0].tolist() == [-1, nvox, 0, 0, 0, *shape, 0] and not table.cpu()[1:].any()


def check_rank_cap(device):
    """cap = 3 with 2, 3, 4 and 40 components: the overflow row, count[1], and the volume's ranks unchanged by the cap."""
    from cfun_amd import lesions
    for n in (2, 3, 4, 40):
        pred = np.zeros((11, 9, 70), np.uint8)
        idx = np.random.default_rng(n).choice(6 * 5 * 23, n, replace=False)      # on a lattice two voxels clear in z and y,
        z, y, x = 2 * (idx // (5 * 23)), 2 * ((idx // 23) % 5), 3 * (idx % 23)   # three in x: isolated
        pred[z, y, x] = 1 + idx % 3
        pred[z[0], y[0], x[0] + 1] = pred[z[0], y[0], x[0]]                      # one of them two voxels large
        for conn in CONNS:
            ranks, table, count = check_rank(device, pred, conn, "class", cap=3)
            assert count.cpu().tolist() == [n, max(n - 3, 0)]
            full, _, _ = lesions.rank_components(_dev(pred, device), conn, "class", cap=4095)
            assert torch.equal(ranks, full) and int(ranks.max()) == n
            assert (table.cpu()[4, 0] == -1) == (n > 3)


# --------------------------------------------------------------------------------------------------------------- overlap
def check_overlap(device, a, b, cap_a, cap_b):
    from cfun_amd import lesions
    ta, tb = _dev(a.astype(np.int32), device), _dev(b.astype(np.int32), device)
    got = lesions.rank_overlap(ta, tb, cap_a, cap_b)
    want = lr.contingency(a, b, cap_a, cap_b)
    assert got.dtype == torch.int64 and tuple(got.shape) == (cap_a + 2, cap_b + 2) and got.device == ta.device
    assert int(got.sum()) == a.size, "the cells do not sum to D * H * W: %d vs %d" % (int(got.sum()), a.size)
    assert torch.equal(got.cpu(), torch.from_numpy(want)), "overlap: %s caps %d %d" % (a.shape, cap_a, cap_b)
    assert torch.equal(ta.cpu(), torch.from_numpy(a.astype(np.int32))) and torch.equal(tb.cpu(), torch.from_numpy(b.astype(np.int32)))
    return got


def check_overlap_shapes(device):
    """Identical, disjoint, one side empty, two random labelings; clamps at cap_a != cap_b on either side of the counts."""
    for shape in ((17, 10, 67), (5, 7, 9), (1, 1, STEP + 1), (3, 4, 3 * STEP // 12 + 5)):
        seed = shape[0] * 7 + shape[2]
        a, na = lr.rank(cc.bernoulli(shape, 0.3, 2, seed), 26, "foreground")
        b, nb = lr.rank(cc.bernoulli(shape, 0.2, 2, seed + 1), 6, "foreground")
        assert na >= 1 and nb >= 1
        check_overlap(device, a, b, max(na, 1), max(nb, 1))
        check_overlap(device, a, b, max(na // 2, 1), nb + 3)            # a clamped, b with rows to spare
        check_overlap(device, a, b, 1, 2)
        got = check_overlap(device, a, a, na + 1, na + 1)               # identical: a diagonal
        assert int(torch.diagonal(got).sum()) == a.size
        half = a.copy()
        half[..., : shape[2] // 2] = 0
        other = a - half                                                # disjoint supports
        got = check_overlap(device, half, other, na, na)
        assert not got.cpu()[1:, 1:].any()
        got = check_overlap(device, a, np.zeros_like(a), na, 5)         # one side empty: column 0 alone
        assert int(got[:, 0].sum()) == a.size
        check_overlap(device, np.zeros_like(a), np.zeros_like(a), 1, 1)


def check_overlap_many_workgroups(device):
    """Dense random rank volumes over many workgroups, the voxel count no multiple of a step: the spans' first voxels, the
    regrouping of the steps and the ragged last workgroup, cell for cell."""
    shape = (37, 61, 131)                                               # 295 667 voxels: 289 steps, 19 workgroups of 16 and a 20th of one
    n = int(np.prod(shape))
    assert n % STEP != 0 and n > 16 * STEP * MIN_STEPS and -(-n // STEP) % MIN_STEPS != 0
    rng = np.random.default_rng(12)
    a = rng.integers(0, 40, shape).astype(np.int32)
    b = rng.integers(0, 25, shape).astype(np.int32)
    a[rng.random(shape) < 0.5] = 0
    check_overlap(device, a, b, 39, 24)
    check_overlap(device, a, b, 10, 30)
    pos = np.arange(n, dtype=np.int32).reshape(shape)                   # a voxel's workgroup and step, readable off the table
    check_overlap(device, 1 + pos // (STEP * MIN_STEPS), 1 + (pos // STEP) % 7, 25, 7)
    tall = (2 * 16 * MIN_STEPS + 3, 1, STEP)                            # 515 steps of one row each: 33 workgroups, the last with three steps
    check_overlap(device, rng.integers(0, 9, tall).astype(np.int32), rng.integers(0, 3, tall).astype(np.int32), 8, 2)


def check_overlap_runs(device):
    """Every run one voxel long (two checkerboards a voxel apart), and one run that covers several loads of a wave."""
    shape = (9, 9, 65)
    a, na = lr.rank(cc.checkerboard(shape), 6, "foreground")
    shifted = (1 - cc.checkerboard(shape)).astype(np.uint8)             # the same board one voxel along
    b, nb = lr.rank(shifted, 6, "foreground")
    assert na > 2000 and nb > 2000 and not (a.astype(bool) & b.astype(bool)).any()
    check_overlap(device, a, b, 300, 200)
    check_overlap(device, a, (a % 5 + 1).astype(np.int32), 300, 5)      # every run one voxel long AND every voxel a pair
    small, ns = lr.rank(cc.checkerboard((5, 7, 9)), 6, "foreground")
    check_overlap(device, small, small, ns, ns)
    wide_a, wide_b = np.zeros((3, 2, 5 * 64 + 7), np.int32), np.zeros((3, 2, 5 * 64 + 7), np.int32)
    wide_a[1, 0, :], wide_b[1, 0, :] = 3, 2                             # one pair across the whole width
    wide_a[2, 1, 10:200], wide_b[2, 1, 100:327] = 1, 4
    got = check_overlap(device, wide_a, wide_b, 4, 4)
    assert int(got[3, 2]) == 5 * 64 + 7 and int(got[1, 4]) == 100


def check_overlap_table_full(device):
    """More distinct pairs in ONE workgroup than its LDS table has slots: the rest goes to global memory directly."""
    n = 2 * PAIR_SLOTS + 100
    assert n <= STEP * MIN_STEPS, "test setup: this volume is no longer one workgroup's"
    i = np.arange(n)
    a = (1 + i % (PAIR_SLOTS + 500)).astype(np.int32).reshape(1, 1, n)
    b = (1 + i % 3).astype(np.int32).reshape(1, 1, n)
    assert len(set(zip(a.reshape(-1).tolist(), b.reshape(-1).tolist()))) > PAIR_SLOTS
    check_overlap(device, a, b, 4095, 3)
    check_overlap(device, a, b, PAIR_SLOTS + 100, 2)                    # and with both sides clamped


# --------------------------------------------------------------------------------------------------------------- entries
def _canary(shape, dtype, device, value):
    """A tensor with 64 canary elements either side of it in one allocation."""
    n = int(np.prod(shape))
    buf = torch.full((n + 128,), value, dtype=dtype, device=device)
    return buf, buf[64:64 + n].view(shape)


def check_entries(device):
    """Every refusal of the C entries with canaries either side of each output; zero-sized volumes; a workspace one byte short."""
    from cfun_amd import _lib, lesions
    lib = _lib.load()
    dims, cap = (3, 5, 70), 7
    pred_np = cc.bernoulli(dims, 0.3, 3, 5)
    pred = _dev(pred_np, device)
    from cfun_amd import components
    labels = components.label_components(pred, 26, "class")
    ranks_buf, ranks = _canary(dims, torch.int32, device, -7)
    count_buf, count = _canary((2,), torch.int64, device, -7)
    table_buf, table = _canary((cap + 2, 9), torch.int64, device, -7)
    over_buf, over = _canary((cap + 2, cap + 3), torch.int64, device, -7)
    ws = _lib.workspace(lib.cfun_lesion_workspace_bytes(*dims, cap), pred)
    assert lib.cfun_lesion_workspace_bytes(*dims, cap) == 4 * -(-pred_np.size // CHUNK)
    i32 = C.c_int32 * 3
    p, st = _lib.ptr, _lib.stream(pred)

    def rank(d=dims, c=cap, nbytes=None):
        return lib.cfun_cc_rank(p(pred), p(labels), i32(*d), c, p(ranks), p(count), p(table), p(ws),
                                ws.numel() if nbytes is None else nbytes, st)

    def overlap(d=dims, ca=cap, cb=cap + 1):
        return lib.cfun_rank_overlap(p(labels), p(labels), i32(*d), ca, cb, p(over), p(ws), ws.numel(), st)

    bad_dims = ((2048, 1024, 1024), (1, 1 << 16, 1 << 15), (1, 1, (1 << 31) - 1), (1 << 30, 1 << 30, 1 << 30), (2, -3, 4), (-1, 0, 4))
    for d in bad_dims:
        assert rank(d=d) == -1 and overlap(d=d) == -1, d
        assert lib.cfun_lesion_workspace_bytes(*d, cap) == 0
    for c in (0, -1, 4096, 1 << 20):
        assert rank(c=c) == -1 and overlap(ca=c) == -1 and overlap(cb=c) == -1, c
        assert lib.cfun_lesion_workspace_bytes(*dims, c) == 0
    assert rank(nbytes=lib.cfun_lesion_workspace_bytes(*dims, cap) - 1) == -2      # (outside guard mode ws has a floor of 256)
    for buf in (ranks_buf, count_buf, table_buf, over_buf):
        assert bool((buf.cpu() == -7).all()), "a refused call wrote to an output"
    assert lib.cfun_lesion_workspace_bytes(1, 1, (1 << 31) - 2, 4095) == 4 * -(-((1 << 31) - 2) // CHUNK)
    # the calls that are accepted: the outputs are fully written, the canaries stay
    assert rank() == 0 and overlap() == 0
    want_ranks, n = lr.rank(pred_np, 26, "class")
    want_count, want_table = lr.table(pred_np, want_ranks, n, cap)
    assert n > cap, "test setup: the overflow row stays empty"
    assert torch.equal(ranks.cpu(), torch.from_numpy(want_ranks)) and torch.equal(count.cpu(), torch.from_numpy(want_count))
    assert torch.equal(table.cpu(), torch.from_numpy(want_table))
    lab_np = labels.cpu().numpy()
    assert torch.equal(over.cpu(), torch.from_numpy(lr.contingency(lab_np, lab_np, cap, cap + 1)))
    for buf, t in ((ranks_buf, ranks), (count_buf, count), (table_buf, table), (over_buf, over)):
        flat = buf.cpu()
        assert bool((flat[:64] == -7).all()) and bool((flat[64 + t.numel():] == -7).all()), "a canary beside an output changed"
    # zero-sized volumes: count, table and overlap all zeros, nothing launched
    for d in ((0, 5, 7), (5, 0, 7), (5, 7, 0)):
        assert lib.cfun_lesion_workspace_bytes(*d, cap) == 0
        count.fill_(-7), table.fill_(-7), over.fill_(-7)
        assert rank(d=d) == 0 and overlap(d=d) == 0
        assert not count.cpu().any() and not table.cpu().any() and not over.cpu().any()
        empty = torch.zeros(d, dtype=torch.uint8, device=device)
        r, t, c = lesions.rank_components(empty, cap=5)
        assert tuple(r.shape) == d and r.dtype == torch.int32 and not t.cpu().any() and not c.cpu().any()
        o = lesions.rank_overlap(r, r, 2, 3)
        assert tuple(o.shape) == (4, 5) and not o.cpu().any()
        s = lesions.LesionScores(lesions.lesion_scores(empty, empty, 2, cap=5))
        assert (s.n_ref, s.n_pred, s.truncated) == (0, 0, False) and np.isnan(s.recall).all()


def check_repeatable(device, shape=(17, 10, 67)):
    """Every kernel twice: the same bits."""
    from cfun_amd import lesions
    t = _dev(cc.bernoulli(shape, 0.3, 4, 77), device)
    u = _dev(cc.bernoulli(shape, 0.25, 4, 78), device)
    for conn in CONNS:
        first, second = lesions.rank_components(t, conn, "class", 50), lesions.rank_components(t, conn, "class", 50)
        for x, y in zip(first, second):
            assert torch.equal(x, y)
        other = lesions.rank_components(u, conn, "foreground", 50)[0]
        assert torch.equal(lesions.rank_overlap(first[0], other, 50, 60), lesions.rank_overlap(first[0], other, 50, 60))
    a, b = lesions.lesion_scores(t, u, (1, 2)), lesions.lesion_scores(t, u, (1, 2))
    assert torch.equal(a.packed, b.packed)


def check_wrapper_preconditions(device):
    from cfun_amd import _lib, lesions
    pred = torch.zeros((4, 5, 6), dtype=torch.uint8, device=device)
    ranks = torch.zeros((4, 5, 6), dtype=torch.int32, device=device)
    for fn in (lesions.rank_components, lambda t, *a, **kw: lesions.lesion_scores(t, pred, 2, *a, **kw)):
        with pytest.raises(ValueError, match="uint8"):
            fn(pred.to(torch.int32))
        with pytest.raises(ValueError, match=r"\[D,H,W\]"):
            fn(pred[0])
        with pytest.raises(ValueError, match="connectivity"):
            fn(pred, 18)
    with pytest.raises(ValueError, match="by must be"):
        lesions.rank_components(pred, 26, "organ")
    huge = torch.zeros(1, dtype=torch.uint8, device=device).expand(2048, 1024, 1024)          # a view: nothing is allocated
    with pytest.raises(ValueError, match=r"2\^31"):
        lesions.rank_components(huge)
    with pytest.raises(RuntimeError, match="contiguous"):
        lesions.rank_components(pred.permute(2, 1, 0).contiguous().permute(2, 1, 0))
    for cap in (0, 4096, -3):
        with pytest.raises(ValueError, match="cap"):
            lesions.rank_components(pred, cap=cap)
        with pytest.raises(ValueError, match="cap_a"):
            lesions.rank_overlap(ranks, ranks, cap_a=cap)
        with pytest.raises(ValueError, match="cap_b"):
            lesions.rank_overlap(ranks, ranks, cap_b=cap)
        with pytest.raises(ValueError, match="cap"):
            lesions.lesion_scores(pred, pred, 2, cap=cap)
    with pytest.raises(ValueError, match="int32"):
        lesions.rank_overlap(ranks.to(torch.int64), ranks)
    with pytest.raises(ValueError, match="differ in shape"):
        lesions.rank_overlap(ranks, ranks[:, :, :5].contiguous())
    with pytest.raises(ValueError, match="differ in shape"):
        lesions.lesion_scores(pred, pred[:, :, :5], 2)
    for cls in (0, 256, (), (1, 0)):
        with pytest.raises(ValueError, match="cls"):
            lesions.lesion_scores(pred, pred, cls)
    for ts in ((), (1.0,), (-0.1,)):
        with pytest.raises(ValueError, match="thresholds"):
            lesions.lesion_scores(pred, pred, 2, thresholds=ts)
    if not _lib.is_emulator():
        with pytest.raises(RuntimeError, match="CPU tensor"):
            lesions.rank_components(pred.cpu())


# ------------------------------------------------------------------------------------------------------------ end to end
PLANTED_SHAPE = (24, 48, 72)
# twelve reference lesions of 1 .. 400 voxels, one per 12^3 cell, each one voxel inside its cell
PLANTED_SIZES = [(1, 1, 1), (1, 1, 3), (2, 2, 2), (2, 3, 4), (3, 3, 5), (3, 4, 6), (4, 4, 7), (4, 5, 8), (5, 5, 8), (5, 6, 8),
                 (5, 8, 8), (5, 8, 10)]


def planted():
    """A box liver (1) with twelve lesions (2) in the label.  In the prediction lesions 0 and 3 are missed, 5, 6 and 7 are split
    in two by a missing plane, 8 and 9 -- neighbours along x -- are bridged into one, 1 and 2 are exact, 4, 10 and 11 are a
    voxel off along x, and thirty one-voxel specks sit in cells of their own.  -> (pred, label) as uint8 [D,H,W]."""
    label = np.zeros(PLANTED_SHAPE, np.uint8)
    label[1:23, 1:47, 1:71] = 1
    pred = label.copy()
    cells = [(cz, cy, cx) for cz in range(2) for cy in range(4) for cx in range(6)]
    for i, (dz, dy, dx) in enumerate(PLANTED_SIZES):
        z, y, x = [12 * c + 1 for c in cells[i]]
        label[z:z + dz, y:y + dy, x:x + dx] = 2
        if i in (0, 3):
            continue
        if i in (4, 10, 11):
            pred[z:z + dz, y:y + dy, x + 1:x + dx + 1] = 2
        else:
            pred[z:z + dz, y:y + dy, x:x + dx] = 2
        if i in (5, 6, 7):
            pred[z:z + dz, y:y + dy, x + dx // 2] = 1
    z, y, x = [12 * c + 1 for c in cells[8]]
    pred[z, y, x:x + 12 + 8] = 2                                         # the bridge from lesion 8 into lesion 9
    for i in range(30):
        z, y, x = [12 * c + 6 for c in cells[12 + i]]
        pred[z, y, x] = 2
    return pred, label


def _same_scores(s, want):
    assert (s.n_ref, s.n_pred) == (want["n_ref"], want["n_pred"]) and s.groups == want["groups"]
    assert np.array_equal(s.sizes_ref, want["sizes_ref"]) and np.array_equal(s.sizes_pred, want["sizes_pred"])
    for key in ("group_dice", "group_iou", "recall", "precision", "f1"):
        np.testing.assert_array_equal(getattr(s, key), want[key], err_msg=key)


def check_planted(device):
    from cfun_amd import lesions
    pred, label = planted()
    assert sorted(int(np.prod(s)) for s in PLANTED_SIZES)[::11] == [1, 400]
    thresholds = (0.0, 0.5, 0.8)
    for conn in CONNS:
        want = lr.scores(pred, label, 2, conn, thresholds)
        # the planted facts, on the host restatement: 12 lesions; 5 whole + 3 x 2 pieces + 1 bridge + 30 specks predicted
        assert (want["n_ref"], want["n_pred"]) == (12, 42) and len(want["groups"]) == 9 + 2 + 30
        assert sum(1 for g, p in want["groups"] if not p) == 2 and sum(1 for g, p in want["groups"] if not g) == 30
        assert sum(1 for g, p in want["groups"] if len(p) == 2) == 3 and sum(1 for g, p in want["groups"] if len(g) == 2) == 1
        assert want["recall"][0] == 10 / 12 and want["precision"][0] == 12 / 42
        # the label as the loader holds it: [H,W,D] int32, read through a permuted view
        label_hwd = _dev(np.ascontiguousarray(label.transpose(1, 2, 0)).astype(np.int32), device)
        buffers = lesions.lesion_scores(_dev(pred, device), label_hwd.permute(2, 0, 1), 2, conn, thresholds)
        assert buffers.packed.dtype == torch.int64 and buffers.packed.device == label_hwd.device
        s = lesions.LesionScores(buffers)
        assert not s.truncated and s.thresholds == thresholds
        _same_scores(s, want)
        assert int(s.overlap.sum()) == pred.size
        # a float label is truncated towards zero, as the other scores of run_test read it
        frac = label.astype(np.float32) + np.float32(0.7)
        _same_scores(lesions.LesionScores(lesions.lesion_scores(_dev(pred, device), _dev(frac, device), 2, conn, thresholds)), want)
        # a float label and a tuple of ids: the liver and the lesions together are one component on either side
        s = lesions.LesionScores(lesions.lesion_scores(_dev(pred, device), _dev(label.astype(np.float32), device), (1, 2), conn))
        _same_scores(s, lr.scores(pred, label, (1, 2), conn))
        assert (s.n_ref, s.n_pred) == (1, 1)
        # a cap below the count: the rates are nan, not wrong
        s = lesions.LesionScores(lesions.lesion_scores(_dev(pred, device), _dev(label, device), 2, conn, thresholds, cap=20))
        assert s.truncated and (s.n_ref, s.n_pred) == (12, 42) and s.groups == [] and s.group_dice.size == 0
        assert np.isnan(s.recall).all() and np.isnan(s.precision).all() and np.isnan(s.f1).all()
        assert np.array_equal(s.sizes_ref, want["sizes_ref"]) and np.array_equal(s.sizes_pred, want["sizes_pred"][:20])
        s = lesions.LesionScores(lesions.lesion_scores(_dev(pred, device), _dev(label, device), 2, conn, thresholds, cap=42))
        assert not s.truncated
        _same_scores(s, want)


def check_nan_rates(device):
    """No reference lesion: recall and F1 are nan, precision is 0; nothing on either side: everything is nan."""
    from cfun_amd import lesions
    pred, label = planted()
    liver = np.minimum(label, 1)
    s = lesions.LesionScores(lesions.lesion_scores(_dev(pred, device), _dev(liver, device), 2))
    _same_scores(s, lr.scores(pred, liver, 2))
    assert s.n_ref == 0 and np.isnan(s.recall).all() and np.isnan(s.f1).all() and s.precision.tolist() == [0.0, 0.0]
    s = lesions.LesionScores(lesions.lesion_scores(_dev(liver, device), _dev(label, device), 2))
    assert s.n_pred == 0 and np.isnan(s.precision).all() and np.isnan(s.f1).all() and s.recall.tolist() == [0.0, 0.0]
    s = lesions.LesionScores(lesions.lesion_scores(_dev(liver, device), _dev(liver, device), 2))
    assert np.isnan(s.recall).all() and np.isnan(s.precision).all() and np.isnan(s.f1).all() and not s.truncated


def _same_summary(a, b):
    """Two run_test dicts, key for key (detect_time is a wall-clock figure: present in both, not compared)."""
    assert set(a) == set(b)
    for key in set(a) - {"results", "saved", "detect_time"}:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert len(a["results"]) == len(b["results"])
    for ra, rb in zip(a["results"], b["results"]):
        assert set(ra) == set(rb)
        for key in ra:
            if torch.is_tensor(ra[key]):
                assert torch.equal(ra[key], rb[key]), key
            else:
                np.testing.assert_array_equal(ra[key], rb[key], err_msg=key)
    assert [os.path.basename(p) for p in a["saved"]] == [os.path.basename(p) for p in b["saved"]]


def check_run_test_lits(device, tmp_path):
    import module_cases as mc
    from cfun_amd import components, evaluate, lesions
    cfg = mc.tiny_lits_config("together", max_dim=64, min_dim=32)
    cfg.PAD_IMAGE_SHAPE = [80, 80, 40]
    k = int(cfg.NUM_CLASSES)
    net = ec._net(device, cfg, 2)
    rng = np.random.default_rng(9)
    image = rng.normal(0.0, 200.0, ec.SRC).astype(np.float32)
    label = np.zeros(ec.SRC, np.int32)
    label[5:30, 10:44, 2:15] = rng.integers(0, k, (25, 34, 13))
    cases = [(image, label, ec.AFFINE, "liver_7.nii.gz", (44, 52, 22))]
    plain = evaluate.run_test(net, cases)
    _same_summary(plain, evaluate.run_test(net, cases, lesions=None))
    assert not plain["results"][0]["empty"], "test setup: no detection"
    assert not any(key.startswith("lesion") or key == "tumour_burden" for key in plain)

    def check(r, opts, scored):
        want = lr.scores(scored, label.transpose(2, 0, 1), opts.get("cls", 2), opts.get("connectivity", 26),
                         opts.get("thresholds", (0.0, 0.5)))
        nt = len(opts.get("thresholds", (0.0, 0.5)))
        for key in ("recall", "precision", "f1"):
            assert r["lesion_" + key].shape == (1, nt)
            np.testing.assert_array_equal(r["lesion_" + key][0], want[key], err_msg=key)
        assert r["lesion_counts"].tolist() == [[want["n_ref"], want["n_pred"]]] and r["lesion_counts"].dtype == np.int64
        ids = opts.get("cls", 2)
        ids = ids if isinstance(ids, tuple) else (ids,)
        burden = [np.isin(v, ids).sum() / float((v > 0).sum()) for v in (label, scored)]
        np.testing.assert_array_equal(r["tumour_burden"], [burden])
        s = r["results"][0]["lesion_scores"]
        assert isinstance(s, lesions.LesionScores) and not s.truncated
        _same_scores(s, want)
        if scored is raw:
            for key in ("per_class_ious", "mask_ious", "dice"):            # the other scores are what they were
                np.testing.assert_array_equal(r[key], plain[key])

    raw = plain["results"][0]["mask_device"].cpu().numpy()
    assert (raw == 2).any() and (label == 2).any(), "test setup: no tumour voxel"
    check(evaluate.run_test(net, cases, lesions=2), {}, raw)
    # the dict form; and with a postprocess it is the cleaned map that is scored
    opts = {"cls": (1, 2), "thresholds": (0.0, 0.25, 0.5), "connectivity": 6, "cap": 4095}
    pp = components.Postprocess(connectivity=26, by="class", largest_only=False, min_voxels=3)
    r = evaluate.run_test(net, cases, postprocess=pp, lesions=opts)
    cleaned = r["results"][0]["mask_device"].cpu().numpy()
    assert np.array_equal(r["results"][0]["mask_device_raw"].cpu().numpy(), raw)
    assert not np.array_equal(cleaned, raw), "test setup: the cleaning removed nothing"
    check(r, opts, cleaned)
    for bad in (0, k, (1, k), {"thresholds": (0.5,)}, {"cls": 2, "min_voxels": 3}):
        with pytest.raises(ValueError):
            evaluate.run_test(net, cases, lesions=bad)
    # the detector-only stage skips it as it skips the mask scores
    cfg.STAGE = "beginning"
    assert net.detector_phase_only
    r = evaluate.run_test(net, cases, lesions=2)
    assert r["lesion_recall"].shape == (0, 2) and r["lesion_counts"].shape == (0, 2) and r["tumour_burden"].shape == (0, 2)
    assert "lesion_scores" not in r["results"][0]


# ------------------------------------------------------------------------------------------------------------ accounting
def lesion_header_symbols():
    """The same parse as test_abi.header_symbols, on include/cfun_lesion.h."""
    txt = open(os.path.join(ROOT, "include", "cfun_lesion.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(cfun_[a-z0-9_]+)\s*\(", txt)))


LESION_NO_LAUNCH = {"cfun_lesion_workspace_bytes": "host-side query: launches nothing, touches no device memory"}


def check_coverage(tier):
    from cfun_amd import _lib
    assert lesion_header_symbols() == sorted(_lib.LESION_EXPORTS)
    for other in (_lib.EXPORTS, _lib.SAMPLE_EXPORTS, _lib.TILE_EXPORTS, _lib.EVAL_EXPORTS, _lib.CC_EXPORTS, _lib.SURFACE_EXPORTS):
        assert not set(_lib.LESION_EXPORTS) & set(other)
    missed = sorted(set(_lib.LESION_EXPORTS) - set(LESION_NO_LAUNCH) - guard.SEEN[tier])
    assert not missed, "lesion entries that launch work but never ran under guard: %s" % missed
