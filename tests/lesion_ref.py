"""Host restatement of the lesion-scoring path (cfun_amd/lesions.py, cfun_amd/csrc/lesion.hip): scipy.ndimage.label and
find_objects for the ranks and the component table, a numpy contingency count for the overlap, and the matching rule written
independently of lesions.py (a breadth-first search over the overlap graph, no union-find).  Plain and slow on purpose; the device
is compared against this with torch.equal / np.array_equal, and this against hand-written answers in tests/test_lesion_ref.py.
The reference project has no such function: this file and those answers are the pin."""
import numpy as np
from scipy import ndimage

import cc_ref as cr

FIELDS = 9


def rank(pred, connectivity=26, by="class"):
    """-> (ranks int32 [D,H,W], n).  by="foreground": scipy.ndimage.label's array AS IT IS.  by="class": one scipy labelling per
    byte value (cc_ref.label), the components numbered in the order of their first voxel."""
    pred = np.asarray(pred)
    if pred.size == 0:
        return np.zeros(pred.shape, np.int32), 0
    if by == "foreground":
        lab, n = ndimage.label(pred > 0, structure=cr._structure(connectivity))
        return lab.astype(np.int32), int(n)
    canon = cr.label(pred, connectivity, "class").astype(np.int64)
    roots = np.unique(canon[canon > 0])
    out = np.zeros(pred.shape, np.int64)
    out[canon > 0] = np.searchsorted(roots, canon[canon > 0]) + 1
    return out.astype(np.int32), int(roots.size)


def table(pred, ranks, n, cap):
    """-> (count int64 [2], table int64 [cap + 2, 9]) from find_objects and bincount."""
    pred, ranks = np.asarray(pred), np.asarray(ranks)
    t = np.zeros((cap + 2, FIELDS), np.int64)
    count = np.array([n, max(n - cap, 0)], np.int64)
    if pred.size == 0:
        return count, t
    sizes = np.bincount(ranks.reshape(-1), minlength=n + 1)
    d, h, w = pred.shape
    t[0] = (-1, sizes[0], 0, 0, 0, d, h, w, 0)
    boxes = ndimage.find_objects(ranks)
    flat_r, flat_p = ranks.reshape(-1), pred.reshape(-1)
    first = np.full(n + 1, flat_r.size, np.int64)
    np.minimum.at(first, flat_r, np.arange(flat_r.size))
    for r in range(1, min(n, cap) + 1):
        b = boxes[r - 1]
        t[r] = (first[r], sizes[r], b[0].start, b[1].start, b[2].start, b[0].stop, b[1].stop, b[2].stop, flat_p[first[r]])
    if n > cap:
        rest = boxes[cap:]
        t[cap + 1] = (-1, sizes[cap + 1:].sum(), min(b[0].start for b in rest), min(b[1].start for b in rest),
                      min(b[2].start for b in rest), max(b[0].stop for b in rest), max(b[1].stop for b in rest),
                      max(b[2].stop for b in rest), -1)
    return count, t


def contingency(a, b, cap_a, cap_b):
    """int64 [cap_a + 2, cap_b + 2]: voxels per (min(a, cap_a + 1), min(b, cap_b + 1))."""
    ia = np.minimum(np.asarray(a, np.int64).reshape(-1), cap_a + 1)
    ib = np.minimum(np.asarray(b, np.int64).reshape(-1), cap_b + 1)
    flat = np.bincount(ia * (cap_b + 2) + ib, minlength=(cap_a + 2) * (cap_b + 2))
    return flat.reshape(cap_a + 2, cap_b + 2).astype(np.int64)


def match(sizes_ref, sizes_pred, overlap, thresholds=(0.0, 0.5)):
    """The matching rule on plain arrays.  sizes_ref [G], sizes_pred [P], overlap [G, P] (shared voxels).  Lesions g and p are
    linked when overlap[g, p] > 0; the connected groups of that graph are the correspondences.  Per group, with A, B, I the
    reference, predicted and shared voxels: iou = I / (A + B - I), dice = 2 I / (A + B).  At threshold t the lesions of a group
    with both sides and iou > t are matched.  -> dict(groups, group_dice, group_iou, recall, precision, f1, n_ref, n_pred);
    groups in the order of their first member, reference lesions before predicted ones; a rate with a zero denominator is nan."""
    sizes_ref, sizes_pred = np.asarray(sizes_ref, np.int64), np.asarray(sizes_pred, np.int64)
    g_n, p_n = sizes_ref.size, sizes_pred.size
    ov = np.asarray(overlap, np.int64).reshape(g_n, p_n)
    seen_g, seen_p = [False] * g_n, [False] * p_n
    groups = []
    for start in [("g", i) for i in range(g_n)] + [("p", j) for j in range(p_n)]:
        if (seen_g if start[0] == "g" else seen_p)[start[1]]:
            continue
        (seen_g if start[0] == "g" else seen_p)[start[1]] = True
        queue, ref, prd = [start], [], []
        while queue:
            side, i = queue.pop(0)
            (ref if side == "g" else prd).append(i)
            near = np.nonzero(ov[i, :] if side == "g" else ov[:, i])[0].tolist()
            other_seen, other = (seen_p, "p") if side == "g" else (seen_g, "g")
            for j in near:
                if not other_seen[j]:
                    other_seen[j] = True
                    queue.append((other, j))
        groups.append((sorted(ref), sorted(prd)))
    dice, iou = [], []
    for ref, prd in groups:
        a, b = int(sizes_ref[ref].sum()), int(sizes_pred[prd].sum())
        i = int(sum(ov[g, p] for g in ref for p in prd))
        dice.append(2.0 * i / (a + b))
        iou.append(i / (a + b - i))
    recall, precision, f1 = [], [], []
    for t in thresholds:
        hit = [k for k, (ref, prd) in enumerate(groups) if ref and prd and iou[k] > t]
        mr, mp = sum(len(groups[k][0]) for k in hit), sum(len(groups[k][1]) for k in hit)
        r = mr / g_n if g_n else float("nan")
        p = mp / p_n if p_n else float("nan")
        recall.append(r)
        precision.append(p)
        f1.append(2.0 * p * r / (p + r) if p + r > 0 else float("nan"))      # (nan + x > 0 is False: nan stays nan)
    return dict(groups=[([g + 1 for g in ref], [p + 1 for p in prd]) for ref, prd in groups],
                group_dice=np.array(dice, np.float64), group_iou=np.array(iou, np.float64), recall=np.array(recall, np.float64),
                precision=np.array(precision, np.float64), f1=np.array(f1, np.float64), n_ref=g_n, n_pred=p_n)


def scores(pred, label, cls, connectivity=26, thresholds=(0.0, 0.5)):
    """pred, label: integer [D,H,W] arrays; cls: an id or a tuple of ids.  The whole route on the host, without any cap."""
    ids = tuple(cls) if isinstance(cls, (tuple, list)) else (cls,)
    lp, lg = np.isin(np.asarray(pred), ids).astype(np.uint8), np.isin(np.asarray(label), ids).astype(np.uint8)
    rg, ng = rank(lg, connectivity, "foreground")
    rp, npr = rank(lp, connectivity, "foreground")
    full = contingency(rg, rp, max(ng, 1), max(npr, 1))
    out = match(np.bincount(rg.reshape(-1), minlength=ng + 1)[1:], np.bincount(rp.reshape(-1), minlength=npr + 1)[1:],
                full[1:ng + 1, 1:npr + 1], thresholds)
    out["sizes_ref"] = np.bincount(rg.reshape(-1), minlength=ng + 1)[1:].astype(np.int64)
    out["sizes_pred"] = np.bincount(rp.reshape(-1), minlength=npr + 1)[1:].astype(np.int64)
    return out
