"""The numpy restatement of include/cfun_surface.h: the surface by the erosion formula, the squared distance field by brute
force in float32 exactly as the header defines it (every candidate of every line, no pruning), and the per-class statistics
in float64 from that field.  tests/test_surface_ref.py holds this file against scipy's exact EDT and answers written by hand."""
import numpy as np
from scipy import ndimage

FIELDS = ("n_pred", "n_label", "sum_pl", "sum_lp", "sumsq_pl", "sumsq_lp", "max_sq_pl", "max_sq_lp", "q_lo_sq", "q_hi_sq", "frac")
_CHUNK = 1 << 24          # elements of one brute-force temporary (64 MB of float32)


def surface(m, cls):
    """S_cls(m): mask & ~erosion(mask) with the 6-neighbourhood and everything outside the volume counted as not-mask."""
    mask = np.asarray(m) == cls
    if mask.size == 0:
        return mask
    return mask & ~ndimage.binary_erosion(mask, ndimage.generate_binary_structure(3, 1), border_value=0)


def spacing2(spacing):
    """(sz, sy, sx) -> the three float32 squares: float32(double(s) * double(s))."""
    return tuple(np.float32(np.float64(s) * np.float64(s)) for s in spacing)


def _sweep(g, axis, a2):
    """out[.., i, ..] = min over j of fl(g[.., j, ..] + fl(float(k * k) * a2)), k = i - j, along ``axis``; all float32."""
    g = np.moveaxis(g, axis, -1)
    n = g.shape[-1]
    k = np.arange(n, dtype=np.int64)
    kk = ((k[:, None] - k[None, :]) ** 2).astype(np.float32)          # exact: n <= 4096
    t = kk * np.float32(a2)                                           # one float32 rounding
    assert t.dtype == np.float32
    flat = np.ascontiguousarray(g).reshape(-1, n)
    out = np.empty_like(flat)
    rows = max(1, _CHUNK // (n * n))
    for r in range(0, flat.shape[0], rows):
        out[r:r + rows] = (flat[r:r + rows, None, :] + t[None]).min(axis=2)      # float32 + float32: one rounding
    return np.moveaxis(out.reshape(g.shape), -1, axis)


def field(surf, spacing):
    """The float32 squared distance field of a boolean surface; +inf everywhere when it is empty."""
    sz2, sy2, sx2 = spacing2(spacing)
    g = np.where(surf, np.float32(0), np.float32(np.inf)).astype(np.float32)
    if g.size == 0:
        return g
    with np.errstate(over="ignore"):
        g = _sweep(g, 2, sx2)          # fl(0 + t) = t: the x sweep of the definition
        g = _sweep(g, 1, sy2)
        g = _sweep(g, 0, sz2)
    return g


def rank_rule(n, qf):
    """(lo, hi, frac) of the header's percentile rule."""
    pos = np.float64(n - 1) * np.float64(qf)
    lo = int(np.floor(pos))
    return lo, min(lo + 1, n - 1), float(pos - np.float64(lo))


def class_stats(pred, label, cls, spacing, q=95.0, fields=None):
    """One CfunSurfaceStats row as a dict, plus ``d2_pl`` / ``d2_lp`` (the float32 directed sets) and, when both surfaces are
    non-empty, ``np_percentile``: numpy's own percentile of the concatenated distances."""
    a, b = surface(pred, cls), surface(label, cls)
    fa, fb = fields if fields is not None else (field(a, spacing), field(b, spacing))
    d2_pl, d2_lp = fb[a], fa[b]
    r = dict.fromkeys(FIELDS, 0.0)
    r["n_pred"], r["n_label"] = int(a.sum()), int(b.sum())
    r["d2_pl"], r["d2_lp"] = d2_pl, d2_lp
    if r["n_pred"] == 0 or r["n_label"] == 0:
        return r
    p64, l64 = d2_pl.astype(np.float64), d2_lp.astype(np.float64)
    r["sum_pl"], r["sum_lp"] = float(np.sqrt(p64).sum()), float(np.sqrt(l64).sum())
    r["sumsq_pl"], r["sumsq_lp"] = float(p64.sum()), float(l64.sum())
    r["max_sq_pl"], r["max_sq_lp"] = float(d2_pl.max()), float(d2_lp.max())
    both = np.sort(np.concatenate([d2_pl, d2_lp]))
    lo, hi, frac = rank_rule(both.size, np.float64(q) / 100.0)
    r["q_lo_sq"], r["q_hi_sq"], r["frac"] = float(both[lo]), float(both[hi]), frac
    r["np_percentile"] = float(np.percentile(np.sqrt(both.astype(np.float64)), q))
    return r


def stats(pred, label, k, spacing, q=95.0):
    """Rows 0 .. k-1 (row 0 all zeros), as class_stats dicts."""
    zero = dict.fromkeys(FIELDS, 0.0)
    zero["n_pred"] = zero["n_label"] = 0
    return [zero] + [class_stats(pred, label, c, spacing, q) for c in range(1, k)]


def scores(row):
    """The scores of evaluate.SurfaceScores from one row, in float64; nan for a class empty on either side."""
    names = ("hausdorff", "hd_percentile", "asd_pred_to_label", "asd_label_to_pred", "assd", "assd_pooled", "rmsd")
    if row["n_pred"] == 0 or row["n_label"] == 0:
        return dict.fromkeys(names, float("nan"))
    n1, n2 = float(row["n_pred"]), float(row["n_label"])
    apl, alp = row["sum_pl"] / n1, row["sum_lp"] / n2
    return dict(hausdorff=float(np.sqrt(max(row["max_sq_pl"], row["max_sq_lp"]))),
                hd_percentile=float((1.0 - row["frac"]) * np.sqrt(row["q_lo_sq"]) + row["frac"] * np.sqrt(row["q_hi_sq"])),
                asd_pred_to_label=apl, asd_label_to_pred=alp, assd=0.5 * (apl + alp),
                assd_pooled=(row["sum_pl"] + row["sum_lp"]) / (n1 + n2),
                rmsd=float(np.sqrt((row["sumsq_pl"] + row["sumsq_lp"]) / (n1 + n2))))
