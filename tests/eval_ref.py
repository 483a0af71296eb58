"""Numpy restatement of the scoring path (cfun_amd/evaluate.py, cfun_amd/csrc/eval.hip): the confusion counts by np.add.at and the
three scores from them.  Plain and slow on purpose; the device is compared against this, and this against the reference's own
compute_per_class_mask_iou / compute_mask_iou through tests/golden/eval_iou.npz."""
import numpy as np


def confusion(pred, label, k):
    """pred, label: integer arrays of one shape (any layout) -> int64 [(k+1),(k+1)], counts[g][p]; values outside [0, k) count in
    row / column k."""
    g = np.asarray(label).astype(np.int64).reshape(-1)
    p = np.asarray(pred).astype(np.int64).reshape(-1)
    assert g.shape == p.shape
    g = np.where((g >= 0) & (g < k), g, k)
    p = np.where((p >= 0) & (p < k), p, k)
    counts = np.zeros((k + 1, k + 1), np.int64)
    np.add.at(counts, (g, p), 1)
    return counts


def per_class_iou(counts):
    k = counts.shape[0] - 1
    out = np.zeros(k - 1, np.float64)
    for j in range(1, k):
        inter = float(counts[j, j])
        out[j - 1] = inter / (float(counts[j, :].sum()) + float(counts[:, j].sum()) - inter + 1e-6)
    return out


def dice(counts):
    k = counts.shape[0] - 1
    out = np.zeros(k - 1, np.float64)
    for j in range(1, k):
        out[j - 1] = 2.0 * float(counts[j, j]) / (float(counts[j, :].sum()) + float(counts[:, j].sum()) + 1e-6)
    return out


def mask_iou(counts):
    """label > 0 against pred > 0 ("other" is foreground)."""
    a1, a2 = float(counts[1:, :].sum()), float(counts[:, 1:].sum())
    inter = float(counts[1:, 1:].sum())
    return inter / (a1 + a2 - inter + 1e-6)
