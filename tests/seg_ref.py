"""CPU restatement of the segmentation scoring: the confusion table ``umhs_seg_confusion`` (csrc/umhs_seg.hip) accumulates, by
``torch.bincount``, and the scores ``umhsnerf.utils.seg_metrics`` derives from it, in float64 numpy from a given assignment.

  table:  p = acc > 0.5 ? (int)seg_raw : C  (the last row: nothing rendered; NaN is not > 0.5);  k = label;  counts[p, k] += 1, unless
          k == ignore, k >= L, or the pixel is rendered and seg_raw is not an integer of [0, C).  Integers: tests compare with ==.
  scores: acc = sum_k counts[pi(k), k] / total;  iou_k = counts[pi(k), k] / (row(pi(k)) + col(k) - counts[pi(k), k]), 0 for an unmatched
          label;  miou = mean of iou_k over the labels with a ground-truth pixel."""
import itertools

import numpy as np
import torch


def confusion(seg_raw, accumulation, labels, n_classes, n_labels, ignore_label=255):
    """seg_raw / accumulation float32, labels uint8, any equal-sized shapes (CPU) -> int64 [n_classes + 1, n_labels]."""
    raw, acc, lab = seg_raw.reshape(-1).float().cpu(), accumulation.reshape(-1).float().cpu(), labels.reshape(-1).cpu().long()
    rendered = acc > 0.5
    is_class = (raw >= 0) & (raw < n_classes) & (raw == raw.nan_to_num(-1.0).floor())  # (NaN fails the comparisons)
    keep = (lab != ignore_label) & (lab < n_labels) & (~rendered | is_class)
    row = torch.where(rendered, raw.nan_to_num(0.0).clamp(0, n_classes - 1).long(), torch.full_like(lab, n_classes))
    flat = (row * n_labels + lab)[keep]
    return torch.bincount(flat, minlength=(n_classes + 1) * n_labels).view(n_classes + 1, n_labels)


def case(n_pixels, n_classes, n_labels, seed=0, ignore_label=255):
    """Random inputs of one call: seg_raw in [0, C), accumulation uniform in [0, 1] with one value in eight exactly 0.5 (not rendered),
    labels in [0, L) with one in eight the ignore label."""
    g = torch.Generator().manual_seed(seed * 1_000_003 + n_pixels * 31 + n_classes * 7 + n_labels)
    raw = torch.randint(0, n_classes, (n_pixels,), generator=g).float()
    acc = torch.rand(n_pixels, generator=g)
    acc[torch.rand(n_pixels, generator=g) < 0.125] = 0.5
    lab = torch.randint(0, n_labels, (n_pixels,), generator=g).to(torch.uint8)
    lab[torch.rand(n_pixels, generator=g) < 0.125] = ignore_label
    return raw, acc, lab


def scores(counts, assignment):
    """float64 scores of ``counts`` [P,K] under ``assignment`` (row of every label, -1: none)."""
    c = np.asarray(counts, dtype=np.float64)
    total = c.sum()
    if total == 0:
        return {}
    out, ious = {}, []
    hit = sum(c[p, k] for k, p in enumerate(assignment) if p >= 0)
    out["seg_acc"] = float(hit / total)
    for k, p in enumerate(assignment):
        if p >= 0:
            union = c[p].sum() + c[:, k].sum() - c[p, k]
            out[f"seg_iou_{k}"] = float(c[p, k] / union) if union > 0 else 0.0
        else:
            out[f"seg_iou_{k}"] = 0.0
        if c[:, k].sum() > 0:
            ious.append(out[f"seg_iou_{k}"])
    out["seg_miou"] = sum(ious) / len(ious)  # (added in label order)
    return out


def scipy_assignment(counts):
    """(assignment [K] with -1 for unmatched labels, matched total) from scipy.optimize.linear_sum_assignment(maximize=True)."""
    from scipy.optimize import linear_sum_assignment

    c = np.asarray(counts, dtype=np.int64)
    rows, cols = linear_sum_assignment(c, maximize=True)
    assignment = [-1] * c.shape[1]
    for p, k in zip(rows, cols):
        assignment[int(k)] = int(p)
    return assignment, int(c[rows, cols].sum())


def brute_force(counts):
    """Every optimal assignment of a small table, by enumeration: (list of assignments, best total)."""
    c = np.asarray(counts, dtype=np.int64)
    P, K = c.shape
    best, arg = -1, []
    if P <= K:
        options = ([(p, k) for p, k in enumerate(cols)] for cols in itertools.permutations(range(K), P))
    else:
        options = ([(p, k) for k, p in enumerate(rows)] for rows in itertools.permutations(range(P), K))
    for pairs in options:
        total = int(sum(c[p, k] for p, k in pairs))
        a = [-1] * K
        for p, k in pairs:
            a[k] = p
        if total > best:
            best, arg = total, [a]
        elif total == best:
            arg.append(a)
    return arg, best
