"""Scores of an unsupervised segmentation against ground-truth labels, from the confusion table ``ops.seg_confusion`` accumulates:
``counts[p, k]`` = pixels the model put into row ``p`` (a cluster, or the last row: "nothing rendered") whose label is ``k``.

Clusters carry no names, so they are matched to the labels first: ``match_clusters`` finds the injective partial map from label ``k`` to
row ``pi(k)`` that maximises ``sum_k counts[pi(k), k]`` -- a rectangular assignment problem of at most 17 x 32, solved here by the
Hungarian method with potentials (shortest augmenting paths, O(n^2 m)) on Python integers, so the optimum is exact.  The empty row takes
part like any cluster: a scene's background label then maps to "nothing rendered".  Host code, numpy / torch only."""
from __future__ import annotations

from typing import Dict, List


def _table(counts) -> List[List[int]]:
    rows = counts.tolist() if hasattr(counts, "tolist") else [list(r) for r in counts]
    if not rows or not isinstance(rows[0], list):
        raise ValueError("counts must be a two-dimensional table [rows, labels]")
    return [[int(v) for v in r] for r in rows]


def _assign_min(cost: List[List[int]]) -> List[int]:
    """Column of every row of an n x m cost table, n <= m, all different, with the smallest total."""
    n, m = len(cost), len(cost[0])
    inf = float("inf")
    u, v, p, way = [0] * (n + 1), [0] * (m + 1), [0] * (m + 1), [0] * (m + 1)  # potentials; p[j] = row matched to column j (1-based)
    for i in range(1, n + 1):
        p[0], j0 = i, 0
        minv, used = [inf] * (m + 1), [False] * (m + 1)
        while True:  # grow the alternating tree from row i until it reaches a free column
            used[j0] = True
            i0, delta, j1 = p[j0], inf, 0
            for j in range(1, m + 1):
                if not used[j]:
                    cur = cost[i0 - 1][j - 1] - u[i0] - v[j]
                    if cur < minv[j]:
                        minv[j], way[j] = cur, j0
                    if minv[j] < delta:
                        delta, j1 = minv[j], j
            for j in range(m + 1):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:  # flip the path
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    col = [0] * n
    for j in range(1, m + 1):
        if p[j]:
            col[p[j] - 1] = j - 1
    return col


def match_clusters(counts) -> List[int]:
    """``assignment[k]`` = the row matched to label ``k``, or -1 for a label left without a row (more labels than rows): the
    ``min(P, K)`` pairs, no row used twice, with the largest ``sum_k counts[assignment[k], k]``."""
    t = _table(counts)
    P, K = len(t), len(t[0])
    assignment = [-1] * K
    if K == 0:
        return assignment
    if P <= K:
        for p, k in enumerate(_assign_min([[-v for v in row] for row in t])):
            assignment[k] = p
    else:
        for k, p in enumerate(_assign_min([[-t[p][k] for p in range(P)] for k in range(K)])):
            assignment[k] = p
    return assignment


def seg_scores(counts) -> Dict:
    """``seg_acc`` = matched pixels / scored pixels; ``seg_iou_<k>`` = counts[pi(k), k] / (row sum of pi(k) + column sum of k - counts[pi(k), k])
    (0 for a label left without a row); ``seg_miou`` = their mean over the labels that have a ground-truth pixel; ``assignment``.
    A table without a single count gives ``{}``."""
    t = _table(counts)
    total = sum(sum(r) for r in t)
    if total == 0:
        return {}
    K = len(t[0])
    assignment = match_clusters(t)
    row_sum, col_sum = [sum(r) for r in t], [sum(r[k] for r in t) for k in range(K)]
    out: Dict = {"seg_acc": sum(t[p][k] for k, p in enumerate(assignment) if p >= 0) / total}
    ious = []
    for k, p in enumerate(assignment):
        hit = t[p][k] if p >= 0 else 0
        union = (row_sum[p] if p >= 0 else 0) + col_sum[k] - hit
        out[f"seg_iou_{k}"] = hit / union if union > 0 else 0.0
        if col_sum[k] > 0:
            ious.append(out[f"seg_iou_{k}"])
    out["seg_miou"] = sum(ious) / len(ious)
    out["assignment"] = assignment
    return out
