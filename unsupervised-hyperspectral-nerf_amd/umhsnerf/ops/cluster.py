"""Spectral clustering (include/umhs_hip.h, "Spectral clustering"): one pass of Lloyd's algorithm over the rows -- the nearest centre
of every row and, in the same pass, the sums of each cluster's rows."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import _hip
from .._hip import ptr
from .statistics import _rows
from .workspace import _workspace

CLUSTER_ANGLE, CLUSTER_EUCLIDEAN = 0, 1
CLUSTER_MAX, CLUSTER_MAX_BANDS = 64, 256
CLUSTER_METRICS = {"angle": CLUSTER_ANGLE, "euclidean": CLUSTER_EUCLIDEAN}


def cluster_chunk() -> int:
    """UMHS_CLUSTER_CHUNK: the rows whose member vectors are summed in float32 before they are added in float64."""
    return int(_hip.lib().umhs_cluster_chunk())


def cluster_step(spectra: torch.Tensor, image: torch.Tensor, K: int, metric, half_norm: Optional[torch.Tensor] = None,
                 mask: Optional[torch.Tensor] = None, acc: Optional[torch.Tensor] = None, want_label: bool = True,
                 want_score: bool = True) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Assigns every row of ``spectra`` (float32 [...,B], read in place as ``library_match`` reads them) to the nearest of K centres,
    given as the operand image ``library_prepare`` makes of them: unit rows for ``metric`` "angle" (or 0), the centres themselves with
    ``half_norm`` float32 [K] = |c|^2 / 2 for "euclidean" (or 1).  ``mask`` float32 [...,1] or [R]: rows at <= 0.5 are left out, as
    are rows that are all zero or hold a NaN or an Inf.  ``acc``: a float64 device tensor [2 + K + K*B] = (valid rows, objective,
    count per cluster, sum of member vectors per cluster) that the caller zeroed before the first call; the call adds to it.
    Returns ``(label int32 [R] or None, score float32 [R] or None)``: -1 / 0 for a row left out; the score is the cosine or the
    squared distance.  One launch without ``acc``; no host sync."""
    s, R, B, stride = _rows(spectra, "cluster_step")
    K = int(K)
    metric = CLUSTER_METRICS.get(metric, metric) if isinstance(metric, str) else int(metric)
    if metric not in (CLUSTER_ANGLE, CLUSTER_EUCLIDEAN):
        raise ValueError(f"metric must be one of {sorted(CLUSTER_METRICS)} (or 0 / 1), got {metric!r}")
    if not 1 <= B <= CLUSTER_MAX_BANDS or not 1 <= K <= CLUSTER_MAX:
        raise ValueError(f"{K} clusters on {B} bands are outside the kernel's limits (1..{CLUSTER_MAX} clusters, 1..{CLUSTER_MAX_BANDS} bands)")
    if not image.is_cuda:
        raise RuntimeError("umhsnerf HIP ops need tensors on a HIP device (cuda:N); there is no CPU path")
    if image.dtype != torch.float32 or int(_hip.lib().umhs_library_image_bytes(K, B)) != image.numel() * 4:
        raise ValueError(f"the image does not belong to {K} centres x {B} bands")
    if metric == CLUSTER_EUCLIDEAN:
        if half_norm is None or half_norm.dtype != torch.float32 or tuple(half_norm.shape) != (K,):
            raise ValueError(f"the euclidean metric needs half_norm float32 [{K}]")
    else:
        half_norm = None
    if acc is not None and (acc.dtype != torch.float64 or tuple(acc.shape) != (2 + K + K * B,)):
        raise ValueError(f"acc must be float64 [{2 + K + K * B}]")
    m = None
    if mask is not None:
        m = mask.detach().reshape(-1)
        if m.dtype != torch.float32 or m.numel() != R:
            raise ValueError(f"mask must be float32 with one value per row ({R})")
        m = m.contiguous()
    label = torch.empty(R, dtype=torch.int32, device=s.device) if want_label else None
    score = torch.empty(R, dtype=torch.float32, device=s.device) if want_score else None
    if R == 0:
        return label, score
    lib = _hip.lib()
    ws, nbytes = None, 0
    if acc is not None:
        nbytes = int(lib.umhs_cluster_workspace_bytes(R, K, B))
        ws = _workspace(nbytes, s.device, "cluster", floor=1 << 16)
    _hip.check(lib.umhs_cluster_step(_hip.C.c_void_p(s.data_ptr()), stride, R, ptr(m), ptr(image), ptr(half_norm), K, B, metric,
                                     ptr(label), ptr(score), ptr(acc), ptr(ws), ws.numel() if ws is not None else 0, _hip.stream()),
               "umhs_cluster_step")
    return label, score
