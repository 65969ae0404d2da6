"""Evaluation operators: image metrics, SSIM, the segmentation confusion table and per-segment gradient statistics."""
from __future__ import annotations

from typing import List, Optional

import torch

from .. import _hip
from .._hip import ptr
from .workspace import _workspace


def pixel_metrics(pred, gt):
    """(sum of squared errors, sum of finite spectral angles, number of finite angles) over channel-last images [...,K]; float64."""
    k = pred.shape[-1]
    p, g = _hip.f32c(pred).view(-1, k), _hip.f32c(gt).view(-1, k)
    assert p.shape == g.shape
    nb = max(1, min(1024, (p.shape[0] + 255) // 256))
    part = torch.empty(nb, 3, dtype=torch.float64, device=p.device)
    _hip.check(_hip.lib().umhs_pixel_metrics(ptr(p), ptr(g), p.shape[0], k, ptr(part), nb, _hip.stream()), "umhs_pixel_metrics")
    return part.sum(0)


class SegmentBounds:
    """Ascending element offsets [K+1] of ``segment_stats``, kept in both places the call needs them: ``host`` (the argument checks and
    the grid size are host arithmetic) and ``device`` (what the kernels read).  Built once -- ``SegmentBounds(offsets, device)`` or
    ``SegmentBounds.of_layout(layout, device)`` -- and reused, so a call uploads nothing and reads nothing back."""

    def __init__(self, offsets, device):
        values = [int(v) for v in (offsets.tolist() if torch.is_tensor(offsets) else offsets)]  # (a device tensor is read once, here)
        if len(values) < 2:
            raise ValueError("segment bounds need at least two offsets (K >= 1)")
        self.k = len(values) - 1
        self.values = values
        self.host = (_hip._i64 * len(values))(*values)
        self.device = torch.tensor(values, dtype=torch.int64, device=device)
        self.names: Optional[List[str]] = None

    @classmethod
    def of_layout(cls, layout, device) -> "SegmentBounds":
        """One segment per entry of a flat parameter layout, in layout order: entry i = [offset_i, offset_i + numel_i).  The layout pads
        every entry to 16 bytes, so segment i is cut at offset_{i+1} and a statistics row covers the entry plus its (zero) padding."""
        names = list(layout.entries)
        offsets = [layout.entries[k][0] for k in names] + [layout.total]
        self = cls(offsets, device)
        self.names = names
        return self


def segment_stats_tile() -> int:
    """Elements per tile of ``segment_stats`` (its error bound is a function of it: tests/stats_f64.py)."""
    return int(_hip.lib().umhs_segment_stats_tile())


def segment_stats(x, bounds, out=None):
    """float64 [K,3] per segment ``[bounds[k], bounds[k+1])`` of the contiguous float32 device buffer ``x``: the sum of x^2 and the
    maximum of |x| over the finite elements, and the number of NaN / +-Inf.  ``bounds``: a ``SegmentBounds`` (nothing is uploaded) or
    int64 offsets [K+1] as a list / tensor (a ``SegmentBounds`` is built for the call; a device tensor costs a host read).  One pass over
    ``x``, float64 sums in a fixed order (the same bits on every launch), no host sync; descending offsets or offsets outside the buffer
    raise before anything is launched.  ``out``: a float64 [K,3] device tensor to fill."""
    if not torch.is_tensor(x) or x.dtype != torch.float32:
        raise ValueError("segment_stats needs a float32 tensor")
    flat = x.detach().reshape(-1) if x.is_contiguous() else None
    pointer = ptr(flat if flat is not None else x.detach())  # (a CPU or non-contiguous tensor raises here: there is no CPU path)
    if not isinstance(bounds, SegmentBounds):
        bounds = SegmentBounds(bounds, flat.device)
    if bounds.device.device != flat.device:
        raise ValueError(f"segment bounds live on {bounds.device.device}, the buffer on {flat.device}")
    if out is None:
        out = torch.empty(bounds.k, 3, dtype=torch.float64, device=flat.device)
    elif out.dtype != torch.float64 or tuple(out.shape) != (bounds.k, 3) or out.device != flat.device:
        raise ValueError(f"out must be float64 [{bounds.k}, 3] on {flat.device}")
    lib = _hip.lib()
    ws = _workspace(lib.umhs_segment_stats_workspace_bytes(flat.numel(), bounds.k), flat.device, "segment_stats", floor=1 << 16)
    _hip.check(lib.umhs_segment_stats(pointer, flat.numel(), ptr(bounds.device), bounds.host, bounds.k, ptr(out), ptr(ws), ws.numel(),
                                      _hip.stream()), "umhs_segment_stats")
    return out


def seg_confusion(seg_raw, accumulation, seg_image, n_classes: int, n_labels: int, ignore_label: int = 255, out=None):
    """Confusion table int64 [n_classes + 1, n_labels] of the labels the model emitted against a ground-truth label image: per pixel
    one count at [accumulation > 0.5 ? seg_raw : n_classes, seg_image] (the last row is "nothing rendered"); pixels whose label is
    ``ignore_label`` (-1: none) or >= n_labels, or whose ``seg_raw`` is no class, are skipped.  Any shapes with equal element counts;
    ``out``: a table to ADD into (returned).  One launch, no host sync."""
    raw, acc = _hip.f32c(seg_raw).reshape(-1), _hip.f32c(accumulation).reshape(-1)
    if seg_image.dtype != torch.uint8:
        raise ValueError(f"seg_image must be uint8, got {seg_image.dtype}")
    lab = seg_image.reshape(-1)  # (a view of a contiguous slice keeps its byte offset: the kernel takes any alignment)
    if not raw.numel() == acc.numel() == lab.numel():
        raise ValueError(f"seg_raw, accumulation and seg_image differ in size: {raw.numel()}, {acc.numel()}, {lab.numel()}")
    pointers = ptr(raw), ptr(acc), ptr(lab)  # (a CPU tensor raises here: there is no CPU path)
    if out is None:
        out = torch.zeros(n_classes + 1, n_labels, dtype=torch.int64, device=raw.device)
    elif out.dtype != torch.int64 or tuple(out.shape) != (n_classes + 1, n_labels):
        raise ValueError(f"out must be int64 [{n_classes + 1}, {n_labels}], got {out.dtype} {tuple(out.shape)}")
    if raw.numel() == 0:
        return out
    _hip.check(_hip.lib().umhs_seg_confusion(*pointers, raw.numel(), int(n_classes), int(n_labels), int(ignore_label),
                                             ptr(out), _hip.stream()), "umhs_seg_confusion")
    return out


def ssim(a, b, data_range=None):
    """torchmetrics structural_similarity_index_measure (gaussian 11x11, sigma 1.5) of channel-last images [H,W,K] -> 0-dim float64."""
    a, b = _hip.f32c(a), _hip.f32c(b)
    assert a.dim() == 3 and a.shape == b.shape
    h, w, k = a.shape
    n = _hip.lib().umhs_ssim_partials(h, w, k)
    if n == 0:
        raise ValueError(f"SSIM needs images of at least 11x11 pixels, got {h}x{w}")
    if data_range is None:
        (alo, ahi), (blo, bhi) = torch.aminmax(a), torch.aminmax(b)
        dr = torch.maximum(ahi - alo, bhi - blo).reshape(1)
    else:
        dr = torch.full((1,), float(data_range), device=a.device)
    part = torch.empty(n, dtype=torch.float64, device=a.device)
    _hip.check(_hip.lib().umhs_ssim(ptr(a), ptr(b), h, w, k, ptr(dr), ptr(part), n, _hip.stream()), "umhs_ssim")
    return part.sum() / float((h - 10) * (w - 10) * k)
