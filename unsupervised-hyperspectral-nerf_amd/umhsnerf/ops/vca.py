"""Vertex component analysis on the device: the endmember initialiser, run once at load."""
from __future__ import annotations

import torch

from .. import _hip
from .._hip import ptr


def vca_rows_per_partial() -> int:
    """K: rows a workgroup of ``vca_moments`` accumulates in fp32 before the partial goes to float64 (its error bound is that of an
    fp32 dot product of length K)."""
    return int(_hip.lib().umhs_vca_rows_per_partial())


def _vca_ws(nbytes: int, dev) -> torch.Tensor:
    """A fresh allocation per call, on purpose: sized by the rows of the split and used once at load, a cached one would pin that
    memory for the whole run.  It goes back to the allocator; it is not parked in the workspace registry."""
    return torch.empty(max(int(nbytes), 8), device=dev, dtype=torch.uint8)


def vca_moments(rows, sum_out=None, s_out=None):
    """(sum [B], S [B,B]) float64 of pixel rows [N,B] fp32: sum_n y_nb and sum_n y_ni y_nj.  Given ``sum_out`` / ``s_out`` (both) the
    call ADDS to them -- a stack is fed one frame at a time.  Bitwise reproducible."""
    assert rows.dim() == 2 and rows.dtype == torch.float32 and (sum_out is None) == (s_out is None)
    n, b = rows.shape
    accumulate = sum_out is not None
    if not accumulate:
        sum_out, s_out = (torch.zeros(s, dtype=torch.float64, device=rows.device) for s in ((b,), (b, b)))
    lib = _hip.lib()
    ws = _vca_ws(lib.umhs_vca_moments_workspace_bytes(n, b), rows.device)
    _hip.check(lib.umhs_vca_moments(ptr(rows), n, b, int(accumulate), ptr(sum_out), ptr(s_out), ptr(ws), ws.numel(), _hip.stream()),
               "umhs_vca_moments")
    return sum_out, s_out


def vca_project(rows, basis16, num_classes: int, mean=None, out=None):
    """y [N,16] fp32 from rows [N,B] and basis16 [B,16].  ``mean`` None: the projective form (column 15 of the basis = Ud u,
    y = x / (x_15 + 1e-6)) -> (y, None); ``mean`` [B]: the affine form x = basis^T (row - mean) -> (y, max_n |x_n|^2 as a 1-element
    tensor).  ``out``: a [N,16] slice of a larger y to fill."""
    assert rows.dim() == 2 and rows.dtype == torch.float32 and tuple(basis16.shape) == (rows.shape[1], 16)
    n, b = rows.shape
    dev = rows.device
    y = torch.empty(n, 16, device=dev, dtype=torch.float32) if out is None else out
    assert tuple(y.shape) == (n, 16) and y.dtype == torch.float32
    affine = mean is not None
    mx = torch.zeros(1, device=dev, dtype=torch.float32) if affine else None
    lib = _hip.lib()
    ws = _vca_ws(lib.umhs_vca_project_workspace_bytes(n), dev)
    _hip.check(lib.umhs_vca_project(ptr(rows), n, b, ptr(_hip.f32c(basis16)), ptr(_hip.f32c(mean)) if affine else None, int(num_classes),
                                    int(affine), ptr(y), ptr(mx), ptr(ws), ws.numel(), _hip.stream()), "umhs_vca_project")
    return y, mx


def vca_argmax(y, f, bias: float = 0.0):
    """argmax_n |bias + f . y_n| over y [N,16] (``f``: up to 16 host floats), the lowest index among equal values
    -> (index [1] int64, row [16] fp32, value [1] fp32), all on the device."""
    assert y.dim() == 2 and y.shape[1] == 16 and y.dtype == torch.float32 and y.shape[0] > 0
    dev = y.device
    fh = (_hip._f32 * 16)(*[float(v) for v in f])
    index = torch.zeros(1, dtype=torch.int64, device=dev)
    row, value = torch.zeros(16, device=dev), torch.zeros(1, device=dev)
    lib = _hip.lib()
    ws = _vca_ws(lib.umhs_vca_argmax_workspace_bytes(y.shape[0]), dev)
    _hip.check(lib.umhs_vca_argmax(ptr(y), y.shape[0], fh, float(bias), ptr(index), ptr(row), ptr(value), ptr(ws), ws.numel(),
                                   _hip.stream()), "umhs_vca_argmax")
    return index, row, value
