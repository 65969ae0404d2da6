"""Spectral unmixing (include/umhs_hip.h, "Spectral unmixing"): the constrained least-squares abundances of every row against K
endmembers, by one launch of csrc/umhs_unmix.hip."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import _hip
from .._hip import ptr
from .statistics import _rows
from .workspace import _workspace

UNMIX_NNLS, UNMIX_FCLS = 0, 1  # UMHS_UNMIX_NNLS, UMHS_UNMIX_FCLS
UNMIX_MAX_ENDMEMBERS = 16  # UMHS_UNMIX_MAX_ENDMEMBERS
UNMIX_MAX_BANDS = 256


def unmix(spectra: torch.Tensor, image: torch.Tensor, gram: torch.Tensor, K: int, mode: int, want_residual: bool = True,
          want_status: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """a = argmin |x - E^T a|^2 over a >= 0 (``mode`` UNMIX_NNLS) and sum a = 1 (UNMIX_FCLS) for every row of ``spectra`` (float32
    [...,B], read in place as ``library_match`` reads them).  ``image``: ``library_prepare(E)`` of the float32 endmembers E [K,B], NOT
    normalised; ``gram``: float32 [K,K] = E E^T formed in float64 and rounded once.  Returns ``(abundances float32 [R,K], residual
    float32 [R] or None, status int32 [R] or None)``: residual = |x - E^T a|^2; status = the solves used, -1 for an invalid row (a NaN,
    an Inf, all zeros: abundances 0), -2 for a row stopped at the cap of 3 K + 3 solves.  One launch, no host sync."""
    s, R, B, stride = _rows(spectra, "unmix")
    K, mode = int(K), int(mode)
    if not image.is_cuda or not gram.is_cuda:
        raise RuntimeError("umhsnerf HIP ops need tensors on a HIP device (cuda:N); there is no CPU path")
    if not 1 <= B <= UNMIX_MAX_BANDS or not 1 <= K <= UNMIX_MAX_ENDMEMBERS:
        raise ValueError(f"{K} endmembers on {B} bands are outside the kernel's limits (1..{UNMIX_MAX_ENDMEMBERS}, 1..{UNMIX_MAX_BANDS})")
    if mode not in (UNMIX_NNLS, UNMIX_FCLS):
        raise ValueError(f"mode must be UNMIX_NNLS (0) or UNMIX_FCLS (1), got {mode}")
    lib = _hip.lib()
    if image.dtype != torch.float32 or int(lib.umhs_library_image_bytes(K, B)) != image.numel() * 4:
        raise ValueError(f"the image does not belong to a matrix of {K} rows x {B} bands")
    if gram.dtype != torch.float32 or tuple(gram.shape) != (K, K) or not gram.is_contiguous():
        raise ValueError(f"gram must be a contiguous float32 [{K},{K}]")
    abundances = torch.empty(R, K, dtype=torch.float32, device=s.device)
    residual = torch.empty(R, dtype=torch.float32, device=s.device) if want_residual else None
    status = torch.empty(R, dtype=torch.int32, device=s.device) if want_status else None
    nbytes = int(lib.umhs_unmix_workspace_bytes(R, K, B))
    ws = _workspace(nbytes, s.device, "unmix") if nbytes > 0 else None
    _hip.check(lib.umhs_unmix(_hip.C.c_void_p(s.data_ptr()), stride, R, ptr(image), ptr(gram), K, B, mode, ptr(abundances), ptr(residual),
                              ptr(status), ptr(ws), nbytes, _hip.stream()), "umhs_unmix")
    return abundances, residual, status
