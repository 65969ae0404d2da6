"""Scene statistics (include/umhs_hip.h, "Scene statistics"): the count, sum and Gram matrix of the valid spectra, and the centred
projection that turns them into principal components and RX scores."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import _hip
from .._hip import ptr
from .workspace import _workspace

STATISTICS_MAX_BANDS = 256


def gram_chunk() -> int:
    """UMHS_GRAM_CHUNK: the rows whose products are chained in float32 before they are added in float64."""
    return int(_hip.lib().umhs_gram_chunk())


def _rows(spectra: torch.Tensor, what: str):
    """[...,B] float32 device tensor -> (rows [R,B] read in place where the strides allow it, R, B, stride)."""
    if spectra.dtype != torch.float32 or spectra.dim() < 1:
        raise ValueError(f"{what} needs a float32 tensor [...,B]")
    if not spectra.is_cuda:
        raise RuntimeError("umhsnerf HIP ops need tensors on a HIP device (cuda:N); there is no CPU path")
    B = int(spectra.shape[-1])
    s = spectra.detach().reshape(-1, B)  # (a view when the leading dimensions allow it, else a copy)
    R = int(s.shape[0])
    if (B > 1 and s.stride(1) != 1) or (R > 1 and s.stride(0) < B):
        s = s.contiguous()
    return s, R, B, (int(s.stride(0)) if R > 1 else B)


def gram_accumulate(spectra: torch.Tensor, shift: torch.Tensor, acc: torch.Tensor, accumulation: Optional[torch.Tensor] = None) -> None:
    """Adds the valid rows of ``spectra`` (float32 [...,B], read in place as ``library_match`` reads them) to ``acc``, a float64 device
    tensor [1 + B + B*B] = (count, sum of x - shift, Gram matrix of x - shift) that the caller zeroed before the first call.  ``shift``
    float32 [B] stays the same for the whole accumulation; ``accumulation`` float32 [...,1] or [R]: rows at <= 0.5 are left out, as are
    rows with a NaN or an Inf.  No host sync."""
    s, R, B, stride = _rows(spectra, "gram_accumulate")
    if not 1 <= B <= STATISTICS_MAX_BANDS:
        raise ValueError(f"{B} bands are outside the kernel's limits (1..{STATISTICS_MAX_BANDS})")
    if shift.dtype != torch.float32 or tuple(shift.shape) != (B,):
        raise ValueError(f"shift must be float32 [{B}]")
    if acc.dtype != torch.float64 or tuple(acc.shape) != (1 + B + B * B,):
        raise ValueError(f"acc must be float64 [{1 + B + B * B}]")
    a = None
    if accumulation is not None:
        a = accumulation.detach().reshape(-1)
        if a.dtype != torch.float32 or a.numel() != R:
            raise ValueError(f"accumulation must be float32 with one value per row ({R})")
        a = a.contiguous()
    if R == 0:
        return
    lib = _hip.lib()
    nbytes = int(lib.umhs_gram_workspace_bytes(R, B))
    ws = _workspace(nbytes, s.device, "gram", floor=1 << 16)
    _hip.check(lib.umhs_gram_accumulate(_hip.C.c_void_p(s.data_ptr()), stride, R, B, ptr(shift), ptr(a), ptr(acc), ptr(ws), ws.numel(),
                                        _hip.stream()), "umhs_gram_accumulate")


def spectral_project(spectra: torch.Tensor, mean: torch.Tensor, image: torch.Tensor, K: int, P: int,
                     want_score: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """y = W (x - mean) for every row of ``spectra`` (float32 [...,B], read in place), W [K,B] given as the operand image
    ``library_prepare(W)`` makes.  Returns ``(components float32 [R,P], score float32 [R] or None)``: the first P entries of y, and the
    sum of the squares of all K.  A row with a NaN or an Inf gives zeros.  One launch, no host sync."""
    s, R, B, stride = _rows(spectra, "spectral_project")
    K, P = int(K), int(P)
    if not image.is_cuda:
        raise RuntimeError("umhsnerf HIP ops need tensors on a HIP device (cuda:N); there is no CPU path")
    if not 0 <= P <= K:
        raise ValueError(f"P = {P} components of K = {K}")
    if mean.dtype != torch.float32 or tuple(mean.shape) != (B,):
        raise ValueError(f"mean must be float32 [{B}]")
    if image.dtype != torch.float32 or int(_hip.lib().umhs_library_image_bytes(K, B)) != image.numel() * 4 or image.numel() == 0:
        raise ValueError(f"the image does not belong to a matrix of {K} rows x {B} bands (1..256 each)")
    components = torch.empty(R, P, dtype=torch.float32, device=s.device)
    score = torch.empty(R, dtype=torch.float32, device=s.device) if want_score else None
    _hip.check(_hip.lib().umhs_spectral_project(_hip.C.c_void_p(s.data_ptr()), stride, R, ptr(mean), ptr(image), K, B, P,
                                                ptr(components) if P > 0 else None, ptr(score), _hip.stream()), "umhs_spectral_project")
    return components, score
