"""Spectral library matching (include/umhs_hip.h, "Spectral library matching"): the two best entries of a library per spectrum."""
from __future__ import annotations

from typing import Tuple

import torch

from .. import _hip
from .._hip import ptr

LIBRARY_MAX_BANDS = 256
LIBRARY_MAX_ENTRIES = 65536


def library_prepare(unit: torch.Tensor) -> torch.Tensor:
    """``unit``: float32 [L,B] device tensor of library rows already of unit length -> the operand image ``library_match`` streams
    (a flat float32 tensor; made once per library)."""
    if unit.dim() != 2 or unit.dtype != torch.float32:
        raise ValueError("library_prepare needs a float32 [L,B] tensor")
    L, B = int(unit.shape[0]), int(unit.shape[1])
    pointer = ptr(unit)  # (a CPU or non-contiguous tensor raises here: there is no CPU path)
    nbytes = int(_hip.lib().umhs_library_image_bytes(L, B))
    if nbytes == 0:
        raise ValueError(f"a library of {L} entries x {B} bands is outside the kernel's limits "
                         f"(1..{LIBRARY_MAX_ENTRIES} entries, 1..{LIBRARY_MAX_BANDS} bands)")
    image = torch.empty(nbytes // 4, dtype=torch.float32, device=unit.device)
    _hip.check(_hip.lib().umhs_library_prepare(pointer, L, B, ptr(image), _hip.stream()), "umhs_library_prepare")
    return image


def library_match(spectra: torch.Tensor, image: torch.Tensor, L: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``spectra``: float32 [...,B] device tensor whose rows are ``stride(-2)`` floats apart (a column slice of a wider array is read
    in place).  Returns ``(index int32 [R,2], cos float32 [R,2])``, R the number of rows: the entry of largest cosine and the one of
    second largest; -1 where there is none (the header has every rule).  One launch, no host sync."""
    if spectra.dtype != torch.float32 or spectra.dim() < 1:
        raise ValueError("library_match needs a float32 tensor [...,B]")
    if not spectra.is_cuda or not image.is_cuda:
        raise RuntimeError("umhsnerf HIP ops need tensors on a HIP device (cuda:N); there is no CPU path")
    B = int(spectra.shape[-1])
    s = spectra.detach().reshape(-1, B)  # (a view when the leading dimensions allow it, else a copy)
    R = int(s.shape[0])
    if (B > 1 and s.stride(1) != 1) or (R > 1 and s.stride(0) < B):
        s = s.contiguous()
    stride = int(s.stride(0)) if R > 1 else B
    if int(_hip.lib().umhs_library_image_bytes(int(L), B)) != image.numel() * 4 or image.dtype != torch.float32:
        raise ValueError(f"the image does not belong to a library of {L} entries x {B} bands")
    index = torch.empty(R, 2, dtype=torch.int32, device=s.device)
    cos = torch.empty(R, 2, dtype=torch.float32, device=s.device)
    _hip.check(_hip.lib().umhs_library_match(_hip.C.c_void_p(s.data_ptr()), stride, R, ptr(image), int(L), B, ptr(index), ptr(cos),
                                             _hip.stream()), "umhs_library_match")
    return index, cos
