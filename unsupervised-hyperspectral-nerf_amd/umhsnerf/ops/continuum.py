"""Continuum removal (include/umhs_hip.h, "Continuum removal"): every row divided by the upper convex hull of its spectrum over
wavelength, and depth / centre / area of up to 8 absorption features, by one launch of csrc/umhs_continuum.hip."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch

from .. import _hip
from .._hip import ptr
from .statistics import _rows
from .workspace import _workspace

CONTINUUM_MAX_BANDS = 256  # UMHS_CONTINUUM_MAX_BANDS
CONTINUUM_MAX_FEATURES = 8  # UMHS_CONTINUUM_MAX_FEATURES
CONTINUUM_MIN_FEATURE_BANDS = 3


def continuum(spectra: torch.Tensor, wavelengths: torch.Tensor, feature_ranges: Sequence[Sequence[int]] = (), want_removed: bool = True,
              want_status: bool = False) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]:
    """``spectra`` float32 [...,B], read in place as ``library_match`` reads them; ``wavelengths`` float32 [B] on the device, finite and
    strictly increasing (the caller's to check: ``umhsnerf.continuum.ContinuumAnalysis`` does); ``feature_ranges``: up to 8 inclusive
    band ranges (lo, hi) of at least 3 bands, host integers -- they travel as kernel arguments.  Returns ``(removed float32 [R,B] or
    None, features float32 [R,F,3] or None (F = 0), status int32 [R] or None)``: removed = x / continuum over the full range (1 where
    the continuum is not positive); features[:, f] = (depth, centre, area) of feature f on the hull of its own range; status = the
    vertices of the full-range hull, -1 for a row with a NaN or an Inf (removed and features 0).  One launch, no host sync."""
    s, R, B, stride = _rows(spectra, "continuum")
    ranges = [(int(lo), int(hi)) for lo, hi in feature_ranges]
    F = len(ranges)
    if not 1 <= B <= CONTINUUM_MAX_BANDS or F > CONTINUUM_MAX_FEATURES:
        raise ValueError(f"{F} features on {B} bands are outside the kernel's limits (0..{CONTINUUM_MAX_FEATURES}, 1..{CONTINUUM_MAX_BANDS})")
    for f, (lo, hi) in enumerate(ranges):
        if not 0 <= lo <= hi < B:
            raise ValueError(f"feature {f}: the band range [{lo}, {hi}] is outside 0..{B - 1}")
        if hi - lo + 1 < CONTINUUM_MIN_FEATURE_BANDS:
            raise ValueError(f"feature {f}: the band range [{lo}, {hi}] holds fewer than {CONTINUUM_MIN_FEATURE_BANDS} bands")
    if not wavelengths.is_cuda:
        raise RuntimeError("umhsnerf HIP ops need tensors on a HIP device (cuda:N); there is no CPU path")
    if wavelengths.dtype != torch.float32 or tuple(wavelengths.shape) != (B,) or not wavelengths.is_contiguous():
        raise ValueError(f"wavelengths must be a contiguous float32 [{B}]")
    removed = torch.empty(R, B, dtype=torch.float32, device=s.device) if want_removed else None
    features = torch.empty(R, F, 3, dtype=torch.float32, device=s.device) if F else None
    status = torch.empty(R, dtype=torch.int32, device=s.device) if want_status else None
    lib = _hip.lib()
    nbytes = int(lib.umhs_continuum_workspace_bytes(R, B, F))
    ws = _workspace(nbytes, s.device, "continuum") if nbytes > 0 else None
    host = (C.c_int32 * (2 * max(F, 1)))(*[v for r in ranges for v in r])
    _hip.check(lib.umhs_continuum(C.c_void_p(s.data_ptr()), stride, R, ptr(wavelengths), B, C.cast(host, C.c_void_p) if F else None, F,
                                  ptr(removed), ptr(features), ptr(status), ptr(ws), nbytes, _hip.stream()), "umhs_continuum")
    return removed, features, status
