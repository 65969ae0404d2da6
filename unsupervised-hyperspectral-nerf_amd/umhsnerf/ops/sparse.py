"""Sparse unmixing (include/umhs_hip.h, "Sparse unmixing"): the non-negative lasso of every row against a whole spectral library, by
one launch of csrc/umhs_sparse.hip."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from .. import _hip
from .._hip import ptr
from .library import library_prepare
from .statistics import _rows

SPARSE_MAX_ENTRIES = 128  # UMHS_SPARSE_MAX_ENTRIES
SPARSE_MAX_BANDS = 256
SPARSE_RHO = 0.1  # mu = SPARSE_RHO trace(A A^T) / L (DESIGN.md has the table it was chosen from)


@dataclass(frozen=True)
class SparseOperands:
    """What ``sparse_prepare`` makes once per (library, lambda, mu) and ``sparse_unmix`` streams."""
    q_image: torch.Tensor
    m_image: torch.Tensor
    a_image: torch.Tensor
    g_image: torch.Tensor
    theta: float
    lambda_: float
    mu: float
    L: int
    B: int


def sparse_auto_mu(A, rho: float = SPARSE_RHO) -> float:
    """mu = rho trace(A A^T) / L, in float64 from the float32 A."""
    A64 = (A.detach().cpu().numpy() if isinstance(A, torch.Tensor) else np.asarray(A)).astype(np.float32).astype(np.float64)
    return float(rho * (A64 * A64).sum() / A64.shape[0])


def _square_image(matrix: np.ndarray, device) -> torch.Tensor:
    m = torch.from_numpy(np.ascontiguousarray(matrix.astype(np.float32))).to(device)
    L = int(m.shape[0])
    image = torch.empty(int(_hip.lib().umhs_sparse_image_bytes(L)) // 4, dtype=torch.float32, device=device)
    _hip.check(_hip.lib().umhs_sparse_prepare(ptr(m), L, ptr(image), _hip.stream()), "umhs_sparse_prepare")
    return image


def sparse_prepare(A: torch.Tensor, lambda_: float, mu: float) -> SparseOperands:
    """``A``: float32 [L,B] device tensor, the library as it is (NOT normalised).  Forms G = A A^T, F = (G + mu I)^-1, Q = F A,
    M = mu F and theta = lambda / mu in float64 on the host, rounds each to float32 once and lays them out for the kernel.  Made once
    per (library, lambda, mu); it copies A to the host, so it synchronises."""
    if A.dim() != 2 or A.dtype != torch.float32:
        raise ValueError("sparse_prepare needs a float32 [L,B] tensor")
    if not A.is_cuda:
        raise RuntimeError("umhsnerf HIP ops need tensors on a HIP device (cuda:N); there is no CPU path")
    L, B = int(A.shape[0]), int(A.shape[1])
    if not 1 <= L <= SPARSE_MAX_ENTRIES or not 1 <= B <= SPARSE_MAX_BANDS:
        raise ValueError(f"a library of {L} entries x {B} bands is outside the kernel's limits (1..{SPARSE_MAX_ENTRIES} entries, "
                         f"1..{SPARSE_MAX_BANDS} bands)")
    lambda_, mu = float(lambda_), float(mu)
    if not lambda_ >= 0.0 or not np.isfinite(lambda_):
        raise ValueError(f"lambda must be finite and >= 0, got {lambda_}")
    if not mu > 0.0 or not np.isfinite(mu):
        raise ValueError(f"mu must be finite and > 0, got {mu}")
    A64 = A.detach().cpu().numpy().astype(np.float64)
    if not np.isfinite(A64).all():
        raise ValueError("the library holds a NaN or an Inf")
    G = A64 @ A64.T
    F = np.linalg.inv(G + mu * np.eye(L))
    F = 0.5 * (F + F.T)
    Q = torch.from_numpy((F @ A64).astype(np.float32)).to(A.device)
    return SparseOperands(q_image=library_prepare(Q), m_image=_square_image(mu * F, A.device), a_image=library_prepare(A.contiguous()),
                          g_image=_square_image(G, A.device), theta=float(np.float32(lambda_ / mu)), lambda_=lambda_, mu=mu, L=L, B=B)


def sparse_unmix(spectra: torch.Tensor, operands: SparseOperands, epsilon: float = 1e-4, max_iterations: int = 400,
                 want_residual: bool = True,
                 want_status: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """a = argmin 1/2 |x - A^T a|^2 + lambda sqrt(sum x^2) sum a over a >= 0 for every row of ``spectra`` (float32 [...,B], read in
    place as ``library_match`` reads them), by ADMM to the relative tolerance ``epsilon``.  Returns ``(abundances float32 [R,L],
    residual float32 [R] or None, status int32 [R] or None)``: residual = |x - A^T a|^2; status = the iterations used, -1 for an
    invalid row (a NaN, an Inf, all zeros: abundances 0), -2 for a row stopped at ``max_iterations``.  One launch, no host sync."""
    s, R, B, stride = _rows(spectra, "sparse_unmix")
    if not isinstance(operands, SparseOperands):
        raise ValueError("operands must come from sparse_prepare")
    if not 1 <= B <= SPARSE_MAX_BANDS or B != operands.B:
        raise ValueError(f"the operands belong to a library of {operands.L} entries x {operands.B} bands, the rows have {B} bands "
                         f"(the kernel's limits: 1..{SPARSE_MAX_ENTRIES} entries, 1..{SPARSE_MAX_BANDS} bands)")
    if operands.q_image.device != s.device:
        raise ValueError(f"the operands are on {operands.q_image.device}, the rows on {s.device}")
    epsilon, max_iterations = float(epsilon), int(max_iterations)
    if not epsilon > 0.0 or not np.isfinite(epsilon):
        raise ValueError(f"epsilon must be finite and > 0, got {epsilon}")
    if max_iterations < 1:
        raise ValueError(f"max_iterations must be at least 1, got {max_iterations}")
    L = operands.L
    abundances = torch.empty(R, L, dtype=torch.float32, device=s.device)
    residual = torch.empty(R, dtype=torch.float32, device=s.device) if want_residual else None
    status = torch.empty(R, dtype=torch.int32, device=s.device) if want_status else None
    _hip.check(_hip.lib().umhs_sparse_unmix(_hip.C.c_void_p(s.data_ptr()), stride, R, ptr(operands.q_image), ptr(operands.m_image),
                                            ptr(operands.a_image), ptr(operands.g_image), L, B, operands.theta, epsilon, max_iterations,
                                            ptr(abundances), ptr(residual), ptr(status), _hip.stream()), "umhs_sparse_unmix")
    return abundances, residual, status
