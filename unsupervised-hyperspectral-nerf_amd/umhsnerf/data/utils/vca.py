"""Vertex Component Analysis (mirror of ``umhsnerf/data/utils/vca.py``; Nascimento & Dias): the endmember initialisation the
reference runs on the first hyperspectral frame it loads (``hs_dataloader.py:52-58``) and hands to the field through ``vca.npy``
when ``load_vca`` is set (``umhs_field.py:78-81``).  Here the result is returned, not written to a file.

The work is split where the data is.  The three passes over all N pixels run on the GPU on the resident ``hs_image`` stack
(``ops.vca_moments`` / ``vca_project`` / ``vca_argmax``, csrc/umhs_vca.hip); everything between them is float64 NumPy on the host
and importable without a GPU: the B x B basis and the SNR estimate from the moments (``vca_plan``), the R-step recursion on the
R x R matrix ``A`` (``vca_select``) and the final ``Yp[:, indice]`` from the R chosen pixels (``vca_finish``).

The projection to R-1 dimensions that the reference means to take below the SNR threshold (``vca.py:98-116``) sits under
``if verbose:`` there, so its only caller (``verbose=False``) gets an ``UnboundLocalError`` and falls back to ``randn``; it is built
here as the published algorithm states it (branch ``"affine"``)."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

MAX_CLASSES, MAX_BANDS = 15, 256


def vca_plan(band_sum, S, n: int, num_classes: int) -> Dict:
    """Basis and branch from the moments ``band_sum [B] = sum_n y_n`` and ``S [B,B] = sum_n y_n y_n^T`` (``vca.py:76-129`` without
    its passes over the pixels: ``P_y = tr(S)/N`` and ``P_x = tr(Ud^T C0 Ud) + |m|^2``).  -> ``branch`` "projective" | "affine",
    ``snr``, ``snr_th``, ``Ud [B,d]``, ``mean [B]``, ``basis16 [B,16]`` (what ``ops.vca_project`` takes) -- all float64."""
    R, B, N = int(num_classes), int(S.shape[0]), float(n)
    if not 1 <= R <= min(B, MAX_CLASSES) or B > MAX_BANDS:
        raise ValueError(f"VCA needs 1 <= num_classes <= min(B, {MAX_CLASSES}) and B <= {MAX_BANDS}; got num_classes {R}, B {B}")
    band_sum, S = np.asarray(band_sum, np.float64), np.asarray(S, np.float64)
    m = band_sum / N
    C0 = S / N - np.outer(m, m)
    Ud = np.linalg.svd(C0)[0][:, :R]
    P_y = np.trace(S) / N
    P_x = np.trace(Ud.T @ C0 @ Ud) + np.sum(m ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        snr = float(10 * np.log10((P_x - R / B * P_y) / (P_y - P_x)))
    snr_th = float(15 + 10 * np.log10(R))
    basis16 = np.zeros((B, 16))
    if snr < snr_th:  # (a NaN estimate -- noise-free data -- takes the projective branch, as in the reference)
        Ud = Ud[:, : R - 1]
        basis16[:, : R - 1] = Ud
        return dict(branch="affine", snr=snr, snr_th=snr_th, Ud=Ud, mean=m, basis16=basis16, num_classes=R)
    Ud = np.linalg.svd(S / N)[0][:, :R]
    basis16[:, :R] = Ud
    basis16[:, 15] = Ud @ (Ud.T @ m)  # u = mean(x) = Ud^T m: the 16th dot product of a pixel is the denominator u^T x
    return dict(branch="projective", snr=snr, snr_th=snr_th, Ud=Ud, mean=m, basis16=basis16, num_classes=R)


def vca_select(plan: Dict, draws, argmax, max_sq: Optional[float] = None) -> np.ndarray:
    """The recursion of ``vca.py:136-158``: ``argmax(f [16], bias) -> (index, y_row [16])`` is the pass over the pixels;
    ``draws [R,R]``, column i = the reference's i-th ``np.random.rand(R, 1)``.  -> indices [R] int64."""
    R = plan["num_classes"]
    draws = np.asarray(draws, np.float64).reshape(R, R)
    affine = plan["branch"] == "affine"
    c = float(np.sqrt(max_sq)) if affine else 0.0
    A = np.zeros((R, R))
    A[-1, 0] = 1
    indices = np.zeros(R, np.int64)
    for i in range(R):
        w = draws[:, i : i + 1]
        f = w - A @ (np.linalg.pinv(A) @ w)
        f = (f / np.linalg.norm(f) + 1e-6)[:, 0]
        f16 = np.zeros(16)
        if affine:  # y = [x; c]: the constant last component enters the pass as a bias
            f16[: R - 1] = f[: R - 1]
            idx, row = argmax(f16, float(f[R - 1] * c))
            A[:, i] = np.append(np.asarray(row, np.float64)[: R - 1], c)
        else:
            f16[:R] = f
            idx, row = argmax(f16, 0.0)
            A[:, i] = np.asarray(row, np.float64)[:R]
        indices[i] = idx
    return indices


def vca_finish(plan: Dict, pixels) -> np.ndarray:
    """``Yp[:, indice]^T`` [R,B] from the R chosen pixels [R,B]: their projection onto the basis (``vca.py:112,125,160``)."""
    Y, Ud = np.asarray(pixels, np.float64), plan["Ud"]
    if plan["branch"] == "affine":
        return ((Y - plan["mean"]) @ Ud) @ Ud.T + plan["mean"]
    return (Y @ Ud) @ Ud.T


def reference_draws(num_classes: int, seed: Optional[int] = None) -> np.ndarray:
    """[R,R], column i = the i-th ``rand(R, 1)`` of a ``numpy.random.RandomState(seed)``: the stream the reference consumes after
    ``np.random.seed(seed)``."""
    rs = np.random.RandomState(seed)
    return np.concatenate([rs.rand(num_classes, 1) for _ in range(num_classes)], axis=1)


class HipPasses:
    """The three passes on the GPU over a list of frames ``[n_i, B]`` (fp32; on the device, or on the host: then one frame at a
    time is uploaded for each pass).  Each frame is one ``vca_moments(accumulate)`` call whether the stack is resident or not, so
    both give the same bits."""

    def __init__(self, frames: Sequence[torch.Tensor], device):
        from ... import ops

        self.ops, self.device = ops, torch.device(device)
        self.frames = [f for f in frames if f.shape[0] > 0]
        if not self.frames:
            raise ValueError("VCA needs at least one pixel")
        self.bands = int(self.frames[0].shape[1])
        self.offsets = np.cumsum([0] + [int(f.shape[0]) for f in self.frames])
        self.n = int(self.offsets[-1])
        self.y = None

    def _up(self, f: torch.Tensor) -> torch.Tensor:
        return f.to(self.device, torch.float32).contiguous()

    def moments(self) -> Tuple[np.ndarray, np.ndarray, int]:
        s = S = None
        for f in self.frames:
            s, S = self.ops.vca_moments(self._up(f), s, S)
        return s.cpu().numpy(), S.cpu().numpy(), self.n

    def project(self, plan: Dict) -> Optional[float]:
        affine = plan["branch"] == "affine"
        basis = torch.from_numpy(plan["basis16"]).to(self.device, torch.float32)
        mean = torch.from_numpy(plan["mean"]).to(self.device, torch.float32) if affine else None
        self.y = torch.empty(self.n, 16, device=self.device, dtype=torch.float32)
        best = None
        for k, f in enumerate(self.frames):
            _, mx = self.ops.vca_project(self._up(f), basis, plan["num_classes"], mean, out=self.y[self.offsets[k] : self.offsets[k + 1]])
            if affine:
                best = mx if best is None else torch.maximum(best, mx)
        return float(best) if affine else None

    def argmax(self, f16, bias: float):
        index, row, _ = self.ops.vca_argmax(self.y, f16, bias)
        return int(index), row.cpu().numpy()

    def pixels(self, indices) -> np.ndarray:
        out = []
        for i in indices:
            k = int(np.searchsorted(self.offsets, i, side="right")) - 1
            out.append(self.frames[k][int(i - self.offsets[k])].detach().cpu().numpy().astype(np.float64))
        return np.stack(out)


def run_vca(passes, num_classes: int, draws=None, seed: Optional[int] = None):
    """VCA over whatever ``passes`` holds (``HipPasses``; the tests drive the same host code with float64 stand-ins)."""
    band_sum, S, n = passes.moments()
    plan = vca_plan(band_sum, S, n, num_classes)
    max_sq = passes.project(plan)
    if draws is None:
        draws = reference_draws(num_classes, seed)
    indices = vca_select(plan, draws, passes.argmax, max_sq)
    E = vca_finish(plan, passes.pixels(indices))
    info = {"snr": plan["snr"], "snr_th": plan["snr_th"], "branch": plan["branch"]}
    return torch.from_numpy(E.astype(np.float32)), torch.from_numpy(indices), info


def as_frames(rows_or_stack: torch.Tensor) -> List[torch.Tensor]:
    """[N,B] rows -> one frame; [H,W,B] -> one frame; [n,H,W,B] -> n frames of H*W rows."""
    t = rows_or_stack
    if not torch.is_tensor(t):
        t = torch.as_tensor(np.asarray(t))
    if t.dim() not in (2, 3, 4):
        raise ValueError(f"expected pixel rows [N,B], a frame [H,W,B] or a stack [n,H,W,B]; got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        t = t.float()
    if t.dim() == 4:
        return [t[i].reshape(-1, t.shape[-1]) for i in range(t.shape[0])]
    return [t.reshape(-1, t.shape[-1])]


def vca_endmembers(rows_or_stack, num_classes: int, draws=None, seed: Optional[int] = None, device=None):
    """-> (endmembers [R,B] fp32, indices [R] int64 -- rows of the flattened input --, info {snr, snr_th, branch}).
    ``draws [R,R]`` (column i = w_i) replays a given stream; otherwise ``reference_draws(num_classes, seed)``."""
    frames = as_frames(rows_or_stack)
    if device is None:
        device = frames[0].device if frames[0].is_cuda else torch.device("cuda", torch.cuda.current_device())
    return run_vca(HipPasses(frames, device), num_classes, draws, seed)
